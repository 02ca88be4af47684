// Micro-benchmark: fp32-accurate layer chains on bf16 MFMA (each operand split into three bf16
// parts, the six products down to 2^-16 relative, fp32 accumulate) vs plain f32 MFMA.
// 16 activation columns per wave, 128 -> 128 layers, weights as the A operand.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short shortx8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int lane_id() {
    int l = threadIdx.x & 63;
    asm volatile("" : "+v"(l));
    return l;
}

struct Split3 { bf16x8 h, m, l; };

// 8 fp32 -> hi/mid/lo bf16 parts
__device__ __forceinline__ Split3 split8(const float (&v)[8]) {
    Split3 s;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)v[j];
        const float r = v[j] - (float)h;
        const __bf16 m = (__bf16)r;
        const float r2 = r - (float)m;
        s.h[j] = h;
        s.m[j] = m;
        s.l[j] = (__bf16)r2;
    }
    return s;
}

#define MF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)

// y (8 tiles) = W (128x128, packed [t][kk][part][lane] bf16x8) * x (8 tiles)
template <int SPLITS>
__device__ __forceinline__ void layer_split(const bf16x8 *w, const floatx4 (&x)[8], floatx4 (&y)[8]) {
    Split3 xs[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const float v[8] = {x[2 * kk][0], x[2 * kk][1], x[2 * kk][2], x[2 * kk][3],
                            x[2 * kk + 1][0], x[2 * kk + 1][1], x[2 * kk + 1][2], x[2 * kk + 1][3]};
        xs[kk] = split8(v);
    }
    const bf16x8 *wp = w + lane_id();
    constexpr int N = 32, D = 2;   // (t, kk) steps, prefetch depth
    bf16x8 bh[D], bm[D], bl[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        bh[i] = wp[(i * 3 + 0) * 64];
        bm[i] = wp[(i * 3 + 1) * 64];
        bl[i] = wp[(i * 3 + 2) * 64];
    }
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int t = i / 4, kk = i % 4;
        const bf16x8 ah = bh[i % D], am = bm[i % D], al = bl[i % D];
        if (i + D < N) {
            bh[i % D] = wp[((i + D) * 3 + 0) * 64];
            bm[i % D] = wp[((i + D) * 3 + 1) * 64];
            bl[i % D] = wp[((i + D) * 3 + 2) * 64];
        }
        if (kk == 0) acc = floatx4{0.f, 0.f, 0.f, 0.f};
        acc = MF(ah, xs[kk].h, acc);
        acc = MF(ah, xs[kk].m, acc);
        acc = MF(am, xs[kk].h, acc);
        if (SPLITS == 6) {
            acc = MF(ah, xs[kk].l, acc);
            acc = MF(al, xs[kk].h, acc);
            acc = MF(am, xs[kk].m, acc);
        }
        if (kk == 3) y[t] = acc;
        __builtin_amdgcn_sched_barrier(0);
    }
}


// 6 products, output tiles processed in pairs with interleaved accumulators
__device__ __forceinline__ void layer_split_pair(const bf16x8 *w, const floatx4 (&x)[8], floatx4 (&y)[8]) {
    Split3 xs[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const float v[8] = {x[2 * kk][0], x[2 * kk][1], x[2 * kk][2], x[2 * kk][3],
                            x[2 * kk + 1][0], x[2 * kk + 1][1], x[2 * kk + 1][2], x[2 * kk + 1][3]};
        xs[kk] = split8(v);
    }
    const bf16x8 *wp = w + lane_id();
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
        floatx4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int f0 = (2 * tp) * 4 + kk, f1 = (2 * tp + 1) * 4 + kk;
            const bf16x8 h0 = wp[(f0 * 3 + 0) * 64], m0 = wp[(f0 * 3 + 1) * 64], l0 = wp[(f0 * 3 + 2) * 64];
            const bf16x8 h1 = wp[(f1 * 3 + 0) * 64], m1 = wp[(f1 * 3 + 1) * 64], l1 = wp[(f1 * 3 + 2) * 64];
            a0 = MF(h0, xs[kk].h, a0); a1 = MF(h1, xs[kk].h, a1);
            a0 = MF(h0, xs[kk].m, a0); a1 = MF(h1, xs[kk].m, a1);
            a0 = MF(m0, xs[kk].h, a0); a1 = MF(m1, xs[kk].h, a1);
            a0 = MF(h0, xs[kk].l, a0); a1 = MF(h1, xs[kk].l, a1);
            a0 = MF(l0, xs[kk].h, a0); a1 = MF(l1, xs[kk].h, a1);
            a0 = MF(m0, xs[kk].m, a0); a1 = MF(m1, xs[kk].m, a1);
        }
        y[2 * tp] = a0;
        y[2 * tp + 1] = a1;
    }
}

__device__ __forceinline__ void layer_f32(const float4 *w, const floatx4 (&x)[8], floatx4 (&y)[8]) {
    const float4 *wp = w + lane_id();
    constexpr int N = 64, D = 3;
    float4 buf[D];
#pragma unroll
    for (int i = 0; i < D; ++i) buf[i] = wp[i * 64];
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int t = i / 8, q = i % 8;
        const float4 wv = buf[i % D];
        if (i + D < N) buf[i % D] = wp[(i + D) * 64];
        if (q == 0) acc = floatx4{0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, x[q].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, x[q].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, x[q].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, x[q].w, acc, 0, 0, 0);
        if (q == 7) y[t] = acc;
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int MODE>   // 0: f32, 3: bf16 x3 (3 products), 6: bf16 x3 (6 products)
__global__ void __launch_bounds__(256, 2) chain(const void *w, int iters, float *out) {
    extern __shared__ float lds_pad[];
    if (threadIdx.x == 0) lds_pad[0] = 0.f;
    floatx4 x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = floatx4{1e-3f * q, 1e-3f, 2e-3f, 3e-3f};
#pragma nounroll
    for (int it = 0; it < iters; ++it) {
        floatx4 y[8];
        if (MODE == 0) layer_f32(reinterpret_cast<const float4 *>(w) + (it & 3) * 64 * 64, x, y);
        else if (MODE == 7) layer_split_pair(reinterpret_cast<const bf16x8 *>(w) + (it & 3) * 8 * 4 * 3 * 64, x, y);
        else layer_split<MODE>(reinterpret_cast<const bf16x8 *>(w) + (it & 3) * 8 * 4 * 3 * 64, x, y);
#pragma unroll
        for (int t = 0; t < 8; ++t)
            x[t] = floatx4{fmaxf(y[t][0], 0.f) + 1e-3f, fmaxf(y[t][1], 0.f), fmaxf(y[t][2], 0.f), fmaxf(y[t][3], 0.f)};
    }
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += x[q][0] + x[q][1] + x[q][2] + x[q][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int MODE>
static void run(const char *name, const void *w, float *out, int blocks, int iters, int lds) {
    hipFuncSetAttribute((const void *)chain<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    chain<MODE><<<blocks, 256, lds>>>(w, iters, out);
    hipDeviceSynchronize();
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    hipEventRecord(a);
    const int reps = 5;
    for (int r = 0; r < reps; ++r) chain<MODE><<<blocks, 256, lds>>>(w, iters, out);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    ms /= reps;
    const double flop = 2.0 * 128 * 128 * 16 * (double)iters * blocks * 4;   // fp32-equivalent
    printf("%-18s lds=%6d  %.3f ms  %.1f TFLOP/s (fp32-equivalent)\n", name, lds, ms, flop / ms / 1e9);
}

// ---- lin_event-shaped case: K = 192 generated features cos(dt w + phi) (fp64 range reduction + v_cos_f32, as
// walk_kernel's cos_rd), 11 output tiles, weight fragments streamed from L2, the next K step's features
// generated between this step's MFMAs.  MODE 0: v_mfma_f32_16x16x4_f32, 12 K steps of 16 (4 features per lane
// per step); MODE 6: v_mfma_f32_16x16x32_bf16, 6 K steps of 32 (8 features per lane per step, split in
// registers), six products per (tile, step), tile pairs interleaved.
__device__ __forceinline__ float cos_feat(float dt, int k) {
    const float x = dt * (1.0f / (float)(1 + k)) + 0.01f * (float)k;
    const double u = (double)x * 0.15915494309189533577;
    return __builtin_amdgcn_cosf((float)(u - __builtin_rint(u)));
}

template <int MODE>
__global__ void __launch_bounds__(256, 2) lin_ev(const void *w, int iters, float *out) {
    constexpr int NT = 11;
    const int g = lane_id() >> 4;
    floatx4 L[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) L[t] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma nounroll
    for (int it = 0; it < iters; ++it) {
        const float dt = 1e3f * (float)(it + 1) + (float)(threadIdx.x & 15);
        if constexpr (MODE == 0) {
            const float4 *wp = reinterpret_cast<const float4 *>(w) + lane_id();
            constexpr int NQ = 12, N = NT * NQ, D = 4;
            float4 buf[D];
#pragma unroll
            for (int i = 0; i < D; ++i) buf[i] = wp[((i % NT) * NQ + i / NT) * 64];
            floatx4 xq;
#pragma unroll
            for (int s = 0; s < 4; ++s) xq[s] = cos_feat(dt, 4 * g + s);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                floatx4 xn = xq;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int i = q * NT + t;
                    const float4 a = buf[i % D];
                    if (i + D < N) buf[i % D] = wp[(((i + D) % NT) * NQ + (i + D) / NT) * 64];
                    L[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, xq.x, L[t], 0, 0, 0);
                    L[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, xq.y, L[t], 0, 0, 0);
                    L[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, xq.z, L[t], 0, 0, 0);
                    L[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, xq.w, L[t], 0, 0, 0);
                    if (q + 1 < NQ && t < 4) xn[t] = cos_feat(dt, 16 * (q + 1) + 4 * g + t);
                    __builtin_amdgcn_sched_barrier(0);
                }
                xq = xn;
            }
        } else {
            const bf16x8 *wp = reinterpret_cast<const bf16x8 *>(w) + lane_id();
            constexpr int NS = 6, N = NT * NS * 3, D = 12;
            auto off = [](int i) { return ((((i / 3) % NT) * NS + i / (3 * NT)) * 3 + i % 3) * 64; };
            bf16x8 buf[D];
#pragma unroll
            for (int i = 0; i < D; ++i) buf[i] = wp[off(i)];
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = cos_feat(dt, 8 * g + j);
            Split3 xs = split8(v);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float vn[8] = {};
                auto take = [&](int i) {
                    const bf16x8 a = buf[i % D];
                    if (i + D < N) buf[i % D] = wp[off(i + D)];
                    return a;
                };
#pragma unroll
                for (int t = 0; t < NT; t += 2) {
                    const int i = (s * NT + t) * 3;
                    const bool two = t + 1 < NT;
                    const bf16x8 h0 = take(i), m0 = take(i + 1), l0 = take(i + 2);
                    bf16x8 h1 = h0, m1 = m0, l1 = l0;
                    if (two) h1 = take(i + 3), m1 = take(i + 4), l1 = take(i + 5);
                    const int u = two ? t + 1 : t;
                    L[t] = MF(l0, xs.h, L[t]); if (two) L[u] = MF(l1, xs.h, L[u]);
                    L[t] = MF(h0, xs.l, L[t]); if (two) L[u] = MF(h1, xs.l, L[u]);
                    L[t] = MF(m0, xs.m, L[t]); if (two) L[u] = MF(m1, xs.m, L[u]);
                    L[t] = MF(m0, xs.h, L[t]); if (two) L[u] = MF(m1, xs.h, L[u]);
                    L[t] = MF(h0, xs.m, L[t]); if (two) L[u] = MF(h1, xs.m, L[u]);
                    L[t] = MF(h0, xs.h, L[t]); if (two) L[u] = MF(h1, xs.h, L[u]);
                    if (s + 1 < NS && t < 8) {
                        vn[t] = cos_feat(dt, 32 * (s + 1) + 8 * g + t);
                        vn[t + 1] = cos_feat(dt, 32 * (s + 1) + 8 * g + t + 1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (s + 1 < NS) xs = split8(vn);
            }
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) sum += L[t][0] + L[t][1] + L[t][2] + L[t][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = sum;
}

template <int MODE>
static void run_lin_ev(const char *name, const void *w, float *out, int blocks, int iters) {
    lin_ev<MODE><<<blocks, 256>>>(w, iters, out);
    hipDeviceSynchronize();
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    hipEventRecord(a);
    const int reps = 5;
    for (int r = 0; r < reps; ++r) lin_ev<MODE><<<blocks, 256>>>(w, iters, out);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    ms /= reps;
    const double flop = 2.0 * 192 * 176 * 16 * (double)iters * blocks * 4;   // fp32-equivalent
    printf("lin_event %-16s %.3f ms  %.1f TFLOP/s (fp32-equivalent), %.0f ns per 16-column pass\n", name, ms,
           flop / ms / 1e9, ms * 1e6 / iters);
}

// ---- event_gcn-shaped case (zero-node form): H[4 tiles] = bias + G1 relu(L) over K = 176 (11 input tiles in the D-tile
// lane order the previous layer leaves them in), weight fragments streamed from L2, 2 waves per SIMD.  MODE 0:
// v_mfma_f32_16x16x4_f32, 11 K steps, a step's 4 fragments two steps ahead (walk_kernel's form before the split);
// MODE 6: v_mfma_f32_16x16x32_bf16 over 6 pair steps of two input tiles (the B operand split in registers from the
// tile pair, the second half of the last step zero), six products per (tile, step), tile pairs interleaved, all 72
// fragments streamed through a 12-deep ring; MODE 7: the same with the first 3 pair steps' 36 fragments resident in
// LDS (copied once per workgroup), streamed and resident steps alternating.
constexpr int evg_step(int k, int gl, int ns) {
    const int nstr = ns - gl, m = nstr < gl ? nstr : gl;
    if (k < 2 * m) return (k & 1) ? k / 2 : gl + k / 2;
    return nstr > gl ? gl + k - m : k - m;
}

template <int MODE>
__global__ void __launch_bounds__(256, 2) ev_gcn(const void *w, int iters, float *out) {
    constexpr int NT = 11, NS = 6, GL = MODE == 7 ? 3 : 0;
    __shared__ float4 gl[MODE == 7 ? GL * 12 * 64 : 1];
    extern __shared__ float lds_pad[];   // sized by the launch so that two workgroups fill a CU (2 waves per SIMD)
    if (threadIdx.x == 0) lds_pad[0] = 0.f;
    if constexpr (MODE == 7) {
        for (int i = threadIdx.x; i < GL * 12 * 64; i += blockDim.x) {
            const int f = i >> 6, l = i & 63;
            gl[i] = reinterpret_cast<const float4 *>(w)[((((f / 3) % 4) * NS + f / 12) * 3 + f % 3) * 64 + l];
        }
        __syncthreads();
    }
    floatx4 H[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) H[t] = floatx4{1e-3f * t, 1e-3f, 2e-3f, 3e-3f};
#pragma nounroll
    for (int it = 0; it < iters; ++it) {
        floatx4 L[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const float c = 1e-3f * (float)(q - 5);
            L[q] = floatx4{H[q & 3][0] + c, H[q & 3][1] - c, H[q & 3][2] + c, H[q & 3][3] - c};
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) H[t] = floatx4{1e-3f, 2e-3f, 3e-3f, 4e-3f};
        if constexpr (MODE == 0) {
            const float4 *wp = reinterpret_cast<const float4 *>(w) + lane_id();
            float4 wz[3][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                wz[0][t] = wp[(t * NT + 0) * 64];
                wz[1][t] = wp[(t * NT + 1) * 64];
            }
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                if (q + 2 < NT) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) wz[(q + 2) % 3][t] = wp[(t * NT + q + 2) * 64];
                }
                floatx4 A;
#pragma unroll
                for (int r = 0; r < 4; ++r) A[r] = 0.f + fmaxf(0.f + L[q][r], 0.f);
#pragma unroll
                for (int t = 0; t < 4; ++t) H[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[q % 3][t].x, A.x, H[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) H[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[q % 3][t].y, A.y, H[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) H[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[q % 3][t].z, A.z, H[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) H[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[q % 3][t].w, A.w, H[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            const float4 *wp = reinterpret_cast<const float4 *>(w) + lane_id();
            const int ln = lane_id();
            constexpr int N = (NS - GL) * 12, D = 12;
            auto off = [](int i) { return ((((i / 3) % 4) * NS + GL + i / 12) * 3 + i % 3) * 64; };
            float4 buf[D];
#pragma unroll
            for (int i = 0; i < D; ++i) buf[i] = wp[off(i)];
            auto take = [&](int i) {
                const float4 a = buf[i % D];
                if (i + D < N) buf[i % D] = wp[off(i + D)];
                return a;
            };
            auto fetch = [&](int p, float4 (&f)[6]) {
                const int u = evg_step(p / 2, GL, NS), t = 2 * (p & 1);
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (u < GL) f[k] = gl[((u * 4 + t) * 3 + k) * 64 + ln];
                    else f[k] = take(((u - GL) * 4 + t) * 3 + k);
                }
            };
            auto act = [&](float (&v)[8], int u, int j) {
                const int q = 2 * u + (j >> 2);
                v[j] = q < NT ? 0.f + fmaxf(0.f + L[q < NT ? q : 0][j & 3], 0.f) : 0.f;
            };
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) act(v, evg_step(0, GL, NS), j);
            Split3 xb = split8(v);
            float4 wb[2][6];
            fetch(0, wb[0]);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                float vn[8] = {};
#pragma unroll
                for (int t = 0; t < 4; t += 2) {
                    const int pp = 2 * k + t / 2;
                    if (pp + 1 < 2 * NS) fetch(pp + 1, wb[(pp + 1) & 1]);
                    const float4(&f)[6] = wb[pp & 1];
                    const bf16x8 h0 = __builtin_bit_cast(bf16x8, f[0]), m0 = __builtin_bit_cast(bf16x8, f[1]),
                                 l0 = __builtin_bit_cast(bf16x8, f[2]), h1 = __builtin_bit_cast(bf16x8, f[3]),
                                 m1 = __builtin_bit_cast(bf16x8, f[4]), l1 = __builtin_bit_cast(bf16x8, f[5]);
                    H[t] = MF(l0, xb.h, H[t]); H[t + 1] = MF(l1, xb.h, H[t + 1]);
                    H[t] = MF(h0, xb.l, H[t]); H[t + 1] = MF(h1, xb.l, H[t + 1]);
                    H[t] = MF(m0, xb.m, H[t]); H[t + 1] = MF(m1, xb.m, H[t + 1]);
                    H[t] = MF(m0, xb.h, H[t]); H[t + 1] = MF(m1, xb.h, H[t + 1]);
                    H[t] = MF(h0, xb.m, H[t]); H[t + 1] = MF(h1, xb.m, H[t + 1]);
                    H[t] = MF(h0, xb.h, H[t]); H[t + 1] = MF(h1, xb.h, H[t + 1]);
                    if (k + 1 < NS) {
#pragma unroll
                        for (int j = 2 * t; j < 2 * t + 4; ++j) act(vn, evg_step(k + 1, GL, NS), j);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (k + 1 < NS) xb = split8(vn);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            H[t] = floatx4{fmaxf(H[t][0], 0.f), fmaxf(H[t][1], 0.f), fmaxf(H[t][2], 0.f), fmaxf(H[t][3], 0.f)};
    }
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) sum += H[t][0] + H[t][1] + H[t][2] + H[t][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = sum;
}

template <int MODE>
static void run_ev_gcn(const char *name, const void *w, float *out, int blocks, int iters) {
    const int lds = (MODE == 7 ? 24 : 60) * 1024;
    ev_gcn<MODE><<<blocks, 256, lds>>>(w, iters, out);
    hipDeviceSynchronize();
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    hipEventRecord(a);
    const int reps = 5;
    for (int r = 0; r < reps; ++r) ev_gcn<MODE><<<blocks, 256, lds>>>(w, iters, out);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    ms /= reps;
    const double flop = 2.0 * 176 * 64 * 16 * (double)iters * blocks * 4;   // fp32-equivalent
    printf("event_gcn %-24s %.3f ms  %.1f TFLOP/s (fp32-equivalent), %.0f ns per 16-column pass\n", name, ms,
           flop / ms / 1e9, ms * 1e6 / iters);
}

int main() {
    void *w;
    const size_t bytes = 4 * 8 * 4 * 3 * 64 * 16;   // 4 layers, bf16x3 packing (largest)
    hipMalloc(&w, bytes);
    std::vector<unsigned short> h(bytes / 2);
    for (size_t i = 0; i < h.size(); ++i) h[i] = 0x3a80 + (i % 13);   // small bf16 / f32 halves
    hipMemcpy(w, h.data(), bytes, hipMemcpyHostToDevice);
    float *out;
    const int blocks = 256 * 2 * 8;
    hipMalloc(&out, sizeof(float) * blocks * 256);
    for (int lds : {64 * 1024, 100 * 1024}) {
        run<0>("f32 16x16x4", w, out, blocks, 200, lds);
        run<6>("bf16x3 6-prod", w, out, blocks, 200, lds);
        run<3>("bf16x3 3-prod", w, out, blocks, 200, lds);
        run<7>("bf16x3 6-prod pair", w, out, blocks, 200, lds);
    }
    run_lin_ev<0>("f32 16x16x4", w, out, blocks, 200);
    run_lin_ev<6>("bf16x3 6-prod", w, out, blocks, 200);
    run_ev_gcn<0>("f32 16x16x4", w, out, blocks, 600);
    run_ev_gcn<6>("bf16x3 6-prod streamed", w, out, blocks, 600);
    run_ev_gcn<7>("bf16x3 6-prod half in LDS", w, out, blocks, 600);
    return 0;
}
