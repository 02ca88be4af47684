// Micro-benchmark: the vector-issue price of single VALU instructions beside bf16 MFMAs (sibling of valu.hip).
// Two waves per SIMD (256-thread workgroups, two per CU) each run a chain of v_mfma_f32_16x16x32_bf16 over four
// independent accumulators from register operands (no loads); after every MFMA come NF independent filler
// instructions of one kind, written as inline assembly so that the instruction measured is the one named:
//   the five fp64 instructions of cos_rd's range reduction (v_cvt_f64_f32, v_mul_f64, v_rndne_f64, v_fma_f64,
//   v_cvt_f32_f64), v_cos_f32, v_cvt_pk_bf16_f32, v_pk_add_f32 against two v_add_f32 (the same two sums).
// Printed per case: shader cycles (s_memtime) per MFMA slot of one wave, and the difference to the bare chain divided
// by NF = the cycles one filler adds to a wave's slot.  The last rows are the bare chains of the 32-deep and of the
// 16-deep (v_mfma_f32_16x16x16_bf16) form.  Build: hipcc --offload-arch=gfx950 -O3 micro/valu_issue.hip -o micro/valu_issue
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short shortx4 __attribute__((ext_vector_type(4)));

enum Kind { NONE, CVT_F64_F32, MUL_F64, RNDNE_F64, FMA_F64, CVT_F32_F64, COS_F32, CVT_PK_BF16, PK_ADD, ADD2, N_KIND };
static const char *NAMES[N_KIND] = {"none", "v_cvt_f64_f32", "v_mul_f64", "v_rndne_f64", "v_fma_f64", "v_cvt_f32_f64",
                                    "v_cos_f32", "v_cvt_pk_bf16_f32", "v_pk_add_f32", "2 x v_add_f32"};

template <int K>
__device__ __forceinline__ void filler(float f, double d, floatx2 p, float &of, double &od, floatx2 &op) {
    if constexpr (K == CVT_F64_F32) asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(od) : "v"(f));
    if constexpr (K == MUL_F64) asm volatile("v_mul_f64 %0, %1, %1" : "=v"(od) : "v"(d));
    if constexpr (K == RNDNE_F64) asm volatile("v_rndne_f64 %0, %1" : "=v"(od) : "v"(d));
    if constexpr (K == FMA_F64) asm volatile("v_fma_f64 %0, %1, %1, %1" : "=v"(od) : "v"(d));
    if constexpr (K == CVT_F32_F64) asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(of) : "v"(d));
    if constexpr (K == COS_F32) asm volatile("v_cos_f32 %0, %1" : "=v"(of) : "v"(f));
    if constexpr (K == CVT_PK_BF16) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %1" : "=v"(of) : "v"(f));
    if constexpr (K == PK_ADD) asm volatile("v_pk_add_f32 %0, %1, %1" : "=v"(op) : "v"(p));
    if constexpr (K == ADD2) {
        asm volatile("v_add_f32 %0, %1, %1" : "=v"(of) : "v"(f));
        asm volatile("v_add_f32 %0, %1, %1" : "=v"(op.x) : "v"(f));
    }
}

// K: the filler, NF: fillers per MFMA, D16: the 16-deep MFMA.  cyc[wave] = s_memtime cycles of the wave's loop.
template <int K, int NF, bool D16>
__global__ void __launch_bounds__(256) kern(int iters, float seed, float *out, unsigned long long *cyc) {
    floatx4 acc[4];
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = (__bf16)(seed * (float)(j + 1));
        b[j] = (__bf16)(seed * (float)(threadIdx.x & 7));
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float f = seed + (float)threadIdx.x;
    const double d = f;
    const floatx2 p = {f, seed};
    float of[4] = {};
    double od[4] = {};
    floatx2 op[4] = {};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma nounroll
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if constexpr (D16) {
                const shortx4 a4 = __builtin_bit_cast(shortx4, __builtin_shufflevector(a, a, 0, 1, 2, 3));
                const shortx4 b4 = __builtin_bit_cast(shortx4, __builtin_shufflevector(b, b, 0, 1, 2, 3));
                acc[u & 3] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a4, b4, acc[u & 3], 0, 0, 0);
            } else {
                acc[u & 3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[u & 3], 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < NF; ++v) filler<K>(f, d, p, of[v & 3], od[v & 3], op[v & 3]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) s += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3] + of[t] + (float)od[t] + op[t].x + op[t].y;
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) cyc[(blockIdx.x * blockDim.x + threadIdx.x) >> 6] = t1 - t0;
}

static float *g_out;
static unsigned long long *g_cyc;
static const int BLOCKS = 512, ITERS = 2000;   // 512 workgroups of 4 waves on 256 CUs: 2 waves per SIMD, one round

template <int K, int NF, bool D16>
static double run() {
    const int waves = BLOCKS * 4;
    kern<K, NF, D16><<<BLOCKS, 256>>>(ITERS, 1e-3f, g_out, g_cyc);
    kern<K, NF, D16><<<BLOCKS, 256>>>(ITERS, 1e-3f, g_out, g_cyc);
    if (hipDeviceSynchronize() != hipSuccess) {
        printf("launch failed\n");
        exit(1);
    }
    std::vector<unsigned long long> h(waves);
    (void)hipMemcpy(h.data(), g_cyc, sizeof(unsigned long long) * waves, hipMemcpyDeviceToHost);
    double sum = 0;
    for (auto c : h) sum += (double)c;
    return sum / waves / ((double)ITERS * 16);
}

template <int K>
static void price(double base) {
    const double c1 = run<K, 1, false>(), c2 = run<K, 2, false>(), c4 = run<K, 4, false>();
    printf("%-20s per MFMA slot: 1 filler %.2f, 2 fillers %.2f, 4 fillers %.2f cycles; per filler %+.2f / %+.2f / %+.2f\n", NAMES[K], c1,
           c2, c4, c1 - base, (c2 - base) / 2, (c4 - base) / 4);
}

int main() {
    (void)hipMalloc(&g_out, sizeof(float) * BLOCKS * 256);
    (void)hipMalloc(&g_cyc, sizeof(unsigned long long) * BLOCKS * 4);
    for (int rep = 0; rep < 2; ++rep) {
        const double base = run<NONE, 0, false>(), base16 = run<NONE, 0, true>();
        printf("== round %d: s_memtime cycles per MFMA slot of one wave, two waves per SIMD\n", rep + 1);
        printf("bare v_mfma_f32_16x16x32_bf16 chain %.2f, bare v_mfma_f32_16x16x16_bf16 chain %.2f\n", base, base16);
        price<CVT_F64_F32>(base);
        price<MUL_F64>(base);
        price<RNDNE_F64>(base);
        price<FMA_F64>(base);
        price<CVT_F32_F64>(base);
        price<COS_F32>(base);
        price<CVT_PK_BF16>(base);
        price<PK_ADD>(base);
        price<ADD2>(base);
    }
    return 0;
}
