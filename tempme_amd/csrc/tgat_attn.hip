// Base-TGAT temporal attention with explanation weights, and the fused layer tail, on gfx950
// (the consumer of TempME.retrieve_edge_imp_node: temp_exp_main.py:609-616 feeds the per-side
// (hop-1, hop-2) weights into TGAT.contrast(if_explain=True)).
//
// Reference (dharunm236/TempME, TGAT/TGAT.py):
//   forward_msg :607-619 / forward_msg_layer :678-706  three attention passes per side (DESIGN.md "TGAT contrast")
//   AttnModel :362-386            query = [src | 0 (d_edge) | src_t], key = value = [ngh | edge | ngh_t],
//                                 then MergeLayer(LayerNorm(fc(out) + query), src)
//   MultiHeadAttention :110-137   d_model = d_node + d_edge + d_time, per-head width d_model / n_head,
//                                 mask and explanation weight .repeat(n_head, 1, 1) (:128-130)
//   ScaledDotProductAttention :64-80  bmm / temperature, masked_fill(-1e10), softmax, * weight, bmm with v
//   TimeEncode :230-241           cos(t * basis_freq + phase): a multiply and then an in-place add, two
//                                 fp32 roundings (TGN's Linear(1, d) rounds once)
//
// The attention kernels use the folded formulation of tgn_attn.hip: qf_h = W_k,h^T W_q,h query is
// supplied per source row, the kernel builds every key on the fly from the tables and produces
// z_h = sum_j softmax(s)_j ew_j key_j; (fc W_v) z follows in the tail.  One 64-lane wave per source
// row, key element c = lane + 64 i in register i.  They differ from the TGN kernels in the time
// feature's rounding and in the backward, which also returns the gradient of qf: TGAT's second layer
// queries with the first layer's output, which depends on the explanation weights.
// The kernels are a separate set on purpose: the TGN kernels keep their code and bitwise results.
#include "tgat_common.h"

namespace tmk {
namespace tgat {

// one online-softmax step of head state (m, l, acc) with key k
template <int KPL>
__device__ __forceinline__ void att_step(const tm_tgat_attn &a, const float q[KPL], const float k[KPL], int64_t ms,
                                         float &m, float &l, float acc[KPL]) {
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < KPL; ++i) p = __builtin_fmaf(q[i], k[i], p);
    float s = wave_sum(p) / a.temperature;
    if (a.mask_node[ms] == 0) s = -1e10f;
    const float e = a.ew ? a.ew[ms] : 1.f;
    const float mn = fmaxf(m, s);
    const float sc = expf(m - mn), w = expf(s - mn);
    l = l * sc + w;
    const float we = w * e;
#pragma unroll
    for (int i = 0; i < KPL; ++i) acc[i] = __builtin_fmaf(we, k[i], acc[i] * sc);
    m = mn;
}

// n_ngh < ATT_WAVES: one wave per row walks all its neighbours
template <int KPL, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) tgat_attn_fwd_kernel(tm_tgat_attn a, float *__restrict__ z,
                                                                       float *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * ATT_WAVES + (threadIdx.x >> 6);
    if (r >= a.rows) return;
    const int H = a.n_head, N = a.n_ngh, dk = a.d_node + a.d_edge + a.d_time;
    const KeyLane<KPL> L = key_lane<KPL>(a, lane);
    float q[HM][KPL], acc[HM][KPL], m[HM], l[HM];
    int64_t mr[HM];
#pragma unroll
    for (int h = 0; h < HM; ++h) {
        m[h] = -__builtin_inff();
        l[h] = 0.f;
        mr[h] = h < H ? pair_row(a, r, h) : 0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int c = lane + 64 * i;
            q[h][i] = (h < H && c < dk) ? a.qf[(r * H + h) * dk + c] : 0.f;
            acc[h][i] = 0.f;
        }
    }
    for (int j = 0; j < N; ++j) {
        float k[KPL];
        build_key<KPL>(a, L, r * N + j, k);
#pragma unroll
        for (int h = 0; h < HM; ++h)
            if (h < H) att_step<KPL>(a, q[h], k, mr[h] * N + j, m[h], l[h], acc[h]);
    }
#pragma unroll
    for (int h = 0; h < HM; ++h) {
        if (h < H) {
            const float inv = 1.f / l[h];
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                const int c = lane + 64 * i;
                if (c < dk) z[(r * H + h) * dk + c] = acc[h][i] * inv;
            }
            if (lane == 0) {
                stats[(r * H + h) * 2] = m[h];
                stats[(r * H + h) * 2 + 1] = l[h];
            }
        }
    }
}

// n_ngh >= ATT_WAVES: one row per workgroup, wave w takes neighbours j = w, w + 4, ... with its own
// online softmax; the partial states merge through LDS in wave order (as tgn_attn_fwd_split_kernel)
template <int KPL, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) tgat_attn_fwd_split_kernel(tm_tgat_attn a, float *__restrict__ z,
                                                                             float *__restrict__ stats) {
    __shared__ float s_acc[ATT_WAVES][HM][KPL][64], s_m[ATT_WAVES][HM], s_l[ATT_WAVES][HM];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r = blockIdx.x;
    const int H = a.n_head, N = a.n_ngh, dk = a.d_node + a.d_edge + a.d_time;
    const KeyLane<KPL> L = key_lane<KPL>(a, lane);
    float q[HM][KPL], acc[HM][KPL], m[HM], l[HM];
    int64_t mr[HM];
#pragma unroll
    for (int h = 0; h < HM; ++h) {
        m[h] = -__builtin_inff();
        l[h] = 0.f;
        mr[h] = h < H ? pair_row(a, r, h) : 0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int c = lane + 64 * i;
            q[h][i] = (h < H && c < dk) ? a.qf[(r * H + h) * dk + c] : 0.f;
            acc[h][i] = 0.f;
        }
    }
    for (int j = wv; j < N; j += ATT_WAVES) {
        float k[KPL];
        build_key<KPL>(a, L, r * N + j, k);
#pragma unroll
        for (int h = 0; h < HM; ++h)
            if (h < H) att_step<KPL>(a, q[h], k, mr[h] * N + j, m[h], l[h], acc[h]);
    }
#pragma unroll
    for (int h = 0; h < HM; ++h) {
#pragma unroll
        for (int i = 0; i < KPL; ++i) s_acc[wv][h][i][lane] = acc[h][i];
        if (lane == 0) {
            s_m[wv][h] = m[h];
            s_l[wv][h] = l[h];
        }
    }
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int h = 0; h < HM; ++h) {
        if (h >= H) continue;
        float M = s_m[0][h];
#pragma unroll
        for (int w = 1; w < ATT_WAVES; ++w) M = fmaxf(M, s_m[w][h]);
        float Ls = 0.f, sc[ATT_WAVES];
#pragma unroll
        for (int w = 0; w < ATT_WAVES; ++w) {
            sc[w] = s_l[w][h] > 0.f ? expf(s_m[w][h] - M) : 0.f;   // a wave with no neighbour adds nothing
            Ls += s_l[w][h] * sc[w];
        }
        const float inv = 1.f / Ls;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < ATT_WAVES; ++w) v = __builtin_fmaf(s_acc[w][h][i][lane], sc[w], v);
            const int c = lane + 64 * i;
            if (c < dk) z[(r * H + h) * dk + c] = v * inv;
        }
        if (lane == 0) {
            stats[(r * H + h) * 2] = M;
            stats[(r * H + h) * 2 + 1] = Ls;
        }
    }
}

// Backward of z[r,h] = sum_j p_j e_j k_j, p = softmax(s), s_j = qf_h.k_j / T (masked: constant):
//   c_j = gz_h.k_j;  d e_j += p_j c_j;  S_h = sum_j p_j e_j c_j;  ds_j = p_j (e_j c_j - S_h) (0 if masked)
//   d k_j  = sum_h p_j e_j gz_h + (ds_j / T) qf_h          (node-feature columns only are written)
//   d qf_h = (1/T) sum_j ds_j k_j                          (s_j = qf_h.k_j / T, so ds_j/dqf_h = k_j / T)
// Pass 1 builds every key (scores and c_j) and leaves the per-(j,h) scalars in LDS.  S_h is complete only
// after it, so pass 2 forms ds_j from those scalars: d k_j needs no key, d qf_h rebuilds key j once more
// (the row's keys are cache-resident from pass 1) and accumulates it with the head's ds_j.
template <int KPL, bool DNODE, bool DQF, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) tgat_attn_bwd_kernel(tm_tgat_attn a, const float *__restrict__ stats,
                                                                       const float *__restrict__ gz,
                                                                       float *__restrict__ d_parts,
                                                                       float *__restrict__ d_node,
                                                                       float *__restrict__ d_qf) {
    extern __shared__ float sh[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * ATT_WAVES + wave;
    if (r >= a.rows) return;
    const int H = a.n_head, N = a.n_ngh, dk = a.d_node + a.d_edge + a.d_time;
    float *pe_s = sh + (size_t)wave * 3 * N * HM;  // [N][HM] p*e
    float *ds_s = pe_s + N * HM;                   // [N][HM] p (0 if masked)
    float *ec_s = ds_s + N * HM;                   // [N][HM] e*c
    const KeyLane<KPL> L = key_lane<KPL>(a, lane);
    float q[HM][KPL], g[HM][KPL], m[HM], il[HM], S[HM];
    int64_t mr[HM];
#pragma unroll
    for (int h = 0; h < HM; ++h) {
        S[h] = 0.f;
        mr[h] = h < H ? pair_row(a, r, h) : 0;
        m[h] = h < H ? stats[(r * H + h) * 2] : 0.f;
        il[h] = h < H ? 1.f / stats[(r * H + h) * 2 + 1] : 0.f;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int c = lane + 64 * i;
            const bool ok = h < H && c < dk;
            q[h][i] = ok ? a.qf[(r * H + h) * dk + c] : 0.f;
            g[h][i] = ok ? gz[(r * H + h) * dk + c] : 0.f;
        }
    }
    for (int j = 0; j < N; ++j) {
        float k[KPL];
        build_key<KPL>(a, L, r * N + j, k);
#pragma unroll
        for (int h = 0; h < HM; ++h) {
            if (h < H) {
                float ps = 0.f, pc = 0.f;
#pragma unroll
                for (int i = 0; i < KPL; ++i) {
                    ps = __builtin_fmaf(q[h][i], k[i], ps);
                    pc = __builtin_fmaf(g[h][i], k[i], pc);
                }
                float s = wave_sum(ps) / a.temperature;
                const float c = wave_sum(pc);
                const int64_t ms = mr[h] * N + j;
                const bool masked = a.mask_node[ms] == 0;
                if (masked) s = -1e10f;
                const float e = a.ew ? a.ew[ms] : 1.f;
                const float p = expf(s - m[h]) * il[h];
                S[h] = __builtin_fmaf(p * e, c, S[h]);
                if (lane == 0) {
                    d_parts[(r * H + h) * N + j] = p * c;
                    if (DNODE || DQF) {
                        pe_s[j * HM + h] = p * e;
                        ds_s[j * HM + h] = masked ? 0.f : p;
                        ec_s[j * HM + h] = e * c;
                    }
                }
            }
        }
    }
    if (!DNODE && !DQF) return;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float invT = 1.f / a.temperature;
    float dq[HM][KPL];
#pragma unroll
    for (int h = 0; h < HM; ++h)
#pragma unroll
        for (int i = 0; i < KPL; ++i) dq[h][i] = 0.f;
    for (int j = 0; j < N; ++j) {
        float dkv[KPL], k[KPL];
#pragma unroll
        for (int i = 0; i < KPL; ++i) dkv[i] = 0.f;
        if (DQF) build_key<KPL>(a, L, r * N + j, k);
#pragma unroll
        for (int h = 0; h < HM; ++h) {
            if (h < H) {
                const float pe = pe_s[j * HM + h];
                const float ds = ds_s[j * HM + h] * (ec_s[j * HM + h] - S[h]) * invT;
                if (DNODE) {
#pragma unroll
                    for (int i = 0; i < KPL; ++i)
                        dkv[i] = __builtin_fmaf(pe, g[h][i], __builtin_fmaf(ds, q[h][i], dkv[i]));
                }
                if (DQF) {
#pragma unroll
                    for (int i = 0; i < KPL; ++i) dq[h][i] = __builtin_fmaf(ds, k[i], dq[h][i]);
                }
            }
        }
        if (DNODE) {
            float *dst = d_node + (r * N + j) * (int64_t)a.d_node;
#pragma unroll
            for (int i = 0; i < KPL; ++i)
                if (L.seg[i] == 0) dst[L.off[i]] = dkv[i];
        }
    }
    if (DQF) {
#pragma unroll
        for (int h = 0; h < HM; ++h) {
            if (h < H) {
#pragma unroll
                for (int i = 0; i < KPL; ++i) {
                    const int c = lane + 64 * i;
                    if (c < dk) d_qf[(r * H + h) * dk + c] = dq[h][i];
                }
            }
        }
    }
}

// ------------------------------------------------------------------ fused layer tail
// Per tile of MG_ROWS source rows (one workgroup, all d_key columns, so the LayerNorm reduction stays in LDS):
//   u   = z G^T + fc_b + query                      z [rows, K1 = n_head d_key], G = fc W_v folded on the host
//   h   = LayerNorm(u) (eps 1e-5, over d_key)
//   out = W21 relu(W11 h + b11) + b21 + W22 relu(W12 src + b12) + b22,   src = query[:, :feat]
// All four products run on v_mfma_f32_16x16x4_f32.  The weights come transposed ([K][N] row-major), so a B
// fragment is 16 consecutive floats of one weight row; the A operand is always an LDS tile whose K extent is
// zero-padded to a multiple of 16.  d_key and feat need not be multiples of the MFMA tile: B loads past
// the K or N extent are replaced by zeros (never read), stores past N are skipped.
constexpr int MG_ROWS = 16;      // rows per workgroup = one MFMA row tile
constexpr int MG_WAVES = 4;
constexpr int MG_KC = 128;       // K chunk of the z G^T product staged through LDS
constexpr int MG_MAXT = 9;       // most column tiles per wave: 16 * MG_WAVES * MG_MAXT = 576 columns; the kernel is
                                 // instantiated for 8 tiles (d_key <= 512, the code it always was) and for 9
constexpr int MG_PAD = 4;        // row stride padding of the LDS tiles (floats)

typedef float floatx4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int mg_up16(int x) { return (x + 15) & ~15; }

// acc[t] += A[16][k0..k0+kn) (LDS, row stride lda, kn a multiple of 16, zero-padded) * BT[kg0 + k][n] for the
// wave's column tiles nt = wave + MG_WAVES t.  Within a 16-deep step lane l feeds k = 4 (l >> 4) + s to the
// s-th MFMA on both operands (any order of k is the same sum of products per MFMA step).
template <int MAXT>
__device__ __forceinline__ void mg_gemm(const float *A, int lda, int kn, const float *__restrict__ BT, int kg0, int K,
                                        int N, floatx4 acc[MAXT]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int arow = lane & 15, ak = 4 * (lane >> 4);
    const int nt_n = (N + 15) >> 4;
    for (int k0 = 0; k0 < kn; k0 += 16) {
        const float4 av = *reinterpret_cast<const float4 *>(A + arow * lda + k0 + ak);
        const float a4[4] = {av.x, av.y, av.z, av.w};
        const int kg = kg0 + k0 + ak;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const int nt = wave + MG_WAVES * t;
            if (nt < nt_n) {
                const int n = nt * 16 + arow;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float b = (kg + s < K && n < N) ? BT[(int64_t)(kg + s) * N + n] : 0.f;
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[s], b, acc[t], 0, 0, 0);
                }
            }
        }
    }
}

template <int MAXT>
__device__ __forceinline__ void mg_zero(floatx4 acc[MAXT]) {
#pragma unroll
    for (int t = 0; t < MAXT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
}

// epilogue: f(row in tile, column, value) for every element this lane holds of its wave's column tiles
template <int MAXT, class F>
__device__ __forceinline__ void mg_epi(const floatx4 acc[MAXT], int N, F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt_n = (N + 15) >> 4;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int nt = wave + MG_WAVES * t;
        if (nt < nt_n) {
            const int n = nt * 16 + (lane & 15);
            if (n < N) {
#pragma unroll
                for (int r = 0; r < 4; ++r) f(4 * (lane >> 4) + r, n, acc[t][r]);
            }
        }
    }
}

template <int MAXT>
__global__ void __launch_bounds__(64 * MG_WAVES) tgat_merge_fwd_kernel(tm_tgat_merge a, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int dk = a.d_key, F = a.feat, K1 = a.n_head * a.d_key;
    const int dkp = mg_up16(dk), fp = mg_up16(F);
    const int ldu = dkp + MG_PAD;
    const int ldt = (fp > MG_KC ? fp : MG_KC) + MG_PAD;
    float *U = sm;                       // [16][ldu]  u, then h
    float *T1 = U + MG_ROWS * ldu;       // [16][ldt]  z chunk, then src, then relu(W11 h + b11)
    float *T2 = T1 + MG_ROWS * ldt;      // [16][ldt]  relu(W12 src + b12)
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * MG_ROWS;
    floatx4 acc[MAXT];

    // u = z G^T: z in K chunks through T1
    mg_zero<MAXT>(acc);
    for (int kc = 0; kc < K1; kc += MG_KC) {
        const int kn = K1 - kc < MG_KC ? mg_up16(K1 - kc) : MG_KC;
        __syncthreads();
        for (int i = tid; i < MG_ROWS * kn; i += 64 * MG_WAVES) {
            const int r = i / kn, c = i - r * kn;
            const bool ok = row0 + r < a.rows && kc + c < K1;
            T1[r * ldt + c] = ok ? a.z[(row0 + r) * K1 + kc + c] : 0.f;
        }
        __syncthreads();
        mg_gemm<MAXT>(T1, ldt, kn, a.gt, kc, K1, dk, acc);
    }
    mg_epi<MAXT>(acc, dk, [&](int r, int n, float v) {
        const float qv = row0 + r < a.rows ? a.query[(row0 + r) * dk + n] : 0.f;
        U[r * ldu + n] = v + a.fc_b[n] + qv;
    });
    __syncthreads();

    // LayerNorm over d_key: 16 threads per row (two passes: mean, then the centred second moment);
    // meanwhile src = query[:, :feat] goes to T1 (the z chunks are done)
    {
        const int r = tid >> 4, sub = tid & 15;
        float s = 0.f;
        for (int c = sub; c < dk; c += 16) s += U[r * ldu + c];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mean = s / (float)dk;
        float v = 0.f;
        for (int c = sub; c < dk; c += 16) {
            const float d = U[r * ldu + c] - mean;
            v = __builtin_fmaf(d, d, v);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        const float rstd = 1.f / sqrtf(v / (float)dk + 1e-5f);
        for (int c = sub; c < dkp; c += 16)
            U[r * ldu + c] = c < dk ? (U[r * ldu + c] - mean) * rstd * a.ln_w[c] + a.ln_b[c] : 0.f;
        for (int c = sub; c < fp; c += 16) {
            const bool ok = row0 + r < a.rows && c < F;
            T1[r * ldt + c] = ok ? a.query[(row0 + r) * dk + c] : 0.f;
        }
    }
    __syncthreads();

    // T2 = relu(src W12^T + b12)
    mg_zero<MAXT>(acc);
    mg_gemm<MAXT>(T1, ldt, fp, a.w12t, 0, F, F, acc);
    mg_epi<MAXT>(acc, F, [&](int r, int n, float v) { T2[r * ldt + n] = fmaxf(v + a.b12[n], 0.f); });
    __syncthreads();      // every wave is done reading src before T1 is rewritten
    // T1 = relu(h W11^T + b11)
    mg_zero<MAXT>(acc);
    mg_gemm<MAXT>(U, ldu, dkp, a.w11t, 0, dk, F, acc);
    mg_epi<MAXT>(acc, F, [&](int r, int n, float v) { T1[r * ldt + n] = fmaxf(v + a.b11[n], 0.f); });
    // zero the K padding of both tiles (columns F..fp-1 were never written by the epilogues)
    for (int i = tid; i < MG_ROWS * (fp - F); i += 64 * MG_WAVES) {
        const int r = i / (fp - F), c = F + i % (fp - F);
        T1[r * ldt + c] = 0.f;
        T2[r * ldt + c] = 0.f;
    }
    __syncthreads();

    // out = T1 W21^T + T2 W22^T + b21 + b22
    mg_zero<MAXT>(acc);
    mg_gemm<MAXT>(T1, ldt, fp, a.w21t, 0, F, F, acc);
    mg_gemm<MAXT>(T2, ldt, fp, a.w22t, 0, F, F, acc);
    mg_epi<MAXT>(acc, F, [&](int r, int n, float v) {
        if (row0 + r < a.rows) out[(row0 + r) * F + n] = v + a.b21[n] + a.b22[n];
    });
}

static size_t mg_lds_bytes(int dk, int F) {
    const int ldu = mg_up16(dk) + MG_PAD;
    const int fp = mg_up16(F);
    const int ldt = (fp > MG_KC ? fp : MG_KC) + MG_PAD;
    return sizeof(float) * (size_t)MG_ROWS * (ldu + 2 * ldt);
}

}  // namespace tgat
}  // namespace tmk

using namespace tmk;
using namespace tmk::tgat;

static int check_attn(const tm_tgat_attn *a, const char *who) {
    if (!a) return fail(TM_E_ARG, std::string(who) + ": NULL descriptor");
    if (a->rows < 0 || a->n_ngh <= 0 || a->n_head < 1 || a->d_node <= 0 || a->d_edge < 0 || a->d_time < 0 ||
        !(a->temperature > 0.f))
        return fail(TM_E_ARG, std::string(who) + ": bad sizes");
    if (a->n_head > ATT_MAXH) return fail(TM_E_UNSUPPORTED, std::string(who) + ": n_head > 4");
    const int dk = a->d_node + a->d_edge + a->d_time;
    if (dk > 64 * 9) return fail(TM_E_UNSUPPORTED, std::string(who) + ": d_key > 576");
    if (a->rows == 0) return TM_OK;
    if (!a->node_tab || (a->d_edge && !a->edge_tab) || !a->dt || (a->d_time && (!a->time_w || !a->time_b)) ||
        !a->mask_node || !a->qf)
        return fail(TM_E_ARG, std::string(who) + ": NULL pointer");
    if (a->seg_rows < 0 || (a->seg_rows > 0 && a->rows % a->seg_rows))
        return fail(TM_E_SHAPE, std::string(who) + ": rows must be a multiple of seg_rows");
    if ((a->node_idx && a->node_rows <= 0) || (a->edge_idx && a->edge_rows <= 0))
        return fail(TM_E_ARG, std::string(who) + ": empty feature table");
    return TM_OK;
}

template <int KPL>
static void launch_fwd(const tm_tgat_attn &a, float *z, float *stats, hipStream_t s) {
    // the heads' register arrays are sized for 2 heads where that covers them, else for 4 (as the TGN kernels)
    if (a.n_ngh >= ATT_WAVES) {
        if (a.n_head <= 2) tgat_attn_fwd_split_kernel<KPL, 2><<<dim3((unsigned)a.rows), 64 * ATT_WAVES, 0, s>>>(a, z, stats);
        else tgat_attn_fwd_split_kernel<KPL, ATT_MAXH><<<dim3((unsigned)a.rows), 64 * ATT_WAVES, 0, s>>>(a, z, stats);
        return;
    }
    const unsigned blocks = (unsigned)((a.rows + ATT_WAVES - 1) / ATT_WAVES);
    if (a.n_head <= 2) tgat_attn_fwd_kernel<KPL, 2><<<dim3(blocks), 64 * ATT_WAVES, 0, s>>>(a, z, stats);
    else tgat_attn_fwd_kernel<KPL, ATT_MAXH><<<dim3(blocks), 64 * ATT_WAVES, 0, s>>>(a, z, stats);
}

template <int KPL, int HM>
static void launch_bwd_h(const tm_tgat_attn &a, const float *stats, const float *gz, float *dp, float *dn, float *dq,
                         hipStream_t s) {
    const unsigned blocks = (unsigned)((a.rows + ATT_WAVES - 1) / ATT_WAVES);
    const size_t lds = (dn || dq) ? sizeof(float) * 3 * a.n_ngh * HM * ATT_WAVES : 0;
    const dim3 g(blocks), b(64 * ATT_WAVES);
    if (dn && dq) tgat_attn_bwd_kernel<KPL, true, true, HM><<<g, b, lds, s>>>(a, stats, gz, dp, dn, dq);
    else if (dn) tgat_attn_bwd_kernel<KPL, true, false, HM><<<g, b, lds, s>>>(a, stats, gz, dp, dn, dq);
    else if (dq) tgat_attn_bwd_kernel<KPL, false, true, HM><<<g, b, lds, s>>>(a, stats, gz, dp, dn, dq);
    else tgat_attn_bwd_kernel<KPL, false, false, HM><<<g, b, 0, s>>>(a, stats, gz, dp, dn, dq);
}

template <int KPL>
static void launch_bwd(const tm_tgat_attn &a, const float *stats, const float *gz, float *dp, float *dn, float *dq,
                       hipStream_t s) {
    if (a.n_head <= 2) launch_bwd_h<KPL, 2>(a, stats, gz, dp, dn, dq, s);
    else launch_bwd_h<KPL, ATT_MAXH>(a, stats, gz, dp, dn, dq, s);
}

#define TM_TGAT_KPL_DISPATCH(KPLV, CALL) \
    switch (KPLV) {                      \
        case 1: CALL(1); break;          \
        case 2: CALL(2); break;          \
        case 3: CALL(3); break;          \
        case 4: CALL(4); break;          \
        case 5: CALL(5); break;          \
        case 6: CALL(6); break;          \
        case 7: CALL(7); break;          \
        case 8: CALL(8); break;          \
        default: CALL(9); break;         \
    }

extern "C" int tm_tgat_attn_fwd(const tm_tgat_attn *a, float *z, float *stats, void *stream) {
    int rc = check_attn(a, "tm_tgat_attn_fwd");
    if (rc != TM_OK || a->rows == 0) return rc;
    if (!z || !stats) return fail(TM_E_ARG, "tm_tgat_attn_fwd: NULL output");
    hipStream_t s = (hipStream_t)stream;
    const int kpl = (a->d_node + a->d_edge + a->d_time + 63) / 64;
    hipEvent_t pe = prof_begin(s);
#define TM_FWD(K) launch_fwd<K>(*a, z, stats, s)
    TM_TGAT_KPL_DISPATCH(kpl, TM_FWD)
#undef TM_FWD
    TM_CHECK_LAUNCH();
    prof_end("tgat_attn_fwd_kernel", s, pe);
    return TM_OK;
}

extern "C" int tm_tgat_attn_bwd(const tm_tgat_attn *a, const float *stats, const float *gz, float *d_ew_parts,
                                float *d_node, float *d_qf, void *stream) {
    int rc = check_attn(a, "tm_tgat_attn_bwd");
    if (rc != TM_OK || a->rows == 0) return rc;
    if (!stats || !gz || !d_ew_parts) return fail(TM_E_ARG, "tm_tgat_attn_bwd: NULL pointer");
    if (d_node && a->node_idx) return fail(TM_E_ARG, "tm_tgat_attn_bwd: d_node needs a dense node table");
    if ((size_t)3 * a->n_ngh * ATT_MAXH * ATT_WAVES * sizeof(float) > 64 * 1024)
        return fail(TM_E_UNSUPPORTED, "tm_tgat_attn_bwd: n_ngh too large");
    hipStream_t s = (hipStream_t)stream;
    const int kpl = (a->d_node + a->d_edge + a->d_time + 63) / 64;
    hipEvent_t pe = prof_begin(s);
#define TM_BWD(K) launch_bwd<K>(*a, stats, gz, d_ew_parts, d_node, d_qf, s)
    TM_TGAT_KPL_DISPATCH(kpl, TM_BWD)
#undef TM_BWD
    TM_CHECK_LAUNCH();
    prof_end("tgat_attn_bwd_kernel", s, pe);
    return TM_OK;
}

extern "C" int tm_tgat_merge_fwd(const tm_tgat_merge *a, float *out, void *stream) {
    if (!a) return fail(TM_E_ARG, "tm_tgat_merge_fwd: NULL descriptor");
    if (a->rows < 0 || a->n_head < 1 || a->d_key <= 0 || a->feat <= 0 || a->feat > a->d_key)
        return fail(TM_E_ARG, "tm_tgat_merge_fwd: bad sizes");
    if (a->d_key > 16 * MG_WAVES * MG_MAXT) return fail(TM_E_UNSUPPORTED, "tm_tgat_merge_fwd: d_key > 576");
    const size_t lds = mg_lds_bytes(a->d_key, a->feat);
    if (lds > 64 * 1024)
        return fail(TM_E_UNSUPPORTED, "tm_tgat_merge_fwd: the row tile of d_key + 2 feat columns exceeds 64 KiB of LDS");
    if (a->rows == 0) return TM_OK;
    if (!a->z || !a->query || !a->gt || !a->fc_b || !a->ln_w || !a->ln_b || !a->w11t || !a->b11 || !a->w12t ||
        !a->b12 || !a->w21t || !a->b21 || !a->w22t || !a->b22 || !out)
        return fail(TM_E_ARG, "tm_tgat_merge_fwd: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)(((int64_t)a->rows + MG_ROWS - 1) / MG_ROWS);
    hipEvent_t pe = prof_begin(s);
    // 8 column tiles per wave cover d_key <= 512; only the wider keys pay for the ninth accumulator
    if (a->d_key <= 16 * MG_WAVES * 8) tgat_merge_fwd_kernel<8><<<dim3(blocks), 64 * MG_WAVES, lds, s>>>(*a, out);
    else tgat_merge_fwd_kernel<MG_MAXT><<<dim3(blocks), 64 * MG_WAVES, lds, s>>>(*a, out);
    TM_CHECK_LAUNCH();
    prof_end("tgat_merge_fwd_kernel", s, pe);
    return TM_OK;
}
