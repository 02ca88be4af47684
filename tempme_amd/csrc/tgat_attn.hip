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
// The attention entry points run attn_kernels.h's kernels, shared with TGN, in their TgatTime instances (the time
// feature's two roundings): qf_h = W_k,h^T W_q,h query is supplied per source row, the kernel builds every key on
// the fly from the tables and produces z_h = sum_j softmax(s)_j ew_j key_j; (fc W_v) z follows in the tail.  The
// backward also returns the gradient of qf: TGAT's second layer queries with the first layer's output, which
// depends on the explanation weights.
#include "attn_kernels.h"

namespace tmk {
namespace tgat {

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
using namespace tmk::attn;
using namespace tmk::tgat;

extern "C" int tm_tgat_attn_fwd(const tm_tgat_attn *a, float *z, float *stats, void *stream) {
    return attn_fwd<TgatTime>(a, z, stats, stream, "tm_tgat_attn_fwd", "tgat_attn_fwd_kernel");
}

extern "C" int tm_tgat_attn_bwd(const tm_tgat_attn *a, const float *stats, const float *gz, float *d_ew_parts,
                                float *d_node, float *d_qf, void *stream) {
    return attn_bwd<TgatTime, true>(a, stats, gz, d_ew_parts, d_node, d_qf, stream, "tm_tgat_attn_bwd",
                                    "tgat_attn_bwd_kernel");
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
