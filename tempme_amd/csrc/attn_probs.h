// The attention probabilities of the base TGN and the base TGAT on gfx950: what attn_kernels.h's forward keeps to
// itself.  The forward runs an online softmax and stores z and the (max, normaliser) pair per (row, head); the
// backward writes p * c, never p.  The kernels here return p itself, the attention baseline (ATTN) an explainer
// is compared against:
//     s_j = (qf[r,h] . key[r,j]) / temperature,  s_j = -1e10 where mask_node[pair_row(a, r, h) * N + j] == 0
//     probs[r,h,j] = softmax_j(s),   mean[r,j] = (1/H) sum_h probs[r,h,j]   (summed in head order)
// Templated on <TE, KPL, HM> as the forward.  The key comes from build_key and the score from att_step's fma chain,
// butterfly sum and division, so a score has the forward's bits, and an out-of-range id sets the forward's error
// flag.
//
// a->ew is ignored: the forward multiplies by ew after the softmax and does not renormalise, so the probabilities
// do not depend on it (a non-NULL buffer of any content gives the same bits).
//
// A fully masked (row, head) has N equal scores and comes out uniform, 1/N, as the forward's arithmetic gives it;
// the Python layer zeroes padded slots.
//
// The scores of a row sit in LDS as [n_ngh][HM].  One wave then takes, per head, the max and the sum over j: lanes
// stride over j (n_ngh may exceed 64), then a 64-lane butterfly.  Both are fixed orders and nothing is added with
// atomics, so every launch gives the same bits.
#pragma once
#include "attn_common.h"

namespace tmk {
namespace attn {

// the split form keeps one [n_ngh][HM] float row in LDS; sized for ATT_MAXH heads like bwd_lds_fits
inline bool probs_lds_fits(const tm_attn *a) {
    return (size_t)a->n_ngh * ATT_MAXH * sizeof(float) <= 64 * 1024;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// this lane's queries of row r, as the forward loads them
template <int KPL, int HM>
__device__ __forceinline__ void probs_queries(const tm_attn &a, int64_t r, int lane, float q[HM][KPL],
                                              int64_t mr[HM]) {
    const int H = a.n_head, dk = a.d_node + a.d_edge + a.d_time;
#pragma unroll
    for (int h = 0; h < HM; ++h) {
        mr[h] = h < H ? pair_row(a, r, h) : 0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int c = lane + 64 * i;
            q[h][i] = (h < H && c < dk) ? a.qf[(r * H + h) * dk + c] : 0.f;
        }
    }
}

// the masked scores of neighbour j against every head -> sc[j][.] (att_step's score, bit for bit)
template <int KPL, int HM>
__device__ __forceinline__ void probs_scores(const tm_attn &a, const float q[HM][KPL], const float k[KPL],
                                             const int64_t mr[HM], int j, int lane, float *sc) {
#pragma unroll
    for (int h = 0; h < HM; ++h) {
        if (h < a.n_head) {
            float p = 0.f;
#pragma unroll
            for (int i = 0; i < KPL; ++i) p = __builtin_fmaf(q[h][i], k[i], p);
            float s = wave_sum(p) / a.temperature;
            if (a.mask_node[mr[h] * a.n_ngh + j] == 0) s = -1e10f;
            if (lane == 0) sc[j * HM + h] = s;
        }
    }
}

// one wave: softmax over j of the row's scores sc [n_ngh][HM] and the stores.  A lane reads back only the
// exponentials it wrote itself.
template <int HM>
__device__ __forceinline__ void probs_finish(const tm_attn &a, int64_t r, int lane, float *sc,
                                             float *__restrict__ probs, float *__restrict__ mean) {
    const int H = a.n_head, N = a.n_ngh;
    float inv[HM];
#pragma unroll
    for (int h = 0; h < HM; ++h) {
        inv[h] = 0.f;
        if (h < H) {
            float mx = -__builtin_inff();
            for (int j = lane; j < N; j += 64) mx = fmaxf(mx, sc[j * HM + h]);
            mx = wave_max(mx);
            float l = 0.f;
            for (int j = lane; j < N; j += 64) {
                const float e = expf(sc[j * HM + h] - mx);
                sc[j * HM + h] = e;
                l += e;
            }
            inv[h] = 1.f / wave_sum(l);
        }
    }
    for (int j = lane; j < N; j += 64) {
        float sum = 0.f;
#pragma unroll
        for (int h = 0; h < HM; ++h) {
            if (h < H) {
                const float p = sc[j * HM + h] * inv[h];
                if (probs) probs[(r * H + h) * N + j] = p;
                sum += p;
            }
        }
        if (mean) mean[r * N + j] = sum / (float)H;
    }
}

// n_ngh < ATT_WAVES: one wave per row walks all its neighbours
template <class TE, int KPL, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) attn_probs_kernel(tm_attn a, float *__restrict__ probs,
                                                                    float *__restrict__ mean) {
    __shared__ float s_sc[ATT_WAVES][(ATT_WAVES - 1) * HM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * ATT_WAVES + wave;
    if (r >= a.rows) return;
    const KeyLane<KPL> L = key_lane<KPL>(a, lane);
    float q[HM][KPL];
    int64_t mr[HM];
    probs_queries<KPL, HM>(a, r, lane, q, mr);
    for (int j = 0; j < a.n_ngh; ++j) {
        float k[KPL];
        build_key<TE, KPL>(a, L, r * a.n_ngh + j, k);
        probs_scores<KPL, HM>(a, q, k, mr, j, lane, s_sc[wave]);
    }
    // lane 0's scores, read by the wave's other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    probs_finish<HM>(a, r, lane, s_sc[wave], probs, mean);
}

// n_ngh >= ATT_WAVES: one row per workgroup, wave w scores neighbours j = w, w + 4, ... (the forward's split of a
// row's independent gathers), wave 0 takes the softmax
template <class TE, int KPL, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) attn_probs_split_kernel(tm_attn a, float *__restrict__ probs,
                                                                          float *__restrict__ mean) {
    extern __shared__ float sh_sc[];   // [n_ngh][HM]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r = blockIdx.x;
    const KeyLane<KPL> L = key_lane<KPL>(a, lane);
    float q[HM][KPL];
    int64_t mr[HM];
    probs_queries<KPL, HM>(a, r, lane, q, mr);
    for (int j = wv; j < a.n_ngh; j += ATT_WAVES) {
        float k[KPL];
        build_key<TE, KPL>(a, L, r * a.n_ngh + j, k);
        probs_scores<KPL, HM>(a, q, k, mr, j, lane, sh_sc);
    }
    __syncthreads();
    if (wv != 0) return;
    probs_finish<HM>(a, r, lane, sh_sc, probs, mean);
}

template <class TE, int KPL, int HM>
void launch_probs_h(const tm_attn &a, float *probs, float *mean, hipStream_t s) {
    if (a.n_ngh >= ATT_WAVES) {
        const size_t lds = sizeof(float) * a.n_ngh * HM;
        attn_probs_split_kernel<TE, KPL, HM><<<dim3((unsigned)a.rows), 64 * ATT_WAVES, lds, s>>>(a, probs, mean);
        return;
    }
    const unsigned blocks = (unsigned)((a.rows + ATT_WAVES - 1) / ATT_WAVES);
    attn_probs_kernel<TE, KPL, HM><<<dim3(blocks), 64 * ATT_WAVES, 0, s>>>(a, probs, mean);
}

// the body of the C entry points; who: the entry point's name (error messages); label: its kernel's name in the
// per-kernel timing
template <class TE>
int attn_probs(const tm_attn *a, float *probs, float *mean, void *stream, const char *who, const char *label) {
    int rc = check_attn(a, who, 9, false);
    if (rc != TM_OK) return rc;
    if (!probs_lds_fits(a)) return fail(TM_E_UNSUPPORTED, std::string(who) + ": n_ngh too large");
    if (a->rows == 0) return TM_OK;
    if (!probs && !mean) return fail(TM_E_ARG, std::string(who) + ": NULL output (probs and mean)");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pe = prof_begin(s);
#define TM_PROBS(K)                                                        \
    do {                                                                   \
        if (a->n_head <= 2) launch_probs_h<TE, K, 2>(*a, probs, mean, s);  \
        else launch_probs_h<TE, K, ATT_MAXH>(*a, probs, mean, s);          \
    } while (0)
    TM_KPL_DISPATCH(key_regs(a), TM_PROBS)
#undef TM_PROBS
    TM_CHECK_LAUNCH();
    prof_end(label, s, pe);
    return TM_OK;
}

}  // namespace attn
}  // namespace tmk
