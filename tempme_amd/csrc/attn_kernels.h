// The frozen temporal-attention pair of the base TGN and the base TGAT on gfx950: one set of kernels, templated
// on the flavour's time rounding TE (attn_common.h), the key registers per lane KPL and the heads the register
// arrays are sized for, HM.  tgn_attn.hip and tgat_attn.hip hold the C entry points.
//
// With W_q,h / W_k,h / W_v,h the head-h row blocks of w_qs / w_ks / w_vs, the score (W_q,h q).(W_k,h k_j) equals
// qf_h . k_j with qf_h = W_k,h^T W_q,h q, and sum_j a_j W_v,h k_j equals W_v,h (sum_j a_j k_j).  So the caller
// projects each SOURCE row once (qf, then fc*W_v on the result) and these kernels only touch raw keys: they build
// key[r,j] on the fly from the feature tables (never materialised), score it against every head, and accumulate
// the weighted raw keys with an online softmax.  The reference's per-neighbour 2*H*d_key^2 MACs (the bulk of its
// FLOPs) are gone; what is left is gather-bound (one key row per neighbour).
//
// Mapping: one 64-lane wave per source row, all heads; key element c = lane + 64*i lives in register i of that
// lane (KPL = ceil(d_key/64) registers), so every feature-table row is read with consecutive lanes on
// consecutive floats.
#pragma once
#include "attn_common.h"

namespace tmk {
namespace attn {

// one online-softmax step of head state (m, l, acc) with key k
template <int KPL>
__device__ __forceinline__ void att_step(const tm_attn &a, const float q[KPL], const float k[KPL], int64_t ms,
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
template <class TE, int KPL, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) attn_fwd_kernel(tm_attn a, float *__restrict__ z,
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
        build_key<TE, KPL>(a, L, r * N + j, k);
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

// n_ngh >= ATT_WAVES: one row per workgroup, wave w takes neighbours j = w, w + 4, ... with its own online
// softmax; the partial states (max, normaliser, weighted key sum) merge through LDS in wave order.  A row's
// neighbours are independent gathers, so four waves keep four of them in flight where one wave walked the chain
// alone; the 300-row root layer of a bs=100 TGN contrast had only 300 waves for 1,024 SIMDs.
template <class TE, int KPL, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) attn_fwd_split_kernel(tm_attn a, float *__restrict__ z,
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
        build_key<TE, KPL>(a, L, r * N + j, k);
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
// TGN's frozen model never asks for d qf (its queries do not depend on the explanation weights): it runs the
// DQF = false instances.  TGAT's second layer queries with the first layer's output, which does.
template <class TE, int KPL, bool DNODE, bool DQF, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) attn_bwd_kernel(tm_attn a, const float *__restrict__ stats,
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
        build_key<TE, KPL>(a, L, r * N + j, k);
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
        if (DQF) build_key<TE, KPL>(a, L, r * N + j, k);
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

// ------------------------------------------------------------------ launchers
// The heads' register arrays are sized for 2 heads where that covers them (TGN's default n_heads), else for 4:
// the split forward went 143 -> 96 VGPRs, 3 -> 5 waves per SIMD, 0.075 -> 0.055 ms per launch
// (profiles/r05_tgn_attn_ab.txt).
template <class TE, int KPL, int HM>
void launch_fwd_h(const tm_attn &a, float *z, float *stats, hipStream_t s) {
    if (a.n_ngh >= ATT_WAVES) {   // one row per workgroup, its neighbours over the waves
        attn_fwd_split_kernel<TE, KPL, HM><<<dim3((unsigned)a.rows), 64 * ATT_WAVES, 0, s>>>(a, z, stats);
        return;
    }
    const unsigned blocks = (unsigned)((a.rows + ATT_WAVES - 1) / ATT_WAVES);
    attn_fwd_kernel<TE, KPL, HM><<<dim3(blocks), 64 * ATT_WAVES, 0, s>>>(a, z, stats);
}

// WITH_DQF false: the d_qf instances are not built (dq must be NULL)
template <class TE, bool WITH_DQF, int KPL, int HM>
void launch_bwd_h(const tm_attn &a, const float *stats, const float *gz, float *dp, float *dn, float *dq,
                  hipStream_t s) {
    const unsigned blocks = (unsigned)((a.rows + ATT_WAVES - 1) / ATT_WAVES);
    // the per-wave (p e, p, e c) rows are [n_ngh][HM]: LDS sized for the instance launched, so the 2-head form
    // does not reserve (and lose occupancy to) 4 heads' worth
    const size_t lds = (dn || dq) ? sizeof(float) * 3 * a.n_ngh * HM * ATT_WAVES : 0;
    const dim3 g(blocks), b(64 * ATT_WAVES);
    if constexpr (WITH_DQF) {
        if (dq) {
            if (dn) attn_bwd_kernel<TE, KPL, true, true, HM><<<g, b, lds, s>>>(a, stats, gz, dp, dn, dq);
            else attn_bwd_kernel<TE, KPL, false, true, HM><<<g, b, lds, s>>>(a, stats, gz, dp, dn, dq);
            return;
        }
    }
    if (dn) attn_bwd_kernel<TE, KPL, true, false, HM><<<g, b, lds, s>>>(a, stats, gz, dp, dn, dq);
    else attn_bwd_kernel<TE, KPL, false, false, HM><<<g, b, 0, s>>>(a, stats, gz, dp, dn, dq);
}

// ------------------------------------------------------------------ the bodies of the C entry points
// who: the entry point's name (error messages); label: its kernel's name in the per-kernel timing
template <class TE>
int attn_fwd(const tm_attn *a, float *z, float *stats, void *stream, const char *who, const char *label) {
    int rc = check_attn(a, who, 9, false);
    if (rc != TM_OK || a->rows == 0) return rc;
    if (!z || !stats) return fail(TM_E_ARG, std::string(who) + ": NULL output");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pe = prof_begin(s);
#define TM_FWD(K)                                                   \
    do {                                                            \
        if (a->n_head <= 2) launch_fwd_h<TE, K, 2>(*a, z, stats, s); \
        else launch_fwd_h<TE, K, ATT_MAXH>(*a, z, stats, s);         \
    } while (0)
    TM_KPL_DISPATCH(key_regs(a), TM_FWD)
#undef TM_FWD
    TM_CHECK_LAUNCH();
    prof_end(label, s, pe);
    return TM_OK;
}

template <class TE, bool WITH_DQF>
int attn_bwd(const tm_attn *a, const float *stats, const float *gz, float *d_ew_parts, float *d_node, float *d_qf,
             void *stream, const char *who, const char *label) {
    int rc = check_attn(a, who, 9, false);
    if (rc != TM_OK || a->rows == 0) return rc;
    if (!stats || !gz || !d_ew_parts) return fail(TM_E_ARG, std::string(who) + ": NULL pointer");
    if (d_node && a->node_idx) return fail(TM_E_ARG, std::string(who) + ": d_node needs a dense node table");
    if (!bwd_lds_fits(a)) return fail(TM_E_UNSUPPORTED, std::string(who) + ": n_ngh too large");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pe = prof_begin(s);
#define TM_BWD(K)                                                                                        \
    do {                                                                                                 \
        if (a->n_head <= 2) launch_bwd_h<TE, WITH_DQF, K, 2>(*a, stats, gz, d_ew_parts, d_node, d_qf, s); \
        else launch_bwd_h<TE, WITH_DQF, K, ATT_MAXH>(*a, stats, gz, d_ew_parts, d_node, d_qf, s);         \
    } while (0)
    TM_KPL_DISPATCH(key_regs(a), TM_BWD)
#undef TM_BWD
    TM_CHECK_LAUNCH();
    prof_end(label, s, pe);
    return TM_OK;
}

}  // namespace attn
}  // namespace tmk
