// The training pair of the temporal attention of the base TGN and the base TGAT on gfx950 (learn_base.py):
// attn_kernels.h's forward and backward with the attention dropout of ScaledDotProductAttention (after the
// softmax, before the explanation weight), the gradient of the folded queries and the gradient of the keys' time
// features (the two trainable vectors of TimeEncode).  One set of kernels, templated as the frozen pair;
// tgn_train.hip and tgat_train.hip hold the C entry points (and TGN's gathered-table reduction).
//
//   forward   z[r,h] = sum_j softmax(s)_j e'_j key_j,   e'_j = ew_j keep[(r H + h) N + j] keep_scale
//   backward  attn_bwd_kernel's formulas with e' for e (d ew_j = p_j c_j keep_j keep_scale), and
//             d w_c = sum_{r,j} -sin(u) dt[r,j] dk_j[c],   d b_c = sum_{r,j} -sin(u) dk_j[c]
//             u = TE::arg(dt, w_c, b_c), the argument build_key's cosine took (TGN: one rounding; TGAT: two,
//             and the roundings count as identity),
//             dk_j = sum_h a_jh gz_h + b_jh qf_h,   a_jh = p_j e'_j,   b_jh = ds_j / T.
//
// keep == NULL is no dropout: every product with e' then has the operands of the plain kernels, so z, stats,
// d_ew_parts, d_node and d_qf are those kernels' bits.  The keep bytes of a row are one contiguous run of
// n_head n_ngh bytes; a wave (or the row's workgroup) reads the run once with consecutive lanes and hands the
// factors on through LDS or a shuffle.
//
// The time gradient sums over every (row, neighbour) slot without atomics: a wave keeps its columns' sums in
// registers over all rows it walks (a fixed grid-stride set), the four waves of a workgroup add up in wave
// order through LDS, and the workgroup stores one partial [2][d_time] into the caller's workspace;
// attn_time_reduce_kernel then adds the partials of a column in fp64 in a fixed order.  The number of partials
// is a function of `rows` alone (train_parts), so the result is the same bits on every launch.
#pragma once
#include "attn_common.h"

namespace tmk {
namespace attn {

constexpr int TR_MAX_PARTS = 1024;   // workgroups of the backward = partials of the time gradient
constexpr int TR_RED_WAVES = 16;     // waves of the reducer: a thread walks at most 1024 / 16 = 64 partials

// workgroups of the backward for `rows` rows: every workgroup walks the same number of 4-row groups (up to one)
inline int64_t train_parts(int64_t rows) {
    const int64_t quads = (rows + ATT_WAVES - 1) / ATT_WAVES;
    if (quads <= TR_MAX_PARTS) return quads;
    const int64_t per = (quads + TR_MAX_PARTS - 1) / TR_MAX_PARTS;
    return (quads + per - 1) / per;
}

inline int64_t train_workspace_bytes(int64_t rows, int32_t d_time) {
    if (rows < 0 || d_time < 0) return -1;
    return (int64_t)sizeof(float) * train_parts(rows) * 2 * d_time;
}

// att_step (attn_kernels.h) with the keep factor kf (used only when has_keep)
template <int KPL>
__device__ __forceinline__ void att_step_train(const tm_attn &a, const float q[KPL], const float k[KPL], int64_t ms,
                                               bool has_keep, float kf, float &m, float &l, float acc[KPL]) {
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < KPL; ++i) p = __builtin_fmaf(q[i], k[i], p);
    float s = wave_sum(p) / a.temperature;
    if (a.mask_node[ms] == 0) s = -1e10f;
    float e = a.ew ? a.ew[ms] : 1.f;
    if (has_keep) e *= kf;
    const float mn = fmaxf(m, s);
    const float sc = expf(m - mn), w = expf(s - mn);
    l = l * sc + w;
    const float we = w * e;
#pragma unroll
    for (int i = 0; i < KPL; ++i) acc[i] = __builtin_fmaf(we, k[i], acc[i] * sc);
    m = mn;
}

// n_ngh < ATT_WAVES: one wave per row; the row's n_head n_ngh (<= 12) keep bytes sit one per lane
template <class TE, int KPL, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) attn_train_fwd_kernel(tm_attn a, const uint8_t *__restrict__ keep,
                                                                        float keep_scale, float *__restrict__ z,
                                                                        float *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * ATT_WAVES + (threadIdx.x >> 6);
    if (r >= a.rows) return;
    const int H = a.n_head, N = a.n_ngh, dk = a.d_node + a.d_edge + a.d_time;
    const KeyLane<KPL> L = key_lane<KPL>(a, lane);
    const bool has_keep = keep != nullptr;
    float kv = 0.f;
    if (has_keep && lane < H * N) kv = keep[r * H * N + lane] ? keep_scale : 0.f;
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
            if (h < H) {
                const float kf = __shfl(kv, h * N + j, 64);
                att_step_train<KPL>(a, q[h], k, mr[h] * N + j, has_keep, kf, m[h], l[h], acc[h]);
            }
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

// n_ngh >= ATT_WAVES: one row per workgroup as attn_fwd_split_kernel; the workgroup stages the row's
// keep factors in LDS (dynamic region: n_head n_ngh floats) with one coalesced read
template <class TE, int KPL, int HM>
__global__ void __launch_bounds__(64 * ATT_WAVES) attn_train_fwd_split_kernel(tm_attn a,
                                                                              const uint8_t *__restrict__ keep,
                                                                              float keep_scale, float *__restrict__ z,
                                                                              float *__restrict__ stats) {
    __shared__ float s_acc[ATT_WAVES][HM][KPL][64], s_m[ATT_WAVES][HM], s_l[ATT_WAVES][HM];
    extern __shared__ float s_keep[];      // [n_head][n_ngh], only with keep
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r = blockIdx.x;
    const int H = a.n_head, N = a.n_ngh, dk = a.d_node + a.d_edge + a.d_time;
    const KeyLane<KPL> L = key_lane<KPL>(a, lane);
    const bool has_keep = keep != nullptr;
    if (has_keep) {
        for (int i = threadIdx.x; i < H * N; i += 64 * ATT_WAVES) s_keep[i] = keep[r * H * N + i] ? keep_scale : 0.f;
        __syncthreads();
    }
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
            if (h < H) {
                const float kf = has_keep ? s_keep[h * N + j] : 1.f;
                att_step_train<KPL>(a, q[h], k, mr[h] * N + j, has_keep, kf, m[h], l[h], acc[h]);
            }
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

// attn_bwd_kernel (both passes; d_qf always, d k_j always formed) over a grid-stride set of rows per wave.
// AB: the instance can store the per-(slot, head) scalars (a_jh, b_jh) into slot_ab (nullable), from which TGN's
// tgn_tab_reduce_kernel forms the gradient of a gathered node table; TGAT's instances are built without it.
// Dynamic LDS: per wave 3 [N][HM] float arrays as there; ec_s first holds the row's keep factors (read by the
// whole wave in pass 1 just before lane 0 overwrites the slot with e' c: one wave, LDS accesses in program
// order).  After the row loop the same region takes the workgroup's [2][KPL][64] time-gradient sums.
template <class TE, int KPL, int HM, bool AB>
__global__ void __launch_bounds__(64 * ATT_WAVES) attn_train_bwd_kernel(
    tm_attn a, const uint8_t *__restrict__ keep, float keep_scale, const float *__restrict__ stats,
    const float *__restrict__ gz, float *__restrict__ d_parts, float *__restrict__ d_node, float *__restrict__ d_qf,
    float *__restrict__ slot_ab, float *__restrict__ parts) {
    extern __shared__ float sh[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.n_head, N = a.n_ngh, dk = a.d_node + a.d_edge + a.d_time;
    float *pe_s = sh + (size_t)wave * 3 * N * HM;  // [N][HM] p*e'
    float *ds_s = pe_s + N * HM;                   // [N][HM] p (0 if masked)
    float *ec_s = ds_s + N * HM;                   // [N][HM] keep factor, then e'*c
    const KeyLane<KPL> L = key_lane<KPL>(a, lane);
    const bool has_keep = keep != nullptr;
    const float invT = 1.f / a.temperature;
    float tf[KPL], tp[KPL];                        // this lane's d freq / d phase sums (time columns)
#pragma unroll
    for (int i = 0; i < KPL; ++i) tf[i] = tp[i] = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * ATT_WAVES + wave; r < a.rows; r += (int64_t)gridDim.x * ATT_WAVES) {
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
        if (has_keep) {
            for (int x = lane; x < H * N; x += 64) {
                const int h = x / N, j = x - h * N;
                ec_s[j * HM + h] = keep[r * H * N + x] ? keep_scale : 0.f;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
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
                    float e = a.ew ? a.ew[ms] : 1.f;
                    float kf = 1.f;
                    if (has_keep) {
                        kf = ec_s[j * HM + h];
                        e *= kf;
                    }
                    const float p = expf(s - m[h]) * il[h];
                    S[h] = __builtin_fmaf(p * e, c, S[h]);
                    if (lane == 0) {
                        if (d_parts) d_parts[(r * H + h) * N + j] = has_keep ? p * c * kf : p * c;
                        pe_s[j * HM + h] = p * e;
                        ds_s[j * HM + h] = masked ? 0.f : p;
                        ec_s[j * HM + h] = e * c;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        float dq[HM][KPL];
#pragma unroll
        for (int h = 0; h < HM; ++h)
#pragma unroll
            for (int i = 0; i < KPL; ++i) dq[h][i] = 0.f;
        for (int j = 0; j < N; ++j) {
            float dkv[KPL], k[KPL];
#pragma unroll
            for (int i = 0; i < KPL; ++i) dkv[i] = 0.f;
            build_key<TE, KPL>(a, L, r * N + j, k);
#pragma unroll
            for (int h = 0; h < HM; ++h) {
                if (h < H) {
                    const float pe = pe_s[j * HM + h];
                    const float ds = ds_s[j * HM + h] * (ec_s[j * HM + h] - S[h]) * invT;
                    if (AB && slot_ab && lane == 0) {
                        float *ab = slot_ab + ((r * N + j) * (int64_t)H + h) * 2;
                        ab[0] = pe;
                        ab[1] = ds;
                    }
#pragma unroll
                    for (int i = 0; i < KPL; ++i)
                        dkv[i] = __builtin_fmaf(pe, g[h][i], __builtin_fmaf(ds, q[h][i], dkv[i]));
#pragma unroll
                    for (int i = 0; i < KPL; ++i) dq[h][i] = __builtin_fmaf(ds, k[i], dq[h][i]);
                }
            }
            if (d_node) {
                float *dst = d_node + (r * N + j) * (int64_t)a.d_node;
#pragma unroll
                for (int i = 0; i < KPL; ++i)
                    if (L.seg[i] == 0) dst[L.off[i]] = dkv[i];
            }
            const float t = a.dt[r * N + j];
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                if (L.seg[i] == 2) {
                    const float gs = -sin_rd(TE::arg(t, L.tw[i], L.tb[i])) * dkv[i];
                    tp[i] += gs;
                    tf[i] = __builtin_fmaf(gs, t, tf[i]);
                }
            }
        }
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
        // the next row's keep factors and pass-1 scalars overwrite what pass 2 just read
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    // the workgroup's partial: waves add in wave order into sh[2][KPL][64]
    if (a.d_time == 0) return;
    for (int w = 0; w < ATT_WAVES; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                float *pf = sh + i * 64 + lane, *pp = sh + (KPL + i) * 64 + lane;
                *pf = w == 0 ? tf[i] : *pf + tf[i];
                *pp = w == 0 ? tp[i] : *pp + tp[i];
            }
        }
    }
    if (wave == ATT_WAVES - 1) {
        float *dst = parts + (int64_t)blockIdx.x * 2 * a.d_time;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            if (L.seg[i] == 2) {
                dst[L.off[i]] = sh[i * 64 + lane];
                dst[a.d_time + L.off[i]] = sh[(KPL + i) * 64 + lane];
            }
        }
    }
}

// d_time[x] = sum over the n_parts partials of column x (x < 2 d_time), fp64, fixed order: wave w of the
// workgroup adds partials w, w + 16, ... in turn, the sixteen sums then add in wave order.  No flavour; static,
// as both training translation units include it.
static __global__ void __launch_bounds__(64 * TR_RED_WAVES) attn_time_reduce_kernel(const float *__restrict__ parts,
                                                                                    int n_parts, int cols,
                                                                                    float *__restrict__ d_time) {
    __shared__ double s_sum[TR_RED_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (x < cols)
        for (int p = wv; p < n_parts; p += TR_RED_WAVES) s += (double)parts[(int64_t)p * cols + x];
    s_sum[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && x < cols) {
        double t = s_sum[0][lane];
#pragma unroll
        for (int w = 1; w < TR_RED_WAVES; ++w) t += s_sum[w][lane];
        d_time[x] = (float)t;
    }
}

// ------------------------------------------------------------------ launchers
template <class TE, int KPL, int HM>
void launch_train_fwd_h(const tm_attn &a, const uint8_t *keep, float ks, float *z, float *stats, hipStream_t s) {
    if (a.n_ngh >= ATT_WAVES) {
        const size_t lds = keep ? sizeof(float) * a.n_head * a.n_ngh : 0;
        attn_train_fwd_split_kernel<TE, KPL, HM><<<dim3((unsigned)a.rows), 64 * ATT_WAVES, lds, s>>>(a, keep, ks, z, stats);
        return;
    }
    const unsigned blocks = (unsigned)((a.rows + ATT_WAVES - 1) / ATT_WAVES);
    attn_train_fwd_kernel<TE, KPL, HM><<<dim3(blocks), 64 * ATT_WAVES, 0, s>>>(a, keep, ks, z, stats);
}

template <class TE, int KPL, int HM, bool AB>
void launch_train_bwd_h(const tm_attn &a, const uint8_t *keep, float ks, const float *stats, const float *gz,
                        float *dp, float *dn, float *dq, float *ab, float *parts, unsigned blocks, hipStream_t s) {
    size_t lds = sizeof(float) * 3 * a.n_ngh * HM * ATT_WAVES;
    const size_t red = sizeof(float) * 2 * KPL * 64;
    if (lds < red) lds = red;
    attn_train_bwd_kernel<TE, KPL, HM, AB><<<dim3(blocks), 64 * ATT_WAVES, lds, s>>>(a, keep, ks, stats, gz, dp, dn, dq, ab, parts);
}

// ------------------------------------------------------------------ the bodies of the C entry points
// who: the entry point's name (error messages); max_kpl: the flavour's widest key in registers per lane (the TGN
// training entry points stop at 8); label / red_label: the kernels' names in the per-kernel timing
template <class TE>
int attn_train_fwd(const tm_attn *a, const uint8_t *keep, float keep_scale, float *z, float *stats, void *stream,
                   const char *who, int max_kpl, const char *label) {
    int rc = check_attn(a, who, max_kpl, true);
    if (rc != TM_OK || a->rows == 0) return rc;
    if (!z || !stats) return fail(TM_E_ARG, std::string(who) + ": NULL output");
    if (keep && !(keep_scale > 0.f)) return fail(TM_E_ARG, std::string(who) + ": keep_scale must be positive");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pe = prof_begin(s);
#define TM_FWD(K)                                                                             \
    do {                                                                                      \
        if (a->n_head <= 2) launch_train_fwd_h<TE, K, 2>(*a, keep, keep_scale, z, stats, s);   \
        else launch_train_fwd_h<TE, K, ATT_MAXH>(*a, keep, keep_scale, z, stats, s);           \
    } while (0)
    TM_KPL_DISPATCH(key_regs(a), TM_FWD)
#undef TM_FWD
    TM_CHECK_LAUNCH();
    prof_end(label, s, pe);
    return TM_OK;
}

// AB: the flavour's backward takes slot_ab (TGN); else slot_ab must be NULL
template <class TE, bool AB>
int attn_train_bwd(const tm_attn *a, const uint8_t *keep, float keep_scale, const float *stats, const float *gz,
                   float *d_ew_parts, float *d_node, float *d_qf, float *d_time, float *slot_ab, void *workspace,
                   void *stream, const char *who, int max_kpl, const char *label, const char *red_label) {
    int rc = check_attn(a, who, max_kpl, true);
    if (rc != TM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (a->rows == 0) {
        if (d_time && a->d_time) TM_HIP(hipMemsetAsync(d_time, 0, sizeof(float) * 2 * a->d_time, s));
        return TM_OK;
    }
    const std::string w(who);
    if (!stats || !gz || !d_qf) return fail(TM_E_ARG, w + ": NULL pointer");
    if (a->d_time && (!d_time || !workspace)) return fail(TM_E_ARG, w + ": d_time and the workspace are required");
    if (keep && !(keep_scale > 0.f)) return fail(TM_E_ARG, w + ": keep_scale must be positive");
    if (d_node && a->node_idx) return fail(TM_E_ARG, w + ": d_node needs a dense node table");
    const unsigned blocks = (unsigned)train_parts(a->rows);
    float *parts = (float *)workspace;
    hipEvent_t pe = prof_begin(s);
#define TM_BWD(K)                                                                                              \
    do {                                                                                                       \
        if (a->n_head <= 2)                                                                                    \
            launch_train_bwd_h<TE, K, 2, AB>(*a, keep, keep_scale, stats, gz, d_ew_parts, d_node, d_qf, slot_ab, \
                                             parts, blocks, s);                                                \
        else                                                                                                   \
            launch_train_bwd_h<TE, K, ATT_MAXH, AB>(*a, keep, keep_scale, stats, gz, d_ew_parts, d_node, d_qf,  \
                                                    slot_ab, parts, blocks, s);                                \
    } while (0)
    TM_KPL_DISPATCH(key_regs(a), TM_BWD)
#undef TM_BWD
    TM_CHECK_LAUNCH();
    prof_end(label, s, pe);
    if (a->d_time) {
        const int cols = 2 * a->d_time;
        pe = prof_begin(s);
        attn_time_reduce_kernel<<<dim3((unsigned)((cols + 63) / 64)), 64 * TR_RED_WAVES, 0, s>>>(parts, (int)blocks,
                                                                                                  cols, d_time);
        TM_CHECK_LAUNCH();
        prof_end(red_label, s, pe);
    }
    return TM_OK;
}

}  // namespace attn
}  // namespace tmk
