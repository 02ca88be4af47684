// Device and host helpers shared by the temporal-attention kernels of the two attention-based base models, TGN
// and TGAT (attn_kernels.h: the frozen pair; attn_train.h: the training pair): the lane layout of a key, the
// on-the-fly key build, the head-major pairing of mask / weight rows, the 64-lane butterfly sum, the dispatch over
// the key registers per lane and the descriptor check.
//
// The two flavours differ in device code by one thing, the rounding of the time feature's argument, which is a
// template parameter TE of everything that builds a key: a policy type with one static function.
#pragma once
#include "common.h"

namespace tmk {
namespace attn {

constexpr int ATT_MAXH = 4;
constexpr int ATT_WAVES = 4;

// TGN: TimeEncode is Linear(1, d) then cos (embedding_module.py:108-112): torch's CPU addmm rounds t*w+b once,
// i.e. an fma
struct TgnTime {
    static __device__ __forceinline__ float arg(float t, float w, float b) { return __builtin_fmaf(t, w, b); }
};

// TGAT: cos(t * basis_freq + phase) (TGAT.py:230-241), a multiply and then an add: two roundings, never an fma
// (time_arg, common.h, keeps the contraction off)
struct TgatTime {
    static __device__ __forceinline__ float arg(float t, float w, float b) { return time_arg(t, w, b); }
};

__device__ __forceinline__ float wave_sum(float v) {
    // butterfly: every lane ends with the same value (a+b == b+a)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// per-lane constants of the key layout
template <int KPL>
struct KeyLane {
    int seg[KPL];     // 0 node feature, 1 edge feature, 2 time feature, 3 padding
    int off[KPL];     // column inside the segment
    float tw[KPL], tb[KPL];
};

template <int KPL>
__device__ __forceinline__ KeyLane<KPL> key_lane(const tm_attn &a, int lane) {
    KeyLane<KPL> L;
    const int dn = a.d_node, de = a.d_edge, dk = a.d_node + a.d_edge + a.d_time;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const int c = lane + 64 * i;
        L.seg[i] = c < dn ? 0 : c < dn + de ? 1 : c < dk ? 2 : 3;
        L.off[i] = L.seg[i] == 0 ? c : L.seg[i] == 1 ? c - dn : L.seg[i] == 2 ? c - dn - de : 0;
        L.tw[i] = L.seg[i] == 2 ? a.time_w[L.off[i]] : 0.f;
        L.tb[i] = L.seg[i] == 2 ? a.time_b[L.off[i]] : 0.f;
    }
    return L;
}

// key[slot] -> k[] (this lane's elements); out-of-range ids set the flag and read row 0
template <class TE, int KPL>
__device__ __forceinline__ void build_key(const tm_attn &a, const KeyLane<KPL> &L, int64_t slot, float k[KPL]) {
    const float *nrow, *erow;
    if (a.node_idx) {
        int32_t id = a.node_idx[slot];
        if ((uint32_t)id >= (uint32_t)a.node_rows) {
            if (a.err_flag) *a.err_flag = TM_E_ARG;
            id = 0;
        }
        nrow = a.node_tab + (int64_t)id * a.d_node;
    } else {
        nrow = a.node_tab + slot * a.d_node;
    }
    if (a.edge_idx) {
        int32_t id = a.edge_idx[slot];
        if ((uint32_t)id >= (uint32_t)a.edge_rows) {
            if (a.err_flag) *a.err_flag = TM_E_ARG;
            id = 0;
        }
        erow = a.edge_tab + (int64_t)id * a.d_edge;
    } else {
        erow = a.edge_tab + slot * a.d_edge;
    }
    const float t = a.dt[slot];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        float v = 0.f;
        if (L.seg[i] == 0) v = nrow[L.off[i]];
        else if (L.seg[i] == 1) v = erow[L.off[i]];
        else if (L.seg[i] == 2) v = cos_rd(TE::arg(t, L.tw[i], L.tb[i]));
        k[i] = v;
    }
}

__device__ __forceinline__ int64_t pair_row(const tm_attn &a, int64_t r, int h) {
    if (!a.head_major_rows) return r;
    const int64_t seg = a.seg_rows > 0 ? a.seg_rows : a.rows;
    const int64_t base = r - r % seg;
    return base + ((r - base) * a.n_head + h) % seg;
}

// the backward kernels keep three [n_ngh][HM] float rows per wave in LDS
inline bool bwd_lds_fits(const tm_attn *a) {
    return (size_t)3 * a->n_ngh * ATT_MAXH * ATT_WAVES * sizeof(float) <= 64 * 1024;
}

// The descriptor check of every entry point.  max_kpl: the key registers per lane the entry point's kernels are
// dispatched for (d_key <= 64 max_kpl); need_bwd_lds: refuse an n_ngh whose backward rows do not fit in LDS here
// (the training entry points; the frozen backward checks it after its own pointers).
inline int check_attn(const tm_attn *a, const char *who, int max_kpl, bool need_bwd_lds) {
    const std::string w(who);
    if (!a) return fail(TM_E_ARG, w + ": NULL descriptor");
    if (a->rows < 0 || a->n_ngh <= 0 || a->n_head < 1 || a->d_node <= 0 || a->d_edge < 0 || a->d_time < 0 ||
        !(a->temperature > 0.f))
        return fail(TM_E_ARG, w + ": bad sizes");
    if (a->n_head > ATT_MAXH) return fail(TM_E_UNSUPPORTED, w + ": n_head > 4");
    const int dk = a->d_node + a->d_edge + a->d_time;
    if (dk > 64 * max_kpl) return fail(TM_E_UNSUPPORTED, w + ": d_key > " + std::to_string(64 * max_kpl));
    if (need_bwd_lds && !bwd_lds_fits(a)) return fail(TM_E_UNSUPPORTED, w + ": n_ngh too large");
    if (a->rows == 0) return TM_OK;
    if (!a->node_tab || (a->d_edge && !a->edge_tab) || !a->dt || (a->d_time && (!a->time_w || !a->time_b)) ||
        !a->mask_node || !a->qf)
        return fail(TM_E_ARG, w + ": NULL pointer");
    if (a->seg_rows < 0 || (a->seg_rows > 0 && a->rows % a->seg_rows))
        return fail(TM_E_SHAPE, w + ": rows must be a multiple of seg_rows");
    if ((a->node_idx && a->node_rows <= 0) || (a->edge_idx && a->edge_rows <= 0))
        return fail(TM_E_ARG, w + ": empty feature table");
    return TM_OK;
}

inline int key_regs(const tm_attn *a) { return (a->d_node + a->d_edge + a->d_time + 63) / 64; }

}  // namespace attn
}  // namespace tmk

// CALL(K) with K = registers per lane (1..9, d_key up to 576) as a compile-time constant; a caller whose kernels
// stop short of nine checks its bound first
#define TM_KPL_DISPATCH(KPLV, CALL) \
    switch (KPLV) {                 \
        case 1: CALL(1); break;     \
        case 2: CALL(2); break;     \
        case 3: CALL(3); break;     \
        case 4: CALL(4); break;     \
        case 5: CALL(5); break;     \
        case 6: CALL(6); break;     \
        case 7: CALL(7); break;     \
        case 8: CALL(8); break;     \
        default: CALL(9); break;    \
    }
