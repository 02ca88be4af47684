// Device helpers shared by the TGN attention kernels (tgn_attn.hip: the frozen base model; tgn_train.hip: the
// training pair): the lane layout of a key, the on-the-fly key build with TGN's single-rounded time feature
// (TimeEncode is cos(Linear(1, d)): u = fma(dt, w, b)), the head-major pairing of mask / weight rows, the
// 64-lane butterfly sum and the dispatch over the key registers per lane.
#pragma once
#include "common.h"

namespace tmk {
namespace tgn {

constexpr int ATT_MAXH = 4;
constexpr int ATT_WAVES = 4;

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
__device__ __forceinline__ KeyLane<KPL> key_lane(const tm_tgn_attn &a, int lane) {
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

// key[slot] -> k[] (this lane's elements).  TimeEncode is Linear(1, d) then cos
// (embedding_module.py:108-112): torch's CPU addmm rounds t*w+b once, i.e. an fma.
template <int KPL>
__device__ __forceinline__ void build_key(const tm_tgn_attn &a, const KeyLane<KPL> &L, int64_t slot, float k[KPL]) {
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
        else if (L.seg[i] == 2) v = cos_rd(__builtin_fmaf(t, L.tw[i], L.tb[i]));
        k[i] = v;
    }
}

__device__ __forceinline__ int64_t pair_row(const tm_tgn_attn &a, int64_t r, int h) {
    if (!a.head_major_rows) return r;
    const int64_t seg = a.seg_rows > 0 ? a.seg_rows : a.rows;
    const int64_t base = r - r % seg;
    return base + ((r - base) * a.n_head + h) % seg;
}

}  // namespace tgn
}  // namespace tmk

// CALL(K) with K = registers per lane (1..8) as a compile-time constant
#define TM_KPL_DISPATCH(KPLV, CALL) \
    switch (KPLV) {                 \
        case 1: CALL(1); break;     \
        case 2: CALL(2); break;     \
        case 3: CALL(3); break;     \
        case 4: CALL(4); break;     \
        case 5: CALL(5); break;     \
        case 6: CALL(6); break;     \
        case 7: CALL(7); break;     \
        default: CALL(8); break;    \
    }

// the same with a ninth register (d_key up to 576): the frozen attention pair of tgn_attn.hip only; the training
// kernels of tgn_train.hip stop at 8
#define TM_KPL_DISPATCH9(KPLV, CALL)               \
    switch (KPLV) {                                \
        case 9: CALL(9); break;                    \
        default: TM_KPL_DISPATCH(KPLV, CALL) break; \
    }
