// Training pair of the base TGN's temporal attention on gfx950 (learn_base.py for --base_type tgn): the C entry
// points.  Forward and backward run attn_train.h's kernels, shared with TGAT, in their TgnTime instances
// (u = fma(dt, w_c, b_c)); the backward is built with the slot_ab output.  What only TGN needs lives here: the
// gradient of the rows of a GATHERED node table -- in TGN that table is memory + node features, and the memory
// rows of nodes with pending messages are outputs of the trainable message MLP and GRU cell.
//
// The gradient of a gathered table never forms the [rows n_ngh, d_node] tensor of per-slot gradients: the
// backward stores the scalars (a_jh, b_jh) of every (slot, head), and tgn_tab_reduce_kernel, one workgroup per
// table row, walks that row's slots in the caller's (sorted, fixed) order and accumulates
// sum_h a gz[r,h] + b qf[r,h] on the node columns in registers: wave w takes entries w, w + 4, ... of the row's
// list, the four sums add in wave order through LDS, and the row is stored once (zero for a row without slots).
// No atomics, the same bits on every launch.  The same kernel in its dense form sums rows of a gradient
// matrix per table row: the backward of tab[idx] for the query-side gathers.
//
// The training entry points of this layer (_fwd, _bwd, _dtab) stop at eight key registers (d_key <= 512).
#include "attn_train.h"

namespace tmk {
namespace tgn {

using attn::ATT_WAVES;
constexpr int TRAIN_MAX_KPL = 8;

// out[v] = sum over the entries i in [seg_off[v], seg_off[v+1]) of the caller's list `order` of
//   SLOTS:  sum_h ab[s,h,0] gz[r,h][c] + ab[s,h,1] qf[r,h][c],  s = order[i] a slot (r = s / n_ngh), c < d
//   dense:  grad[s][c],                                          s = order[i] a row of grad
// One workgroup per output row v; rows below row_begin are stored as zero without a look at their lists (the
// padding row of a node table gathers a large share of all slots and feeds nothing trainable).
struct TabReduce {
    const int64_t *order;
    const int64_t *seg_off;
    int64_t n_order, n_src;      // entries of order; slots (rows n_ngh) or rows of grad an entry may name
    int32_t d, row_begin;
    const float *ab, *gz, *qf;   // SLOTS
    int32_t n_ngh, n_head, d_key;
    const float *grad;           // dense
    int32_t *err_flag;
};

template <int KPN, bool SLOTS>
__global__ void __launch_bounds__(64 * ATT_WAVES) tgn_tab_reduce_kernel(TabReduce t, float *__restrict__ out) {
    __shared__ float s_acc[ATT_WAVES][KPN][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t v = blockIdx.x;
    float acc[KPN];
#pragma unroll
    for (int i = 0; i < KPN; ++i) acc[i] = 0.f;
    if (v >= t.row_begin) {
        int64_t b = t.seg_off[v], e = t.seg_off[v + 1];
        if (b < 0) b = 0;
        if (e > t.n_order) e = t.n_order;
        for (int64_t x = b + wv; x < e; x += ATT_WAVES) {
            const int64_t s = t.order[x];
            if ((uint64_t)s >= (uint64_t)t.n_src) {
                if (t.err_flag) *t.err_flag = TM_E_ARG;
                continue;
            }
            if (SLOTS) {
                const int64_t r = s / t.n_ngh;
                for (int h = 0; h < t.n_head; ++h) {
                    const float *ab = t.ab + (s * t.n_head + h) * 2;
                    const float a = ab[0], bq = ab[1];
                    if (a == 0.f && bq == 0.f) continue;   // a masked slot of a row with live neighbours
                    const float *gp = t.gz + (r * t.n_head + h) * (int64_t)t.d_key;
                    const float *qp = t.qf + (r * t.n_head + h) * (int64_t)t.d_key;
#pragma unroll
                    for (int i = 0; i < KPN; ++i) {
                        const int c = lane + 64 * i;
                        if (c < t.d) acc[i] = __builtin_fmaf(a, gp[c], __builtin_fmaf(bq, qp[c], acc[i]));
                    }
                }
            } else {
                const float *gp = t.grad + s * (int64_t)t.d;
#pragma unroll
                for (int i = 0; i < KPN; ++i) {
                    const int c = lane + 64 * i;
                    if (c < t.d) acc[i] += gp[c];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < KPN; ++i) s_acc[wv][i][lane] = acc[i];
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int i = 0; i < KPN; ++i) {
        float sum = s_acc[0][i][lane];
#pragma unroll
        for (int w = 1; w < ATT_WAVES; ++w) sum += s_acc[w][i][lane];
        const int c = lane + 64 * i;
        if (c < t.d) out[v * t.d + c] = sum;
    }
}

}  // namespace tgn
}  // namespace tmk

using namespace tmk;
using namespace tmk::attn;
using namespace tmk::tgn;

extern "C" int64_t tm_tgn_attn_train_workspace_bytes(int64_t rows, int32_t d_time) {
    return train_workspace_bytes(rows, d_time);
}

extern "C" int tm_tgn_attn_train_fwd(const tm_tgn_attn *a, const uint8_t *keep, float keep_scale, float *z,
                                      float *stats, void *stream) {
    return attn_train_fwd<TgnTime>(a, keep, keep_scale, z, stats, stream, "tm_tgn_attn_train_fwd", TRAIN_MAX_KPL,
                                   "tgn_attn_train_fwd_kernel");
}

extern "C" int tm_tgn_attn_train_bwd(const tm_tgn_attn *a, const uint8_t *keep, float keep_scale,
                                      const float *stats, const float *gz, float *d_ew_parts, float *d_node,
                                      float *d_qf, float *d_time, float *slot_ab, void *workspace, void *stream) {
    return attn_train_bwd<TgnTime, true>(a, keep, keep_scale, stats, gz, d_ew_parts, d_node, d_qf, d_time, slot_ab,
                                         workspace, stream, "tm_tgn_attn_train_bwd", TRAIN_MAX_KPL,
                                         "tgn_attn_train_bwd_kernel", "tgn_time_reduce_kernel");
}

// every caller has checked d <= 512: the dispatch's ninth instance is never launched
static int launch_tab_reduce(const TabReduce &t, bool slots, int64_t out_rows, float *out, hipStream_t s,
                             const char *name) {
    const int kpn = (t.d + 63) / 64;
    hipEvent_t pe = prof_begin(s);
    const dim3 grid((unsigned)out_rows);
#define TM_RED(K)                                                                       \
    do {                                                                                \
        if (slots) tgn_tab_reduce_kernel<K, true><<<grid, 64 * ATT_WAVES, 0, s>>>(t, out);  \
        else tgn_tab_reduce_kernel<K, false><<<grid, 64 * ATT_WAVES, 0, s>>>(t, out);       \
    } while (0)
    TM_KPL_DISPATCH(kpn, TM_RED)
#undef TM_RED
    TM_CHECK_LAUNCH();
    prof_end(name, s, pe);
    return TM_OK;
}

extern "C" int tm_tgn_attn_train_dtab(const tm_tgn_attn *a, const float *slot_ab, const float *gz,
                                      const int64_t *order, int64_t n_order, const int64_t *seg_off,
                                      int32_t row_begin, float *d_tab, void *stream) {
    int rc = check_attn(a, "tm_tgn_attn_train_dtab", TRAIN_MAX_KPL, true);
    if (rc != TM_OK) return rc;
    if (a->node_rows <= 0 || !d_tab) return fail(TM_E_ARG, "tm_tgn_attn_train_dtab: no table to write");
    if (n_order < 0 || row_begin < 0) return fail(TM_E_ARG, "tm_tgn_attn_train_dtab: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    if (a->rows == 0 || n_order == 0) {
        TM_HIP(hipMemsetAsync(d_tab, 0, sizeof(float) * (size_t)a->node_rows * a->d_node, s));
        return TM_OK;
    }
    if (!a->node_idx) return fail(TM_E_ARG, "tm_tgn_attn_train_dtab: needs a gathered node table (node_idx)");
    if (!slot_ab || !gz || !order || !seg_off) return fail(TM_E_ARG, "tm_tgn_attn_train_dtab: NULL pointer");
    TabReduce t{};
    t.order = order, t.seg_off = seg_off, t.n_order = n_order, t.n_src = (int64_t)a->rows * a->n_ngh;
    t.d = a->d_node, t.row_begin = row_begin;
    t.ab = slot_ab, t.gz = gz, t.qf = a->qf;
    t.n_ngh = a->n_ngh, t.n_head = a->n_head, t.d_key = a->d_node + a->d_edge + a->d_time;
    t.err_flag = a->err_flag;
    return launch_tab_reduce(t, true, a->node_rows, d_tab, s, "tgn_tab_reduce_kernel");
}

extern "C" int tm_tgn_rows_reduce(const float *grad, int64_t n_rows, int32_t d, const int64_t *order, int64_t n_order,
                                  const int64_t *seg_off, int32_t out_rows, int32_t row_begin, float *out,
                                  int32_t *err_flag, void *stream) {
    if (n_rows < 0 || d <= 0 || n_order < 0 || out_rows < 0 || row_begin < 0)
        return fail(TM_E_ARG, "tm_tgn_rows_reduce: bad sizes");
    if (d > 64 * 8) return fail(TM_E_UNSUPPORTED, "tm_tgn_rows_reduce: d > 512");
    if (out_rows == 0) return TM_OK;
    if (!out) return fail(TM_E_ARG, "tm_tgn_rows_reduce: NULL output");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0 || n_order == 0) {
        TM_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)out_rows * d, s));
        return TM_OK;
    }
    if (!grad || !order || !seg_off) return fail(TM_E_ARG, "tm_tgn_rows_reduce: NULL pointer");
    TabReduce t{};
    t.order = order, t.seg_off = seg_off, t.n_order = n_order, t.n_src = n_rows;
    t.d = d, t.row_begin = row_begin, t.grad = grad, t.err_flag = err_flag;
    return launch_tab_reduce(t, false, out_rows, out, s, "tgn_rows_reduce_kernel");
}
