// Training pair of the base TGAT's temporal attention on gfx950 (learn_base.py for --base_type tgat): the C entry
// points.  Forward and backward run attn_train.h's kernels, shared with TGN, in their TgatTime instances: the
// attention dropout of ScaledDotProductAttention (TGAT.py:74-78, after the softmax, before the explanation weight)
// and the gradient of the keys' time features, which reaches the two trainable vectors of TimeEncode (basis_freq,
// phase) with u = fl(fl(dt w_c) + b_c) as build_key forms it.  Keys up to 576 wide (nine registers per lane).
#include "attn_train.h"

using namespace tmk;
using namespace tmk::attn;

extern "C" int64_t tm_tgat_attn_train_workspace_bytes(int64_t rows, int32_t d_time) {
    return train_workspace_bytes(rows, d_time);
}

extern "C" int tm_tgat_attn_train_fwd(const tm_tgat_attn *a, const uint8_t *keep, float keep_scale, float *z,
                                      float *stats, void *stream) {
    return attn_train_fwd<TgatTime>(a, keep, keep_scale, z, stats, stream, "tm_tgat_attn_train_fwd", 9,
                                    "tgat_attn_train_fwd_kernel");
}

extern "C" int tm_tgat_attn_train_bwd(const tm_tgat_attn *a, const uint8_t *keep, float keep_scale,
                                      const float *stats, const float *gz, float *d_ew_parts, float *d_node,
                                      float *d_qf, float *d_time, void *workspace, void *stream) {
    return attn_train_bwd<TgatTime, false>(a, keep, keep_scale, stats, gz, d_ew_parts, d_node, d_qf, d_time, nullptr,
                                           workspace, stream, "tm_tgat_attn_train_bwd", 9,
                                           "tgat_attn_train_bwd_kernel", "tgat_time_reduce_kernel");
}
