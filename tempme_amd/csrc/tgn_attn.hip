// Base-TGN temporal attention with explanation weights on gfx950 (the consumer of the explanation
// path: temp_exp_main.py:614-616 feeds retrieve_explanation's output into TGN.contrast): the C entry points of
// the frozen pair.  The kernels are attn_kernels.h's, shared with TGAT, in their TgnTime instances: TGN's
// TimeEncode is cos(Linear(1, d)), so the time feature's argument is one fma.
//
// Reference (dharunm236/TempME, TGN/modules/embedding_module.py):
//   embedding_update_layer :356-393  per layer: source rows, their n_ngh neighbours, mask = node==0,
//                                    explanation weight row = layer's slice of explain_weights
//   TemporalAttentionLayer :181-216  query = [src feature | cos(b)], key = value = [ngh feature |
//                                    edge feature | cos(dt*w+b)], mask .repeat(n_head,1,1) (:211-212)
//   MultiHeadAttention     :52-86    q/k/v projections (no bias), explain_weight .repeat (:74-75)
//   ScaledDotProductAttention :16-32 bmm / temperature, masked_fill(-1e10), softmax, * explain weight,
//                                    bmm with v
#include "attn_kernels.h"

using namespace tmk;
using namespace tmk::attn;

// this pair reports n_head > 4 with the other bad sizes (TM_E_ARG), as it always has
static bool too_many_heads(const tm_attn *a) { return a && a->n_head > ATT_MAXH; }

extern "C" int tm_tgn_attn_fwd(const tm_tgn_attn *a, float *z, float *stats, void *stream) {
    if (too_many_heads(a)) return fail(TM_E_ARG, "tm_tgn_attn_fwd: bad sizes");
    return attn_fwd<TgnTime>(a, z, stats, stream, "tm_tgn_attn_fwd", "tgn_attn_fwd_kernel");
}

extern "C" int tm_tgn_attn_bwd(const tm_tgn_attn *a, const float *stats, const float *gz, float *d_ew_parts,
                               float *d_node, void *stream) {
    if (too_many_heads(a)) return fail(TM_E_ARG, "tm_tgn_attn_bwd: bad sizes");
    return attn_bwd<TgnTime, false>(a, stats, gz, d_ew_parts, d_node, nullptr, stream, "tm_tgn_attn_bwd",
                                    "tgn_attn_bwd_kernel");
}
