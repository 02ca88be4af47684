// Per-slot attention probabilities of the base TGN and the base TGAT on gfx950: the C entry points of
// attn_probs.h's kernels, in their TgnTime and TgatTime instances (the rounding of the time feature's argument, as
// tgn_attn.hip and tgat_attn.hip).  The reference's attention modules return these weights to their callers
// (TGN/modules/embedding_module.py ScaledDotProductAttention :16-32, TGAT/TGAT.py :64-80: the softmax's output,
// before the explanation weight); they are the attention baseline an explanation is compared against.
#include "attn_probs.h"

using namespace tmk;
using namespace tmk::attn;

extern "C" int tm_tgn_attn_probs(const tm_tgn_attn *a, float *probs, float *mean, void *stream) {
    return attn_probs<TgnTime>(a, probs, mean, stream, "tm_tgn_attn_probs", "tgn_attn_probs_kernel");
}

extern "C" int tm_tgat_attn_probs(const tm_tgat_attn *a, float *probs, float *mean, void *stream) {
    return attn_probs<TgatTime>(a, probs, mean, stream, "tm_tgat_attn_probs", "tgat_attn_probs_kernel");
}
