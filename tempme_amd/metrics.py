"""Per-batch evaluation metrics on the device: average precision and ROC-AUC without scikit-learn.

``rank_metrics(y_true, y_score)`` is ``sklearn.metrics.average_precision_score`` and ``roc_auc_score`` of V
score vectors in one launch of ``tm_rank_metrics`` (csrc/metrics.hip), one workgroup per vector.  The figures
are exact rank statistics over the fp32 scores as given (ties count as ties, so pass torch's own ``sigmoid``
output: fp32 saturation creates ties and the ties decide the figure); a label is positive iff it is > 0.5.
Two differences from scikit-learn, both at inputs it does not score: a vector with a NaN score gives (NaN, NaN)
where scikit-learn raises, and a one-class label vector gives AUC NaN (scikit-learn 1.7 returns NaN with a
warning, older versions raise) and AP 0.0 without positives.  Nothing here waits for the device.
"""
import torch

from . import _lib as L

MAX_N = 8192


def rank_metrics(y_true, y_score, out=None):
    """float64 [V, 2] (AP, ROC-AUC per score vector) on the scores' device, launched on the current stream.

    y_score: [n] or [V, n] float32 (rows may be strided; a last dimension that is not contiguous is copied).
    y_true: [n] or [n, 1] (one label vector for all rows) or [V, n], any real dtype or bool.
    out: optional float64 [V, 2] contiguous device tensor to write into."""
    if not (torch.is_tensor(y_score) and torch.is_tensor(y_true)):
        raise TypeError("rank_metrics: y_true and y_score are torch tensors")
    dev = L.require_device(y_score.device)
    if y_true.device != y_score.device:
        raise RuntimeError(f"rank_metrics: y_true is on {y_true.device}, y_score on {y_score.device}; the hot path "
                           "has no CPU fallback")
    if y_score.dtype != torch.float32:
        raise TypeError(f"rank_metrics: y_score is {y_score.dtype}; the scores are compared as float32 values")
    if y_score.dim() == 1:
        y_score = y_score.unsqueeze(0)
    if y_score.dim() != 2:
        raise ValueError(f"rank_metrics: y_score has shape {tuple(y_score.shape)}, expected [n] or [V, n]")
    V, n = y_score.shape
    if (n > 1 and y_score.stride(1) != 1) or (V > 1 and y_score.stride(0) < n):
        y_score = y_score.contiguous()
    s_stride = y_score.stride(0) if V > 1 else n
    if y_true.is_complex():
        raise TypeError("rank_metrics: y_true must be real or bool")
    if y_true.dim() == 2 and tuple(y_true.shape) == (n, 1):
        y_true = y_true.reshape(n)
    if y_true.dim() == 1 and y_true.shape[0] == n:
        l_stride = 0
    elif y_true.dim() == 2 and tuple(y_true.shape) == (V, n):
        l_stride = n
    else:
        raise ValueError(f"rank_metrics: y_true has shape {tuple(y_true.shape)} for scores {(V, n)}: expected "
                         f"[{n}], [{n}, 1] or [{V}, {n}]")
    y_true = y_true.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty((V, 2), dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.device == y_score.device and out.dtype == torch.float64
              and tuple(out.shape) == (V, 2) and out.is_contiguous()):
        raise ValueError(f"rank_metrics: out must be a contiguous float64 [{V}, 2] tensor on {y_score.device}")
    L.check(L.lib().tm_rank_metrics(L.ptr(y_score), s_stride, L.ptr(y_true), l_stride, V, n, L.ptr(out),
                                    L.stream_ptr(dev)), "rank_metrics")
    return out


__all__ = ["rank_metrics", "MAX_N"]
