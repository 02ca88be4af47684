"""Average precision and ROC-AUC in the count form tm_rank_metrics computes (csrc/metrics.hip), in numpy:
fp32 compares, integer counts, fp64 sums; and the scikit-learn pair and the inputs the tests share.

A label is positive iff it is > 0.5; P positives, Nn = n - P; for element i

    ge_i = #{j: s_j >= s_i}     pge_i = #{j positive: s_j >= s_i}     pgt_i = #{j positive: s_j > s_i}

    AP  = (1 / P) sum_{i positive} pge_i / ge_i             P = 0           -> 0.0
    AUC = sum_{i negative} (pgt_i + pge_i) / (2 P Nn)       P = 0 or Nn = 0 -> NaN

A NaN score makes both figures NaN.
"""
import warnings

import numpy as np
import torch

EPS = 2.0 ** -52
SCORE_REGIMES = ("continuous", "levels1", "levels4", "levels16", "saturated")
LABEL_REGIMES = ("balanced", "one_positive", "one_negative", "all0", "all1")


def rank_metrics_ref(y_true, y_score):
    """(AP, AUC) of one score vector; the counts come from sorted fp32 arrays (searchsorted compares with <, so
    -0.0 and 0.0 tie, as in an fp32 compare)."""
    s = np.asarray(y_score, dtype=np.float32).reshape(-1)
    pos = np.asarray(y_true).reshape(-1).astype(np.float32) > 0.5
    n, P = len(s), int(pos.sum())
    if np.isnan(s).any():
        return float("nan"), float("nan")
    all_sorted, pos_sorted = np.sort(s), np.sort(s[pos])
    ge = n - np.searchsorted(all_sorted, s, side="left")
    pge = P - np.searchsorted(pos_sorted, s, side="left")
    pgt = P - np.searchsorted(pos_sorted, s, side="right")
    ap = float(np.sum(pge[pos].astype(np.float64) / ge[pos].astype(np.float64)) / P) if P else 0.0
    if P == 0 or P == n:
        return ap, float("nan")
    num = int(np.sum((pgt + pge)[~pos].astype(np.int64)))
    return ap, num / (2.0 * P * (n - P))


def sklearn_pair(y_true, y_score):
    """(average_precision_score, roc_auc_score) with scikit-learn's one-class warnings silenced."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(average_precision_score(y_true, y_score)), float(roc_auc_score(y_true, y_score))


def make_scores(rng, n, regime):
    """fp32 scores: sigmoids (torch's) of N(0, 8^2) draws, continuous or floored to 1, 4 or 16 levels, or the
    saturated sigmoid of n logits spaced evenly over [10, 30] (most of them exactly 1.0)."""
    if regime == "saturated":
        x = np.linspace(10.0, 30.0, n)
        rng.shuffle(x)
    else:
        x = rng.normal(0.0, 8.0, n)
    s = torch.sigmoid(torch.from_numpy(x.astype(np.float32))).numpy()
    if regime.startswith("levels"):
        L = np.float32(int(regime[6:]))
        s = np.floor(s * L) / L
    return s.astype(np.float32)


def make_labels(rng, n, regime):
    """fp32 0 / 1 labels."""
    y = np.zeros(n, np.float32)
    if regime == "balanced":
        y[rng.permutation(n)[:n // 2]] = 1
    elif regime == "one_positive":
        y[rng.integers(n)] = 1
    elif regime == "one_negative":
        y[:] = 1
        y[rng.integers(n)] = 0
    elif regime == "all1":
        y[:] = 1
    return y


def close(got, want, tol):
    """got within tol of want, NaN exactly where want is NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.all(np.abs(got - want)[~np.isnan(want)] <= tol))
