"""Device metrics, the parts that need no device: the count-form restatement of AP and ROC-AUC
(tests/rank_metrics_ref.py, what tm_rank_metrics computes) against scikit-learn, gather_rows over tensor rows,
the learn_base flag and the C-ABI symbol.

Tolerance (n + 2) 2^-52: each side rounds at most n fp64 terms and partial sums, all in [0, 1]."""
import os
import re

import numpy as np
import pytest
import torch

import rank_metrics_ref as RR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 2, 3, 63, 64, 65, 200, 257, 1000)


@pytest.mark.parametrize("n", NS)
def test_count_form_equals_sklearn(n):
    rng = np.random.default_rng(100 + n)
    worst = 0.0
    for regime in ("continuous", "levels1", "levels4", "levels16"):
        for labels in RR.LABEL_REGIMES:
            s, y = RR.make_scores(rng, n, regime), RR.make_labels(rng, n, labels)
            got, want = RR.rank_metrics_ref(y, s), RR.sklearn_pair(y, s)
            assert RR.close(got, want, (n + 2) * RR.EPS), (n, regime, labels, got, want)
            d = np.abs(np.array(got) - np.array(want))
            worst = max(worst, float(np.nanmax(d)) if not np.isnan(d).all() else 0.0)
    print(f"n={n}: worst |restatement - sklearn| = {worst:.3g} ({worst / ((n + 2) * RR.EPS):.3f} of the bound)")


def test_edge_cases():
    s = np.array([0.25, 0.5, 0.5, 0.75], np.float32)
    ap, auc = RR.rank_metrics_ref(np.zeros(4), s)
    assert ap == 0.0 and np.isnan(auc)
    ap, auc = RR.rank_metrics_ref(np.ones(4), s)
    assert ap == 1.0 and np.isnan(auc)
    # (-0.0, 0.0) is a tie: the negative at -0.0 counts the positive at 0.0 half
    ap, auc = RR.rank_metrics_ref(np.array([0.0, 1.0]), np.array([-0.0, 0.0], np.float32))
    assert (ap, auc) == (0.5, 0.5)
    assert RR.sklearn_pair(np.array([0.0, 1.0]), np.array([-0.0, 0.0], np.float32)) == (0.5, 0.5)
    assert all(np.isnan(RR.rank_metrics_ref(np.array([0.0, 1.0]), np.array([np.nan, 0.3], np.float32))))


def test_gather_rows_takes_tensor_rows():
    from tempme_amd.evaluate import FIGURES, gather_rows, reduce_epoch
    rng = np.random.default_rng(0)
    rows = {k: rng.uniform(size=len(FIGURES) + 1) for k in (5, 0, 3)}
    rows[3][1] = np.nan
    want = gather_rows(rows)
    got = gather_rows({k: torch.from_numpy(r.copy()) for k, r in rows.items()})
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert reduce_epoch(got).keys() == reduce_epoch(want).keys()
    # float32 tensor rows are widened, as np.asarray(row, float64) widens them
    r32 = {k: torch.from_numpy(r.astype(np.float32)) for k, r in rows.items()}
    np.testing.assert_array_equal(gather_rows(r32), gather_rows({k: v.numpy().astype(np.float64) for k, v in r32.items()}))


def test_run_sharded_keeps_tensor_rows():
    from tempme_amd.evaluate import FIGURES, run_sharded
    F = len(FIGURES) + 1
    spans = [(k, 10 * k, 10 * k + 10) for k in range(4)]
    row = lambda k: np.arange(F, dtype=np.float64) * (k + 1) / 7.0      # noqa: E731
    a = run_sharded(spans, lambda k, s, e: row(k))
    b = run_sharded(spans, lambda k, s, e: torch.from_numpy(row(k)))
    assert a == b


def test_learn_base_parser_knows_device_metrics():
    from tempme_amd import learn_base
    assert learn_base.parser().parse_args([]).device_metrics is False
    assert learn_base.parser().parse_args(["--device_metrics"]).device_metrics is True


def test_symbol_in_header_and_exports():
    from tempme_amd import _lib
    src = open(os.path.join(REPO, "include", "tempme.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+tm_rank_metrics\s*\(", src)
    assert "tm_rank_metrics" in _lib.EXPORTS
    import tempme_amd
    assert hasattr(tempme_amd.lib(), "tm_rank_metrics")
    assert tempme_amd.rank_metrics is tempme_amd.metrics.rank_metrics


def test_rank_metrics_refuses_cpu_tensors():
    import tempme_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tempme_amd.rank_metrics(torch.zeros(4), torch.rand(4))
