"""AP and ROC-AUC on the device: tm_rank_metrics (csrc/metrics.hip) through the C ABI, metrics.rank_metrics, and
the four call sites with ``device_metrics`` against their scikit-learn defaults.

Kernel: |figure - scikit-learn's| <= (n + 2) 2^-52 per vector, NaN exactly where scikit-learn gives NaN.  Each side
rounds at most n fp64 terms and partial sums, all in [0, 1]; the numpy restatement of the kernel's definitions
(tests/rank_metrics_ref.py) uses 0.023 of that bound (tests/test_rank_metrics_cpu.py prints it).

Call sites: a device row copied to the host equals the default row bit for bit in every figure that is a read of an
fp32 device scalar (acc, fid_prob, fid_logit, the losses, their ratio counterparts, the flag), and within
(2 test_bs + 2 + len(ratios)) 2^-52 in aps, auc, ratio_aps, ratio_auc (2 test_bs scores per vector, and the mean over
the ratios taken on the device).
"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rank_metrics_ref as RR
import tgn_inputs as TI

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 200, 255, 256, 257, 1024, 1025, 8192)
VS = (1, 3, 11)
GAP = 5
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ 1. the kernel through the C ABI
def launch(dev, score, s_stride, label, l_stride, V, n):
    """tm_rank_metrics into an [V, 2] window of a guarded buffer -> (rc, out [V, 2] on the host)."""
    from tempme_amd import _lib as L
    buf = torch.full((2 + 2 * V + 2,), SENTINEL, dtype=torch.float64, device=dev)
    rc = L.lib().tm_rank_metrics(L.ptr(score), s_stride, L.ptr(label), l_stride, V, n,
                                 C.c_void_p(buf.data_ptr() + 16), L.stream_ptr(dev))
    h = buf.cpu().numpy()
    assert (h[:2] == SENTINEL).all() and (h[-2:] == SENTINEL).all(), "a guard double around out was written"
    return rc, h[2:2 + 2 * V].reshape(V, 2)


def padded(rows, n):
    """[V, n + GAP] fp32 with NaN in the gaps: a read past a row turns its figures NaN."""
    a = np.full((len(rows), n + GAP), np.nan, np.float32)
    a[:, :n] = np.stack(rows)
    return a


@pytest.mark.parametrize("n", NS)
def test_kernel_equals_sklearn(dev, n):
    rng = np.random.default_rng(1000 + n)
    # per-row vector t (counted over the whole parametrisation) pairs score regime t % 5 with label regime
    # (2 t + t // 5) % 5: 15 distinct pairs per n that hold every regime of both kinds, all 25 pairs over the ns;
    # a shared label vector takes the regimes in turn and its rows' scores cycle
    t, case, worst = 15 * NS.index(n), NS.index(n), 0.0
    for V in VS:
        for per_row in (False, True):
            scores, labels = [], []
            shared = RR.make_labels(rng, n, RR.LABEL_REGIMES[case % 5])
            for r in range(V):
                if per_row:
                    scores.append(RR.make_scores(rng, n, RR.SCORE_REGIMES[t % 5]))
                    labels.append(RR.make_labels(rng, n, RR.LABEL_REGIMES[(2 * t + t // 5) % 5]))
                    t += 1
                else:
                    scores.append(RR.make_scores(rng, n, RR.SCORE_REGIMES[(case + r) % 5]))
                    labels.append(shared)
            case += 1
            s_d = torch.from_numpy(padded(scores, n)).to(dev)
            l_d = torch.from_numpy(padded(labels, n) if per_row else shared).to(dev)
            rc, got = launch(dev, s_d, n + GAP, l_d, n + GAP if per_row else 0, V, n)
            assert rc == 0
            rc, again = launch(dev, s_d, n + GAP, l_d, n + GAP if per_row else 0, V, n)
            assert rc == 0 and got.tobytes() == again.tobytes(), "two launches differ"
            for r in range(V):
                want = RR.sklearn_pair(labels[r], scores[r])
                assert RR.close(got[r], want, (n + 2) * RR.EPS), (n, V, per_row, r, got[r], want)
                d = np.abs(got[r] - np.array(want))
                worst = max(worst, float(np.nanmax(d)) if not np.isnan(d).all() else 0.0)
    print(f"n={n}: worst |kernel - sklearn| = {worst:.3g} ({worst / ((n + 2) * RR.EPS):.3f} of the bound)")


@pytest.mark.parametrize("n", (3, 200, 1025))
def test_nan_row_gives_nan_and_spares_its_neighbours(dev, n):
    rng = np.random.default_rng(n)
    scores = [RR.make_scores(rng, n, "continuous") for _ in range(3)]
    y = RR.make_labels(rng, n, "balanced")
    clean = [RR.sklearn_pair(y, s) for s in scores]
    scores[1][n // 2] = np.nan
    rc, got = launch(dev, torch.from_numpy(padded(scores, n)).to(dev), n + GAP, torch.from_numpy(y).to(dev), 0, 3, n)
    assert rc == 0 and np.isnan(got[1]).all()
    for r in (0, 2):
        assert RR.close(got[r], clean[r], (n + 2) * RR.EPS)


def test_signed_zeros_tie(dev):
    s = torch.tensor([-0.0, 0.0], device=dev)
    rc, got = launch(dev, s, 2, torch.tensor([0.0, 1.0], device=dev), 0, 1, 2)
    assert rc == 0 and tuple(got[0]) == (0.5, 0.5)


def test_limits_are_refused(dev):
    from tempme_amd import _lib as L
    s = torch.rand(2, 8200, device=dev)
    y = (torch.rand(8200, device=dev) > 0.5).float()
    rc, got = launch(dev, s, 8200, y, 0, 2, 8193)
    assert rc == L.TM_E_UNSUPPORTED and "8192" in L.lib().tm_last_error().decode()
    assert (got == SENTINEL).all()
    assert launch(dev, s, 99, y, 0, 2, 100)[0] == L.TM_E_ARG            # score_stride = n - 1
    assert launch(dev, s, 8200, y, 99, 2, 100)[0] == L.TM_E_ARG         # a label stride below n
    assert launch(dev, s, 8200, y, 0, 2, 0)[0] == L.TM_E_ARG            # n = 0
    assert launch(dev, s, 8200, y, 0, -1, 100)[0] == L.TM_E_ARG         # V < 0
    rc, got = launch(dev, s, 8200, y, 0, 0, 100)                        # V = 0: nothing written
    assert rc == 0 and got.size == 0


# ------------------------------------------------------------------ 2. metrics.rank_metrics
def test_rank_metrics_wrapper(dev):
    import tempme_amd as tm
    rng = np.random.default_rng(7)
    n, V = 200, 3
    scores = [RR.make_scores(rng, n, r) for r in ("continuous", "levels4", "saturated")]
    y = RR.make_labels(rng, n, "balanced")
    want = np.array([RR.sklearn_pair(y, s) for s in scores])
    s_d, y_d = torch.from_numpy(np.stack(scores)).to(dev), torch.from_numpy(y).to(dev)
    got = tm.rank_metrics(y_d, s_d)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (V, 2)
    assert RR.close(got.cpu().numpy(), want, (n + 2) * RR.EPS)
    bits = got.cpu().numpy().tobytes()
    for labels in (y_d.reshape(n, 1), y_d > 0.5, y_d.to(torch.int64), y_d.double(), y_d.expand(V, n)):
        assert tm.rank_metrics(labels, s_d).cpu().numpy().tobytes() == bits, labels.dtype
    # strided rows are read in place, a strided last dimension is copied
    wide = torch.full((V, n + GAP), float("nan"), device=dev)
    wide[:, :n] = s_d
    assert tm.rank_metrics(y_d, wide[:, :n]).cpu().numpy().tobytes() == bits
    assert tm.rank_metrics(y_d, s_d.t().contiguous().t()).cpu().numpy().tobytes() == bits
    one = tm.rank_metrics(y_d, s_d[1])
    assert tuple(one.shape) == (1, 2) and one.cpu().numpy().tobytes() == got[1:2].cpu().numpy().tobytes()
    out = torch.empty((V, 2), dtype=torch.float64, device=dev)
    assert tm.rank_metrics(y_d, s_d, out=out) is out and out.cpu().numpy().tobytes() == bits
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm.rank_metrics(y_d.cpu(), s_d.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm.rank_metrics(y_d.cpu(), s_d)
    with pytest.raises(NotImplementedError, match="8192"):
        tm.rank_metrics(torch.zeros(8193, device=dev), torch.rand(8193, device=dev))


# ------------------------------------------------------------------ 3. the call sites
RATIOS = [0.01, 0.05, 0.1, 0.2, 0.3]
TEST_BS = 40
EXACT = ("acc", "fid_prob", "fid_logit", "loss", "pred_loss", "kl_loss", "ratio_acc", "ratio_prob", "ratio_logit")
RANKED = ("aps", "auc", "ratio_aps", "ratio_auc")
SITE_TOL = (2 * TEST_BS + 2 + len(RATIOS)) * RR.EPS


def _args(**kw):
    a = dict(test_bs=TEST_BS, if_bern=False, beta=0.5, prior_p=0.3, test_threshold=True, base_type="tgn", n_degree=10,
             ratios=list(RATIOS))
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.fixture(scope="module")
def setup(dev):
    """tests/test_gpu_eval.py's set-up: 80 nodes, 3,000 edges, N = 10, a random TGN and explainer."""
    import tempme_amd as tm
    from tempme_amd.preprocess import sample_events
    from tempme_amd.tgn import TGN
    from tempme_amd.workload import enron_like, split
    g = enron_like(n_nodes=80, n_edges=3000, seed=4, node_feat="uniform")
    (src, dst, ts, eidx), rows, pool = split(g)
    f = tm.NeighborFinder.from_edges(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"],
                                     device=dev, seed=2)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    ev = (to(src, np.int32), to(dst, np.int32), to(ts, np.float64), to(eidx, np.int32))
    buf = sample_events(f.graph, 2, tm.SPLIT_TEST, 10, 3, *ev, torch.arange(len(src), dtype=torch.int32, device=dev),
                        to(pool, np.int32))
    torch.manual_seed(3)
    base = TGN(g["n_feat"], g["e_feat"], n_neighbors=10, device=dev, n_layers=2, n_heads=2, dropout=0.1)
    base.forbidden_memory_update = True
    base = base.to(dev).eval()
    torch.manual_seed(5)
    ex = tm.TempME(base, "tgn", "enron", out_dim=40, hid_dim=64, device=dev,
                   null_model={k: 1.0 / 12 for k in range(1, 13)}).to(dev).eval()
    return buf, ev, base, ex


def check_figures(got, want, what, tol=SITE_TOL):
    """got / want: {figure: value}; the two rules of the module docstring (tol: the bound for the vector length)."""
    for k in EXACT:
        if k in want:
            a, b = np.float64(got[k]), np.float64(want[k])
            assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (what, k, a, b)
    for k in RANKED:
        if k in want:
            print(f"{what} {k}: device {float(got[k])!r} host {float(want[k])!r}")
            assert RR.close(got[k], want[k], tol), (what, k, got[k], want[k])


def test_eval_batch_device_row(dev, setup):
    from tempme_amd.evaluate import FIGURES, THRESHOLD_RAN, eval_batch, eval_spans
    from tempme_amd.train import batch_from_pack
    buf, ev, base, ex = setup
    args = _args()
    for k, s, e in eval_spans(int(ev[0].shape[0]) - 1, args.test_bs)[:3]:
        rows = torch.arange(s, e, dtype=torch.int64, device=dev)
        want = eval_batch(args, base, ex, batch_from_pack(buf, *ev, rows))
        got = eval_batch(args, base, ex, batch_from_pack(buf, *ev, rows), device_metrics=True)
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float64
        assert tuple(got.shape) == (len(FIGURES) + 1,)
        got = got.cpu().numpy()
        assert got[THRESHOLD_RAN] == want[THRESHOLD_RAN] == 1.0
        check_figures(dict(zip(FIGURES, got)), dict(zip(FIGURES, want)), f"batch {k}")
    # without threshold_test the ratio figures are NaN and the flag is 0, as in the default row
    args = _args(test_threshold=False)
    rows = torch.arange(0, args.test_bs, dtype=torch.int64, device=dev)
    want = eval_batch(args, base, ex, batch_from_pack(buf, *ev, rows))
    got = eval_batch(args, base, ex, batch_from_pack(buf, *ev, rows), device_metrics=True).cpu().numpy()
    assert got[THRESHOLD_RAN] == want[THRESHOLD_RAN] == 0.0 and np.isnan(got[8:THRESHOLD_RAN]).all()
    check_figures(dict(zip(FIGURES[:8], got)), dict(zip(FIGURES[:8], want)), "no threshold_test")


def test_eval_epoch_device_metrics_without_sklearn(dev, setup, monkeypatch):
    import sklearn.metrics

    from tempme_amd import evaluate, fidelity
    buf, ev, base, ex = setup
    args = _args()
    want = evaluate.eval_one_epoch(args, base, ex, buf, *ev)

    def refuse(*a, **k):
        raise AssertionError("scikit-learn was called on the device-metrics path")
    monkeypatch.setattr(sklearn.metrics, "average_precision_score", refuse)
    monkeypatch.setattr(sklearn.metrics, "roc_auc_score", refuse)
    monkeypatch.setattr(evaluate, "_metrics_sklearn", refuse)
    monkeypatch.setattr(fidelity, "average_precision_score", refuse)
    monkeypatch.setattr(fidelity, "roc_auc_score", refuse)
    got = evaluate.eval_one_epoch(args, base, ex, buf, *ev, device_metrics=True)
    assert got.keys() == want.keys() and got["n_batches"] == want["n_batches"] > 3
    check_figures(got, want, "epoch")


def test_gather_rows_device_rows_through_a_collective(dev):
    """Device tensor rows handed to the all_gather on their own device (a world-1 group in this process): the
    rows are padded and gathered as device tensors and equal the numpy rows' result."""
    import torch.distributed as dist

    from tempme_amd.evaluate import FIGURES, gather_rows
    assert not dist.is_initialized()
    rng = np.random.default_rng(1)
    rows = {k: rng.uniform(size=len(FIGURES) + 1) for k in (4, 1, 2)}
    rows[2][1] = np.nan
    want = gather_rows(rows)
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        got = gather_rows({k: torch.from_numpy(r).to(dev) for k, r in rows.items()}, 1, device=dev, collective=True)
    finally:
        dist.destroy_process_group()
    np.testing.assert_array_equal(got, want)


def test_threshold_test_device(dev, setup):
    from tempme_amd import fidelity
    from tempme_amd.train import batch_from_pack, encode_sides, explain_sides, prepare_step
    buf, ev, base, ex = setup
    args = _args()
    b = batch_from_pack(buf, *ev, torch.arange(40, 80, dtype=torch.int64, device=dev))
    with torch.no_grad():
        kw, pos_o, neg_o, y_ori = prepare_step(base, b)
        expl0 = explain_sides(ex, b, encode_sides(ex, b), False)
    a = (args, expl0, base, b.src, b.dst, b.fake, b.ts, b.e_idx, pos_o, neg_o, y_ori, *b.subgraphs)
    want = fidelity.threshold_test(*a)
    got = fidelity.threshold_test(*a, device_metrics=True)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (5,)
    names = ("ratio_aps", "ratio_auc", "ratio_acc", "ratio_prob", "ratio_logit")
    check_figures(dict(zip(names, got.cpu().numpy())), dict(zip(names, want)), "threshold_test")


def test_step_metrics_device(dev, setup):
    import tempme_amd as tm
    from tempme_amd.train import batch_from_pack, step_metrics, steps_metrics_device, train_step
    buf, ev, base, _ = setup
    torch.manual_seed(6)
    ex = tm.TempME(base, "tgn", "enron", out_dim=40, hid_dim=64, device=dev,     # its own: the steps train it
                   null_model={k: 1.0 / 12 for k in range(1, 13)}).to(dev).train()
    opt = torch.optim.Adam(ex.parameters(), lr=1e-3)
    outs = [train_step(ex, base, opt, batch_from_pack(buf, *ev, torch.arange(s, e, device=dev)), if_bern=False)
            for s, e in ((0, 40), (40, 80), (80, 104))]                  # the last batch is shorter
    want = [step_metrics(o) for o in outs]
    got = steps_metrics_device(outs)
    one = step_metrics(outs[1], device=True)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.keys() == w.keys()
        assert all(v.is_cuda and v.dtype == torch.float64 and v.dim() == 0 for v in g.values())
        check_figures({n: v.item() for n, v in g.items()}, w, f"step {k}")
    assert one.keys() == got[1].keys()
    assert all(np.float64(one[n].item()).tobytes() == np.float64(got[1][n].item()).tobytes() for n in one)


def test_train_epoch_device_metrics(dev, setup, monkeypatch):
    """train.train_epoch(metrics=True, device_metrics=True): one dict of device scalars per step, the epoch's
    shorter last batch included, equal to step_metrics of the same step outputs (200 scores per step)."""
    import tempme_amd as tm
    from tempme_amd import train
    buf, ev, base, _ = setup
    torch.manual_seed(6)
    ex = tm.TempME(base, "tgn", "enron", out_dim=40, hid_dim=64, device=dev,
                   null_model={k: 1.0 / 12 for k in range(1, 13)}).to(dev)
    opt = torch.optim.Adam(ex.parameters(), lr=1e-3)
    seen, inner = [], train.steps_metrics_device

    def recording(outs):
        seen.extend(outs)
        return inner(outs)
    monkeypatch.setattr(train, "steps_metrics_device", recording)
    devm = train.train_epoch(ex, base, opt, buf, *ev, 100, generator=torch.Generator().manual_seed(1),
                             if_bern=False, metrics=True, device_metrics=True)
    spans = train.epoch_spans(int(ev[0].shape[0]) - 1, 100)
    assert len(devm) == len(seen) == len(spans) > 2 and spans[-1][1] - spans[-1][0] < 100
    for k, (g, o) in enumerate(zip(devm, seen)):
        assert all(v.is_cuda and v.dtype == torch.float64 for v in g.values())
        check_figures({n: v.item() for n, v in g.items()}, train.step_metrics(o), f"epoch step {k}",
                      tol=(2 * 100 + 2) * RR.EPS)


def test_learn_base_train_epoch_device_metrics(dev):
    """learn_base.train_epoch with a TGN on the uslegis fixture, 3 steps at bs = 32: the same seeds give the same
    steps, so the two epochs differ in where their metrics are computed only.  64 scores per step."""
    import pandas as pd

    from tempme_amd import learn_base
    from tempme_amd.tgn import TGN
    G = os.path.join(TI.G, "data")
    g_df = pd.read_csv(os.path.join(G, "ml_uslegis_sampled.csv"))
    ef = np.load(os.path.join(G, "ml_uslegis_sampled.npy"))
    nf = np.load(os.path.join(G, "ml_uslegis_sampled_node.npy"))
    sp = learn_base.split_data(g_df, device=dev)
    idx = np.random.default_rng(0).permutation(len(sp.train_src_l))
    runs = []
    for device_metrics in (False, True):
        torch.manual_seed(3)
        m = TGN(nf, ef, n_neighbors=20, device=dev, n_layers=2, n_heads=2, dropout=0.1).to(dev)
        m.train_on_hip()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        runs.append(learn_base.train_epoch(m, opt, sp.train_ngh_finder, sp.train_rand_sampler, sp.train_src_l,
                                           sp.train_dst_l, sp.train_ts_l, sp.train_e_idx_l, 32, idx_list=idx,
                                           max_steps=3, device_metrics=device_metrics))
        m.check_errors()
    host, devm = runs
    print("host", host, "device", devm)
    assert host["loss"] == devm["loss"] and len(host["loss"]) == 3
    assert np.float64(host["acc"]).tobytes() == np.float64(devm["acc"]).tobytes()
    tol = (2 * 32 + 2) * RR.EPS
    assert RR.close(devm["ap"], host["ap"], tol) and RR.close(devm["auc"], host["auc"], tol)
    # a shorter last batch gets its own launch
    pairs = [(torch.randn(32, device=dev), torch.randn(32, device=dev)) for _ in range(2)]
    pairs.append((torch.randn(7, device=dev), torch.randn(7, device=dev)))
    want = np.array([learn_base._metrics(p, n) for p, n in pairs])
    got = learn_base._metrics_device(pairs)
    assert got.shape == (3, 3) and got[:, 0].tobytes() == want[:, 0].tobytes()
    assert RR.close(got[:, 1:], want[:, 1:], tol)
