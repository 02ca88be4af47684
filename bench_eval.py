"""Evaluation-epoch time with host metrics (scikit-learn per batch) against device metrics (tm_rank_metrics).

    python bench_eval.py [--pairs 3 --skip-train]

Eval: one ``evaluate.eval_one_epoch`` over the test split of the full-Enron-shaped graph bench.py builds
(tempme_amd/workload.py: V = 184, E = 125,235, Pareto 1.2; the test split is the last 15 % of the events), TGN base
(random init, no checkpoint travels), N = 20, test_bs 100, test_threshold on with the ratios 0.01, 0.05, 0.1, 0.2,
0.3.  The default path copies every batch's scores to the host and calls scikit-learn six times per batch; with
``device_metrics=True`` the batch's row stays on the device and the epoch makes one copy.  Both run in this
process, alternating, ``--pairs`` timed pairs after one warm-up epoch each; a window is a host clock around the
epoch with a device synchronise inside it.

Train: the same A/B for one ``learn_base.train_epoch`` of 20 steps at B = 512 on bench_tgn_train.py's shapes
(d_node = d_time = 172, d_edge = 32, H = 2, N = 20, dropout 0.1, 2,000 nodes, 20,000 edges); every epoch starts
from the same freshly seeded model, so the two paths score the same logits.

Prints one JSON line: the epoch times of both paths and the largest difference in any epoch figure.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

RATIOS = [0.01, 0.05, 0.1, 0.2, 0.3]


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, out


def max_diff(a, b):
    """Largest |a[k] - b[k]| over the float figures (NaN on both sides counts as equal, on one side as inf)."""
    worst = 0.0
    for k in a:
        x, y = float(a[k]), float(b[k])
        if np.isnan(x) or np.isnan(y):
            worst = max(worst, 0.0 if (np.isnan(x) and np.isnan(y)) else float("inf"))
        else:
            worst = max(worst, abs(x - y))
    return worst


def ab(run, pairs, dev, prepare=lambda: None):
    """run(prepare(), device_metrics) -> figures; one warm-up each, then ``pairs`` alternating timed pairs
    (``prepare`` runs outside the timed window)."""
    run(prepare(), False)
    run(prepare(), True)
    host, devm, diffs = [], [], []
    for _ in range(pairs):
        state = prepare()
        th, fh = timed(lambda: run(state, False), dev)
        state = prepare()
        td, fd = timed(lambda: run(state, True), dev)
        host.append(round(th, 3))
        devm.append(round(td, 3))
        diffs.append(max_diff(fh, fd))
    return dict(host_ms=host, device_ms=devm, host_median_ms=float(np.median(host)),
                device_median_ms=float(np.median(devm)), pair_diff_ms=[round(h - d, 3) for h, d in zip(host, devm)],
                max_abs_figure_diff=max(diffs), host_figures={k: float(v) for k, v in fh.items()},
                device_figures={k: float(v) for k, v in fd.items()})


def eval_ab(dev, pairs, seed=0):
    import tempme_amd as tm
    from tempme_amd import evaluate
    from tempme_amd.preprocess import sample_events
    from tempme_amd.tgn import TGN
    from tempme_amd.workload import enron_like, split
    N = 20
    g = enron_like(n_nodes=184, n_edges=125235, alpha=1.2, seed=seed)
    (src, dst, ts, eidx), rows, pool = split(g)
    f = tm.NeighborFinder.from_edges(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"],
                                     device=dev, seed=seed, split=tm.SPLIT_TEST)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    ev = (to(src, np.int32), to(dst, np.int32), to(ts, np.float64), to(eidx, np.int32))
    buf = sample_events(f.graph, seed, tm.SPLIT_TEST, N, 3, *ev, torch.arange(len(src), dtype=torch.int32, device=dev),
                        to(pool, np.int32))
    torch.manual_seed(seed)
    base = TGN(g["n_feat"], g["e_feat"], n_neighbors=N, device=dev, n_layers=2, n_heads=2, dropout=0.1)
    base.forbidden_memory_update = True
    base = base.to(dev).eval()
    torch.manual_seed(seed + 1)
    ex = tm.TempME(base, "tgn", "enron", out_dim=40, hid_dim=64, device=dev,
                   null_model={k: 1.0 / 12 for k in range(1, 13)}).to(dev).eval()
    args = SimpleNamespace(test_bs=100, if_bern=False, beta=0.5, prior_p=0.3, test_threshold=True, base_type="tgn",
                           n_degree=N, ratios=list(RATIOS))

    def run(_, device_metrics):
        out = evaluate.eval_one_epoch(args, base, ex, buf, *ev, device_metrics=device_metrics)
        return {k: v for k, v in out.items() if k != "n_batches"}
    res = ab(run, pairs, dev)
    res.update(events=int(len(src)), batches=len(evaluate.eval_spans(len(src) - 1, args.test_bs)), test_bs=100, N=N)
    return res


def train_ab(dev, pairs, seed=0):
    from tempme_amd import learn_base
    from tempme_amd.tgn import TGN
    from tempme_amd.workload import enron_like
    N, B, steps = 20, 512, 20
    g = enron_like(n_nodes=2000, n_edges=20000, de=32, dn=172, seed=seed, node_feat="uniform")
    g_df = {"u": g["src"], "i": g["dst"], "ts": g["ts"], "label": g["label"], "idx": g["eidx"]}
    sp = learn_base.split_data(g_df, device=dev, sampler_seed=seed)
    idx = np.random.default_rng(seed).permutation(len(sp.train_src_l))

    def fresh():
        torch.manual_seed(seed)
        m = TGN(g["n_feat"], g["e_feat"], n_neighbors=N, device=dev, n_layers=2, n_heads=2, dropout=0.1).to(dev)
        m.train_on_hip()
        return m, torch.optim.Adam(m.parameters(), lr=1e-4)

    def run(state, device_metrics):
        m, opt = state
        out = learn_base.train_epoch(m, opt, sp.train_ngh_finder, sp.train_rand_sampler, sp.train_src_l, sp.train_dst_l,
                                     sp.train_ts_l, sp.train_e_idx_l, B, idx_list=idx, max_steps=steps,
                                     device_metrics=device_metrics)
        m.check_errors()
        assert len(out["loss"]) == steps, len(out["loss"])
        return {k: out[k] for k in ("acc", "ap", "auc")}
    res = ab(run, pairs, dev, prepare=fresh)
    res.update(steps=steps, B=B, N=N, train_events=int(len(sp.train_src_l)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-eval", action="store_true")
    a = ap.parse_args()
    from tempme_amd import _lib as L
    dev = L.require_device(torch.device("cuda", 0))
    out = {"metric": "eval_epoch_ms host metrics (scikit-learn) vs device metrics (tm_rank_metrics)", "unit": "ms",
           "pairs": a.pairs}
    if not a.skip_eval:
        out["eval_epoch"] = eval_ab(dev, a.pairs)
    if not a.skip_train:
        out["train_epoch"] = train_ab(dev, a.pairs)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
