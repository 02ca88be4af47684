"""Timing of ranked_edges at the headline shape (full-Enron-shaped graph, N = 20, M = 3, k = 20, pairs=True) for
B = 100 and B = 512 events, through HIP events and tm_profile_*:

  (a) ExplainPipeline.ranked_edges on the pipeline's buffers after run(): the whole call (the tm_ranked_edges launch
      plus the torch gathers of node / center / ts / hop), and ranked_edges_kernel alone from tm_profile_*;
  (b) a torch-op formulation of the same result on the same device and tensors: a stable sort of every prediction's
      entries by edge id, segment maximum / count / first slot by scatter, a stable sort by score.  It is written here,
      not in the product; its (eid, score, mult, count) are compared with the kernel's before timing.

HIP-event medians of 20 runs after 3 warm-up runs.

    python tools/ranked_edges_profile.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tempme_amd as tm  # noqa: E402
from tempme_amd import _lib as L  # noqa: E402
from tempme_amd.pipeline import ExplainPipeline  # noqa: E402
from tempme_amd.workload import enron_like, split  # noqa: E402

RUNS, WARM = 20, 3
N, M, K, HID = 20, 3, 20, 64


def timed(fn, runs=RUNS):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    L.profile_enable(True)
    for _ in range(runs):
        fn()
    prof = L.profile_read()
    L.profile_enable(False)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "runs": runs,
            "kernels": {k: {"ms_per_run": v[0] / runs, "launches_per_run": v[1] / runs} for k, v in sorted(prof.items())}}


def torch_formulation(imp, node, eid, groups, k):
    """(eid, score, mult [G, k], count [G]) of the predictions ``groups`` [G, R] from [rows, ne] records, in torch ops
    (no NaN handling: the pipeline's scores have none)."""
    G, R = groups.shape
    g = groups.long()
    e = eid[g].reshape(G, -1)
    live = (node[g].reshape(G, -1) != 0) & (e > 0)
    s = imp[g].reshape(G, -1)
    T = e.shape[1]
    big = torch.iinfo(torch.int32).max
    se, order = torch.sort(torch.where(live, e, torch.full_like(e, big)), dim=1, stable=True)
    ss, sl = s.gather(1, order), se != big
    head = torch.ones_like(sl)
    head[:, 1:] = se[:, 1:] != se[:, :-1]
    head &= sl
    count = head.sum(1)
    seg = torch.where(sl, head.long().cumsum(1) - 1, T - 1)      # dead entries: the last segment, never a real one
    seg = seg.clamp(min=0)
    neg = torch.full((G, T), float("-inf"), device=imp.device)
    best = neg.scatter_reduce(1, seg, torch.where(sl, ss, neg), "amax", include_self=True)
    mult = torch.zeros((G, T), dtype=torch.int32, device=imp.device).scatter_add_(1, seg, sl.int())
    seid = torch.zeros((G, T), dtype=torch.int32, device=imp.device).scatter_(1, seg, torch.where(sl, se, 0))
    real = torch.arange(T, device=imp.device).unsqueeze(0) < count.unsqueeze(1)
    best = torch.where(real, best, neg)
    top, perm = torch.sort(best, dim=1, descending=True, stable=True)
    perm, keep = perm[:, :k], real.gather(1, perm[:, :k])
    z = lambda x: torch.where(keep, x, torch.zeros_like(x))  # noqa: E731
    return z(seid.gather(1, perm)), z(top[:, :k]), z(mult.gather(1, perm)), count.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = L.require_device()
    g = enron_like(n_nodes=184, n_edges=125235)
    (src, dst, ts, eidx), rows, pool = split(g)
    f = tm.NeighborFinder.from_edges(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"],
                                     device=dev, seed=1)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731

    class Base:
        n_feat_th = torch.from_numpy(g["n_feat"])
        e_feat_th = torch.from_numpy(g["e_feat"])
        node_raw_features = torch.nn.Embedding.from_pretrained(n_feat_th, padding_idx=0, freeze=True)
        edge_raw_features = torch.nn.Embedding.from_pretrained(e_feat_th, padding_idx=0, freeze=True)

    torch.manual_seed(0)
    ex = tm.TempME(Base(), "tgn", "enron", 40, HID, device=dev, null_model={k: 1 / 12 for k in range(1, 13)}).to(dev).eval()
    res = {"shape": dict(N=N, M=M, k=K, pairs=True, entries_per_prediction=2 * (N + N * N), padded=1024)}
    for B in (100, 512):
        pipe = ExplainPipeline(ex, f.graph, to(pool, np.int32), N, M, B, seed=1)
        with torch.no_grad():
            _, h1, h2 = pipe.run(to(src[:B], np.int32), to(dst[:B], np.int32), to(ts[:B], np.float64),
                                 to(eidx[:B], np.int32), torch.arange(B, dtype=torch.int32, device=dev))
        pipe.check_errors()
        b = pipe.buf
        imp = torch.cat([h1.reshape(3 * B, N), h2.reshape(3 * B, N * N)], 1)
        node = torch.cat([b.sub1_node.reshape(3 * B, N), b.sub2_node.reshape(3 * B, N * N)], 1)
        eid = torch.cat([b.sub1_eid.reshape(3 * B, N), b.sub2_eid.reshape(3 * B, N * N)], 1)
        i = torch.arange(B, dtype=torch.int32, device=dev)
        groups = torch.cat([torch.stack([i, i + B], 1), torch.stack([i, i + 2 * B], 1)])
        got = pipe.ranked_edges(K)
        want = torch_formulation(imp, node, eid, groups, K)
        same = all(torch.equal(a.reshape(w.shape), w) for a, w in
                   zip((got.eid, got.score, got.mult, got.count), want))
        r = {"predictions": 2 * B, "mean_distinct_edges": float(got.count.float().mean()),
             "torch_formulation_equal": bool(same),
             "ranked_edges": timed(lambda: pipe.ranked_edges(K)),
             "torch_formulation": timed(lambda: torch_formulation(imp, node, eid, groups, K))}
        kern = r["ranked_edges"]["kernels"]["ranked_edges_kernel"]["ms_per_run"]
        r["kernel_ms"] = kern
        r["torch_over_call"] = r["torch_formulation"]["median_ms"] / r["ranked_edges"]["median_ms"]
        r["torch_over_kernel"] = r["torch_formulation"]["median_ms"] / kern
        res[f"B{B}"] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
