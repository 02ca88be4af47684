"""Timing of tm_ranked_motifs and tm_motif_mask at the headline shape (full-Enron-shaped graph, N = 20, M = 3, W = 60,
k = 20) for B = 100 and B = 512 events, with pairs (2 B predictions of 120 walks) and with rows (3 B of 60):

  (a) ranked_motifs_kernel and motif_mask_kernel alone, from tm_profile_* around the C entry points, and the whole
      Python calls (ExplainPipeline.ranked_motifs: the launch plus the torch gathers of node / ts;
      fidelity.motif_masked_nodes for m = 1, 5, 20 on the [hop-1 | hop-2] records) by HIP events;
  (b) a torch-op formulation of the same ranking on the same device and tensors: torch.unique over (prediction,
      packed triple) rows, scatter-max / scatter-add per instance, two stable sorts.  It is written here, not in the
      product; the triple is packed into 63 bits, which the graph's edge ids allow and the kernel does not need; its
      (eid, score, mult, count) are compared with the kernel's before timing, and the device kernels one call launches
      are counted with torch.profiler.

Medians of 20 runs after 5 warm-up runs.

    python tools/ranked_motifs_profile.py [--out FILE]
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
from tempme_amd import fidelity  # noqa: E402
from tempme_amd.pipeline import ExplainPipeline  # noqa: E402
from tempme_amd.workload import enron_like, split  # noqa: E402

RUNS, WARM = 20, 5
N, M, K, HID = 20, 3, 20, 64
M_LIST = [1, 5, 20]


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


def device_launches(fn):
    """the device kernels one call of ``fn`` launches (torch.profiler), or None where the profiler gives none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as p:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in p.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:            # noqa: BLE001  (a count is a footnote of the timing, not a reason to lose it)
        return None


def torch_formulation(imp, eid3, cat, groups, k):
    """(eid [G, k, 3], score, mult [G, k], count [G]) of the predictions ``groups`` [G, R] from [rows, W] walks, in
    torch ops (no NaN handling: the pipeline's scores have none; edge ids below 2^21)."""
    G = groups.shape[0]
    g = groups.long()
    e = eid3[g].reshape(G, -1, 3).long()
    c = cat[g].reshape(G, -1)
    s = imp[g].reshape(G, -1)
    live = (e[..., 0] > 0) & (c >= 0) & (c < 12)
    packed = torch.where(live, (e[..., 0] << 42) | (e[..., 1] << 21) | e[..., 2], -1)
    gid = torch.arange(G, device=imp.device).unsqueeze(1).expand_as(packed)
    uniq, inv = torch.unique(torch.stack([gid, packed], -1).reshape(-1, 2), dim=0, return_inverse=True)
    U = uniq.shape[0]
    neg = torch.full((U,), float("-inf"), device=imp.device)
    best = neg.scatter_reduce(0, inv, s.reshape(-1), "amax", include_self=True)
    mult = torch.zeros(U, dtype=torch.int32, device=imp.device).scatter_add_(0, inv, live.reshape(-1).int())
    ug, real = uniq[:, 0], uniq[:, 1] >= 0
    best = torch.where(real, best, neg)                       # a prediction's dead entries: one row, ranked last
    o1 = torch.sort(best, descending=True, stable=True).indices
    o2 = torch.sort(ug[o1], stable=True).indices
    perm = o1[o2]                                             # by prediction, score descending, packed ascending
    per = torch.bincount(ug, minlength=G)
    start = per.cumsum(0) - per
    pos = torch.arange(U, device=imp.device) - start[ug[perm]]
    keep = real[perm] & (pos < k)
    flat = (ug[perm] * k + pos)[keep]
    pk = uniq[perm, 1][keep]
    o_eid = torch.zeros((G * k, 3), dtype=torch.int32, device=imp.device)
    o_eid[flat] = torch.stack([pk >> 42, (pk >> 21) & 0x1FFFFF, pk & 0x1FFFFF], -1).int()
    o_score = torch.zeros(G * k, device=imp.device)
    o_score[flat] = best[perm][keep]
    o_mult = torch.zeros(G * k, dtype=torch.int32, device=imp.device)
    o_mult[flat] = mult[perm][keep]
    count = torch.zeros(G, dtype=torch.int32, device=imp.device).scatter_add_(0, ug, real.int())
    return o_eid.view(G, k, 3), o_score.view(G, k), o_mult.view(G, k), count


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
    W = N * M
    res = {"shape": dict(N=N, M=M, W=W, k=K, m_list=M_LIST, runs=RUNS, warmup=WARM)}
    for B in (100, 512):
        pipe = ExplainPipeline(ex, f.graph, to(pool, np.int32), N, M, B, seed=1)
        with torch.no_grad():
            imp3, _, _ = pipe.run(to(src[:B], np.int32), to(dst[:B], np.int32), to(ts[:B], np.float64),
                                  to(eidx[:B], np.int32), torch.arange(B, dtype=torch.int32, device=dev))
        pipe.check_errors()
        b = pipe.buf
        imp, eid3, cat = imp3.reshape(3 * B, W), b.eid3.view(3 * B, W, 3), b.cat.view(3 * B, W)
        i = torch.arange(B, dtype=torch.int32, device=dev)
        tables = {"pairs": torch.cat([torch.stack([i, i + B], 1), torch.stack([i, i + 2 * B], 1)]),
                  "rows": torch.arange(3 * B, dtype=torch.int32, device=dev).view(-1, 1)}
        sgs = [([b.sub1_node[s], b.sub2_node[s]], [b.sub1_eid[s], b.sub2_eid[s]]) for s in range(3)]
        for mode, groups in tables.items():
            pairs = mode == "pairs"
            got = pipe.ranked_motifs(K, pairs=pairs)
            want = torch_formulation(imp, eid3, cat, groups, K)
            same = all(torch.equal(a.reshape(w.shape), w) for a, w in
                       zip((got.eid, got.score, got.mult, got.count), want))
            r = {"predictions": int(groups.shape[0]), "entries_per_prediction": int(groups.shape[1]) * W,
                 "mean_distinct_instances": float(got.count.float().mean()),
                 "mean_live_walks": float(got.cat_n.sum(-1).float().mean()),
                 "torch_formulation_equal": bool(same),
                 "ranked_motifs": timed(lambda: pipe.ranked_motifs(K, pairs=pairs)),
                 "torch_formulation": timed(lambda: torch_formulation(imp, eid3, cat, groups, K)),
                 "torch_formulation_device_launches": device_launches(
                     lambda: torch_formulation(imp, eid3, cat, groups, K))}
            kern = r["ranked_motifs"]["kernels"]["ranked_motifs_kernel"]["ms_per_run"]
            r["kernel_ms"] = kern
            r["torch_over_call"] = r["torch_formulation"]["median_ms"] / r["ranked_motifs"]["median_ms"]
            r["torch_over_kernel"] = r["torch_formulation"]["median_ms"] / kern
            if not pairs:
                r["motif_masked_nodes"] = timed(lambda: fidelity.motif_masked_nodes(got, sgs, N, M_LIST, 2))
                r["mask_kernel_ms"] = r["motif_masked_nodes"]["kernels"]["motif_mask_kernel"]["ms_per_run"]
            res[f"B{B}_{mode}"] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
