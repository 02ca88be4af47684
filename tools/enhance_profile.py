"""Timing of the motif-enhanced link predictor at the headline shape (full-Enron-shaped graph, B=100 events,
N=20, M=3 walks per hop-1 slot, de=32 / dn=172 with zero node features, the three sides), through HIP events and
tm_profile_*:

  (a) the pooled encoder launch (tm_encoder_pool_fwd, walk_pool_kernel + pool_tail_kernel) beside
      tm_encoder_fwd_tab (walk_kernel) on the same walks and table;
  (b) TempME.enhance_predict_agg in eval (HIP path) beside the torch-op formulation on the same device (both in
      eval mode without gradients, on the host arrays enhance_main.py's loop passes);
  (c) the walk-importance kernel alone;
and the pooled kernel's executed FLOP per walk (bench.flops_model's executed terms minus the scoring MLP's three
products) with its fraction of the fp32 MFMA peak.  A second block repeats (a) at 24 batches (the bench's
persistent-grid regime).

--leg train measures the training step's half instead: enhance_predict_agg forward + backward in train mode
(attention dropouts at p = 0.1) on the same B = 100 inputs, through the pooled encoder's training kernels
(tm_encoder_pool_train_fwd / _bwd / _wgrad) and through _enhance_agg_torch + backward (the torch-op formulation,
the only training path before those kernels) in the same process; tm_profile_* gives the library's kernels,
--torch-kernels adds torch.profiler's device-kernel totals of the torch-op leg.

    python tools/enhance_profile.py [--leg eval|train] [--torch-kernels] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tempme_amd as tm  # noqa: E402
from tempme_amd import _lib as L  # noqa: E402
from tempme_amd.preprocess import sample_events  # noqa: E402
from tempme_amd.workload import enron_like, split  # noqa: E402

RUNS, WARM = 20, 3
B, N, M, HID = 100, 20, 3, 64


def timed(fn, runs=RUNS):
    """Wall time per call without the profiler's events, then the per-kernel totals of as many profiled calls."""
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


def train_leg(ex, call, torch_call, gats, torch_kernels):
    """Forward + backward of enhance_predict_agg in train mode: the HIP training path and the torch-op formulation."""
    ex.train()
    params = [p for p in ex.parameters() if p.requires_grad]

    def step(fn):
        def run():
            for p in params:
                p.grad = None
            for g_ in gats:
                g_.grad = None
            pos, neg = fn()
            (pos.sum() + neg.sum()).backward()
        return run

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    assert ex._enhance_train(), "the HIP training path does not serve this module"
    res = {"dropout_p": ex._enhance_drop_p(),
           "hip_fwd_bwd": timed(step(call)), "torch_fwd_bwd": timed(step(torch_call)),
           "hip_fwd_only": timed(fwd(call)), "torch_fwd_only": timed(fwd(torch_call))}
    res["speedup_fwd_bwd"] = res["torch_fwd_bwd"]["median_ms"] / res["hip_fwd_bwd"]["median_ms"]
    res["speedup_fwd_only"] = res["torch_fwd_only"]["median_ms"] / res["hip_fwd_only"]["median_ms"]
    if torch_kernels:
        from torch.profiler import ProfilerActivity, profile
        for tag, fn in (("hip", step(call)), ("torch", step(torch_call))):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(RUNS):
                    fn()
                torch.cuda.synchronize()
            rows = sorted(prof.key_averages(), key=lambda e: -e.device_time_total)
            res[tag + "_device_kernels"] = {
                "total_ms_per_run": sum(e.device_time_total for e in rows) / RUNS / 1e3, "kernel_names": len(rows),
                "top": [{"name": e.key[:100], "ms_per_run": e.device_time_total / RUNS / 1e3,
                         "launches_per_run": e.count / RUNS} for e in rows[:12]]}
    ex.eval()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=("eval", "train"), default="eval")
    ap.add_argument("--torch-kernels", action="store_true")
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
    ex.set_node_degree(tm.compute_node_degrees(g["src"], g["dst"], g["n_nodes"]))
    res = {"shape": dict(B=B, N=N, M=M, W=N * M, de=32, dn=172, hid=HID, sides=3, zero_node_features=True)}
    fm = bench.flops_model(32, 172, HID, N, M, etab=True, zn=True)
    pool_flop = fm["walk_kernel_executed"] - 2 * ((HID + 12) * HID + HID * (HID + 12) + HID)
    res["flop_per_walk"] = {"walk_kernel_executed": fm["walk_kernel_executed"], "walk_pool_kernel_executed": pool_flop}
    etab = ex.dropin_edge_table()
    w = ex.packed_weights()
    for tag, E in ((("headline_B100", B), ("persistent_24x100", 24 * B)) if args.leg == "eval" else (("train_B100", B),)):
        ev = (to(src[:E], np.int32), to(dst[:E], np.int32), to(ts[:E], np.float64), to(eidx[:E], np.int32))
        buf = sample_events(f.graph, 1, tm.SPLIT_TEST, N, M, *ev, torch.arange(E, dtype=torch.int32, device=dev),
                            to(pool, np.int32))
        W = N * M
        cut = ev[2].reshape(1, E).expand(3, E).contiguous()
        walk_args = (buf.node6, buf.eid3, buf.ts3, buf.cat, cut, buf.cnt, 3, E, W)
        wgt = ex.walk_importance_groups(buf.node6, buf.ts3, cut, 3, E, W)
        n_walks = 3 * E * W
        ws = torch.empty(L.lib().tm_encoder_pool_workspace_bytes(w, n_walks), dtype=torch.uint8, device=dev)
        out = torch.empty(3, E, HID + 12, device=dev)
        imp = torch.empty(n_walks, device=dev)
        nt, et = ex.feature_tables()
        if args.leg == "train":
            h = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
            sides = [((h(buf.node6[s]), h(buf.eid3[s]), h(buf.ts3[s]), h(buf.cat[s])[..., None], None), h(buf.cnt[s]))
                     for s in range(3)]
            gats = [torch.randn(E, 172, device=dev, requires_grad=True) for _ in range(3)]
            cut_h = ts[:E].astype(np.float64)
            res["agg_train"] = train_leg(
                ex, lambda: ex.enhance_predict_agg(cut_h, sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides], *gats),
                lambda: ex._enhance_agg_torch(cut_h, sides, gats), gats, args.torch_kernels)
            break

        def pool_fwd():
            L.check(L.lib().tm_encoder_pool_fwd(w, L.ptr(nt), L.ptr(et), L.ptr(etab), 3, E, W, M, L.ptr(buf.node6),
                                                L.ptr(buf.eid3), L.ptr(buf.ts3), L.ptr(buf.cat), L.ptr(cut),
                                                L.ptr(buf.cnt), L.ptr(wgt), L.ptr(ws), L.ptr(out), HID + 12,
                                                L.stream_ptr(dev)), "tm_encoder_pool_fwd")

        def score_fwd():
            ex.encoder_fwd(*walk_args, out=imp, workspace=ws, M=M, etab=etab, w=w)

        r = {"pool_fwd": timed(pool_fwd), "encoder_fwd_tab": timed(score_fwd),
             "walk_importance": timed(lambda: ex.walk_importance_groups(buf.node6, buf.ts3, cut, 3, E, W, check=False)),
             "enhance_groups": timed(lambda: ex.enhance_groups(*walk_args, M=M, etab=etab, check=False))}
        k = r["pool_fwd"]["kernels"]["walk_pool_kernel"]["ms_per_run"]
        tf = pool_flop * n_walks / (k * 1e-3) / 1e12
        r["walk_pool_kernel_tflops"] = tf
        r["walk_pool_kernel_frac_fp32_mfma"] = tf / bench.FP32_MFMA_PEAK_TF
        k0 = r["encoder_fwd_tab"]["kernels"]["walk_kernel"]["ms_per_run"]
        r["walk_kernel_tflops"] = fm["walk_kernel_executed"] * n_walks / (k0 * 1e-3) / 1e12
        res[tag] = r
        if E != B:
            continue
        # (b) the drop-in call on host arrays, as enhance_main.py's loop makes it: eval HIP path vs torch ops
        h = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
        sides = [((h(buf.node6[s]), h(buf.eid3[s]), h(buf.ts3[s]), h(buf.cat[s])[..., None], None), h(buf.cnt[s]))
                 for s in range(3)]
        gats = [torch.randn(E, 172, device=dev) for _ in range(3)]
        cut_h = ts[:E].astype(np.float64)
        call = lambda: ex.enhance_predict_agg(cut_h, sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides], *gats)  # noqa: E731

        def hip():
            with torch.no_grad():
                return call()

        def torch_ops():
            with torch.no_grad():
                return ex._enhance_agg_torch(cut_h, sides, gats)

        res["agg_eval_hip"] = timed(hip)
        res["agg_torch_ops"] = timed(torch_ops)
        a, b_ = torch.cat(hip()), torch.cat(torch_ops())
        res["agg_hip_vs_torch_max_abs"] = float((a - b_).abs().max())
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
