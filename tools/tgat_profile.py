"""Per-kernel timing of one TGAT contrast at the metric's shape (B=100, N=20, node 172 / edge 32 features,
n_head=2, with explanation weights), through tm_profile_*:

  * no-grad contrast with the fused layer tail (tgat_merge_fwd_kernel) and with the torch-op tail,
    RUNS runs each: median wall time per contrast (HIP events) and per-kernel totals;
  * contrast + backward to the explanation weights;
  * the layer tail alone (fused kernel, torch ops) on the hop-1 pass's and the root pass's rows;
  * tm_tgat_attn_bwd beside tm_tgn_attn_bwd on one descriptor (the two structs share their layout) at the
    hop-1 pass's shape (3*B*N rows) and at the root pass's (3*B rows): d_node only (what TGN returns), and
    d_node + d_qf (TGAT's pass 3).

    python tools/tgat_profile.py [--out FILE]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tempme_amd import _lib as L  # noqa: E402
from tempme_amd.tgat import TGAT  # noqa: E402

RUNS, WARM = 20, 3
B, N, DN, DE, H = 100, 20, 172, 32, 2
NODES, EDGES = 2000, 20000


def inputs(rng):
    def sg():
        n1 = rng.integers(1, NODES, (B, N))
        n2 = rng.integers(1, NODES, (B, N * N))
        n1[rng.uniform(size=n1.shape) < 0.2] = 0
        n2[rng.uniform(size=n2.shape) < 0.3] = 0
        e1, e2 = rng.integers(1, EDGES, (B, N)), rng.integers(1, EDGES, (B, N * N))
        t1 = np.sort(rng.uniform(0, 1e6, (B, N)), axis=1)
        t2 = rng.uniform(0, 1e6, (B, N * N))
        return ([n1.astype(np.float64), n2.astype(np.float64)], [e1.astype(np.float64), e2.astype(np.float64)],
                [t1, t2])
    roots = [rng.integers(1, NODES, B) for _ in range(3)]
    return roots, rng.uniform(1e6, 2e6, B), [sg() for _ in range(3)]


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


def bwd_pair(dev, rows, rng):
    """tm_tgn_attn_bwd and tm_tgat_attn_bwd on the same descriptor values (dense node table)."""
    dk = DN + DE + DN
    g = torch.Generator(device="cpu").manual_seed(rows)
    t = dict(node=torch.randn(rows * N, DN, generator=g), edge=torch.randn(rows * N, DE, generator=g),
             dt=torch.rand(rows * N, generator=g) * 1e5, tw=(1.0 / 10 ** torch.linspace(0, 9, DN)).float(),
             tb=torch.randn(DN, generator=g) * 0.5, qf=torch.randn(rows, H * dk, generator=g) * 0.3,
             mask=(torch.rand(rows * N, generator=g) > 0.25).int(), ew=torch.rand(rows * N, generator=g),
             gz=torch.randn(rows, H * dk, generator=g))
    t = {k: v.to(dev).contiguous() for k, v in t.items()}
    out = {}
    for cls, name in ((L.TgnAttn, "tgn"), (L.TgatAttn, "tgat")):
        a = cls()
        a.rows, a.n_ngh, a.n_head, a.d_node, a.d_edge, a.d_time = rows, N, H, DN, DE, DN
        a.head_major_rows, a.seg_rows, a.temperature = 1, rows // 3, float(np.sqrt(dk / H))
        a.node_tab, a.node_idx, a.edge_tab, a.edge_idx = t["node"].data_ptr(), None, t["edge"].data_ptr(), None
        a.dt, a.time_w, a.time_b = t["dt"].data_ptr(), t["tw"].data_ptr(), t["tb"].data_ptr()
        a.mask_node, a.ew, a.qf, a.err_flag = t["mask"].data_ptr(), t["ew"].data_ptr(), t["qf"].data_ptr(), None
        z = torch.empty(rows, H * dk, device=dev)
        stats = torch.empty(rows, H, 2, device=dev)
        parts = torch.empty(rows * H, N, device=dev)
        d_node, d_qf = torch.empty(rows * N, DN, device=dev), torch.empty(rows, H * dk, device=dev)
        st = L.stream_ptr(dev)
        if name == "tgn":
            L.check(L.lib().tm_tgn_attn_fwd(C.byref(a), L.ptr(z), L.ptr(stats), st))
            out["tgn_attn_bwd d_node"] = timed(lambda: L.check(L.lib().tm_tgn_attn_bwd(
                C.byref(a), L.ptr(stats), L.ptr(t["gz"]), L.ptr(parts), L.ptr(d_node), st)))
        else:
            L.check(L.lib().tm_tgat_attn_fwd(C.byref(a), L.ptr(z), L.ptr(stats), st))
            out["tgat_attn_bwd d_node"] = timed(lambda: L.check(L.lib().tm_tgat_attn_bwd(
                C.byref(a), L.ptr(stats), L.ptr(t["gz"]), L.ptr(parts), L.ptr(d_node), None, st)))
            out["tgat_attn_bwd d_node+d_qf"] = timed(lambda: L.check(L.lib().tm_tgat_attn_bwd(
                C.byref(a), L.ptr(stats), L.ptr(t["gz"]), L.ptr(parts), L.ptr(d_node), L.ptr(d_qf), st)))
    return {k: {"ms": next(iter(v["kernels"].values()))["ms_per_run"]} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = L.require_device()
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    m = TGAT(rng.normal(0, 1, (NODES, DN)).astype(np.float32), rng.normal(0, 1, (EDGES, DE)).astype(np.float32), N,
             num_layers=2, n_head=H).to(dev).eval()
    with torch.no_grad():
        m.time_encoder.phase.normal_(0, 0.5)
    roots, cut, sgs = inputs(rng)
    w = [(torch.rand(B, N, device=dev), torch.rand(B, N * N, device=dev)) for _ in range(3)]
    a = (roots[0], roots[1], roots[2], cut, None, sgs[0], sgs[1], sgs[2])

    def fwd():
        with torch.no_grad():
            return m.contrast(*a, test=True, if_explain=True, exp_weights=[[w[0], w[1]], [w[0], w[2]]])

    def fwd_bwd():
        wg = [tuple(x.clone().requires_grad_(True) for x in p) for p in w]
        pos, neg = m.contrast(*a, test=True, if_explain=True, exp_weights=[[wg[0], wg[1]], [wg[0], wg[2]]])
        (pos.sum() + neg.sum()).backward()

    res = {"shape": dict(B=B, N=N, d_node=DN, d_edge=DE, n_head=H, rows=[3 * B, 3 * B * N, 3 * B])}
    m.fused_tail = True
    res["contrast_fused_tail"] = timed(fwd)
    fused = torch.cat(fwd())
    m.fused_tail = False
    res["contrast_torch_tail"] = timed(fwd)
    res["fused_vs_torch_max_abs"] = float((fused - torch.cat(fwd())).abs().max())
    m.fused_tail = True
    res["contrast_fwd_bwd"] = timed(fwd_bwd)
    # the layer tail alone, fused kernel and torch ops, on the hop-1 pass's rows and on the root pass's
    from tempme_amd.tgat import merge_fwd, merge_torch
    lw = m._pack()["models"][0]
    for rows in (3 * B * N, 3 * B):
        z, q = torch.randn(rows, H * (2 * DN + DE), device=dev), torch.randn(rows, 2 * DN + DE, device=dev)
        with torch.no_grad():
            res[f"tail_rows{rows}"] = {"fused_median_ms": timed(lambda: merge_fwd(z, q, lw, DN))["median_ms"],
                                       "torch_median_ms": timed(lambda: merge_torch(z, q, lw, DN))["median_ms"]}
    res["attn_bwd_hop1_rows"] = bwd_pair(dev, 3 * B * N, rng)
    res["attn_bwd_root_rows"] = bwd_pair(dev, 3 * B, rng)
    m.check_errors()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
