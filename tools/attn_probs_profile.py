"""Timing of the attention-probability kernels (tm_tgn_attn_probs / tm_tgat_attn_probs, csrc/attn_probs.h) beside
the attention forward (tm_*_attn_fwd) on the same descriptor, through tm_profile_*.

Shapes: 6,000 rows (the hop-2 pass of a contrast at bs = 100: 3 sides x 100 events x 20 hop-1 nodes) and 120,000 rows
(bs = 2,000), N = 20, H = 2, gathered node and edge tables; keys (172, 172, 172) = 516 columns (Wikipedia / Reddit
widths) and (172, 32, 172) = 376 columns (the headline base: the Enron-shaped workload's node and edge widths).  A
fifth of the slots are padding (node 0, masked).  Per kernel: the median over 20 single launches after 3 warm-up
launches, each read from tm_profile_* on its own; ``probs+mean`` stores both outputs, ``mean`` only the head mean.

    python tools/attn_probs_profile.py [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tempme_amd import _lib as L  # noqa: E402

RUNS, WARM = 20, 3
N, H = 20, 2
NODES, EDGES = 184, 125236
SHAPES = [(6000, (172, 172, 172)), (120000, (172, 172, 172)), (6000, (172, 32, 172)), (120000, (172, 32, 172))]


def descriptor(dev, rows, dims, flavour, seed=0):
    dn, de, dtm = dims
    dk = dn + de + dtm
    gen = torch.Generator(device=dev).manual_seed(seed)
    f32 = dict(dtype=torch.float32, device=dev)
    t = dict(node_tab=torch.randn(NODES, dn, generator=gen, **f32), edge_tab=torch.randn(EDGES, de, generator=gen, **f32),
             node_idx=torch.randint(1, NODES, (rows, N), generator=gen, dtype=torch.int32, device=dev),
             edge_idx=torch.randint(1, EDGES, (rows, N), generator=gen, dtype=torch.int32, device=dev),
             dt=torch.rand(rows, N, generator=gen, **f32) * 1e5,
             tw=torch.from_numpy((1.0 / 10 ** np.linspace(0, 9, dtm)).astype(np.float32)).to(dev),
             tb=torch.zeros(dtm, **f32), qf=torch.randn(rows, H * dk, generator=gen, **f32),
             err=torch.zeros(1, dtype=torch.int32, device=dev))
    pad = torch.rand(rows, N, generator=gen, device=dev) < 0.2
    t["node_idx"][pad] = 0
    t["edge_idx"][pad] = 0
    a = L.Attn()
    a.rows, a.n_ngh, a.n_head = rows, N, H
    a.d_node, a.d_edge, a.d_time = dims
    a.node_rows, a.edge_rows, a.head_major_rows, a.seg_rows = NODES, EDGES, 1, 0
    a.temperature = float(np.sqrt(dk / H)) if flavour == "tgat" else float(np.sqrt(dk))
    a.node_tab, a.node_idx = t["node_tab"].data_ptr(), t["node_idx"].data_ptr()
    a.edge_tab, a.edge_idx = t["edge_tab"].data_ptr(), t["edge_idx"].data_ptr()
    a.dt, a.time_w, a.time_b = t["dt"].data_ptr(), t["tw"].data_ptr(), t["tb"].data_ptr()
    a.mask_node, a.ew, a.qf = t["node_idx"].data_ptr(), None, t["qf"].data_ptr()
    a.err_flag = t["err"].data_ptr()
    return a, t, dk


def median_ms(fn, label):
    """Median over RUNS single launches of ``label``'s time from tm_profile_*."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        L.profile_enable(True)
        fn()
        total, launches = L.profile_read()[label]
        L.profile_enable(False)
        assert launches == 1
        ms.append(total)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = L.require_device()
    lib = L.lib()
    st = L.stream_ptr(dev)
    lines = ["# tm_profile_* medians (min) in ms over %d single launches after %d warm-up launches; N = %d, H = %d,"
             % (RUNS, WARM, N, H),
             "# gathered node table [%d, d_node] and edge table [%d, d_edge], a fifth of the slots padding" % (NODES, EDGES),
             "# %-5s %8s %-14s %16s %16s %16s %12s" % ("model", "rows", "key", "forward", "probs+mean", "mean only",
                                                      "probs/fwd")]
    for rows, dims in SHAPES:
        for flavour in ("tgn", "tgat"):
            a, t, dk = descriptor(dev, rows, dims, flavour)
            z = torch.empty(rows, H * dk, device=dev)
            stats = torch.empty(rows, H, 2, device=dev)
            probs = torch.empty(rows, H, N, device=dev)
            mean = torch.empty(rows, N, device=dev)
            fwd, prb = getattr(lib, f"tm_{flavour}_attn_fwd"), getattr(lib, f"tm_{flavour}_attn_probs")
            f = median_ms(lambda: L.check(fwd(L.C.byref(a), L.ptr(z), L.ptr(stats), st), "fwd"),
                          f"{flavour}_attn_fwd_kernel")
            p = median_ms(lambda: L.check(prb(L.C.byref(a), L.ptr(probs), L.ptr(mean), st), "probs"),
                          f"{flavour}_attn_probs_kernel")
            m = median_ms(lambda: L.check(prb(L.C.byref(a), None, L.ptr(mean), st), "probs"),
                          f"{flavour}_attn_probs_kernel")
            assert int(t["err"].item()) == 0
            lines.append("  %-5s %8d %-14s %8.4f (%6.4f) %8.4f (%6.4f) %8.4f (%6.4f) %12.3f"
                         % (flavour, rows, "x".join(map(str, dims)), f[0], f[1], p[0], p[1], m[0], m[1], p[0] / f[0]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
