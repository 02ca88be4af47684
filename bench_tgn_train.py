"""Base-TGN training-step time (learn_base.py with --base_type tgn; tempme_amd/learn_base.py).

    python bench_tgn_train.py [--steps 20 --warmup 5 --batch-sizes 100,512 --profile]

One step = learn_base.py:223-239 on a prepared batch (2-hop subgraphs pre-sampled, on the device): zero_grad, the
stateful contrast (forbidden_memory_update=False: pending messages applied, positives persisted, raw messages
stored), BCEWithLogits(pos, 1) + BCEWithLogits(neg, 0), backward, torch.optim.Adam step, memory.detach_memory().
Shapes: d_node = d_time = 172, d_edge = 32, H = 2, N = 20, dropout 0.1, B = 100 and B = 512, 2,000 nodes.
Synthetic features and subgraphs (padding neighbours at rate 0.25), nothing read from disk.  The same batch is
stepped again and again, so from the second step on every root has a message pending.  Two paths on one device:

  hip    TGN.train_on_hip(): tm_tgn_attn_train_fwd / _bwd / _dtab and tm_tgn_rows_reduce (csrc/tgn_train.hip),
         folded projections, the layer tail, the message MLP and the GRU cell as torch ops, the memory state on
         the device without a host synchronisation
  torch  tests/tgn_train_ref.py in fp32: the reference's shape (unfolded w_qs / w_ks / w_vs over every key, bmm,
         masked_fill, softmax, the memory updated for the nodes with a pending message) with autograd; its four
         keep masks drawn on the device every step as the hip path draws its own

Both are timed with HIP events around each step; each figure is the median over the timed steps after the warm-up.
Prints one JSON line per shape and a final summary line.  --profile adds the per-kernel totals of the library's own
launches on the hip path (tm_profile_*).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tests"))


def make_inputs(B, N, dn, de, seed=0):
    rng = np.random.default_rng(seed)
    V, E = 2000, 20000
    nf = rng.uniform(0, 1, (V, dn)).astype(np.float32)
    ef = rng.uniform(0, 1, (E + 1, de)).astype(np.float32)
    nf[0] = ef[0] = 0
    cut = np.floor(rng.uniform(5e7, 1e8, B))
    sgs = []
    for _ in range(3):
        n1 = rng.integers(1, V, (B, N))
        n1[rng.uniform(size=n1.shape) < 0.25] = 0
        n2 = rng.integers(1, V, (B, N, N))
        n2[rng.uniform(size=n2.shape) < 0.25] = 0
        n2[n1 == 0] = 0
        e1 = np.where(n1 > 0, rng.integers(1, E + 1, n1.shape), 0)
        e2 = np.where(n2 > 0, rng.integers(1, E + 1, n2.shape), 0)
        t1 = np.where(n1 > 0, cut[:, None] - np.floor(rng.uniform(0, 1e6, n1.shape)), 0.0)
        t2 = np.where(n2 > 0, t1[:, :, None] - np.floor(rng.uniform(0, 1e6, n2.shape)), 0.0)
        sgs.append(([n1, n2.reshape(B, N * N)], [e1, e2.reshape(B, N * N)], [t1, t2.reshape(B, N * N)]))
    src, dst, fake = (rng.integers(1, V, B) for _ in range(3))
    e_idx = rng.integers(1, E + 1, B)
    return nf, ef, (src, dst, fake, cut, e_idx), sgs


def bce(pos, neg):
    crit = F.binary_cross_entropy_with_logits
    return crit(pos, torch.ones_like(pos)) + crit(neg, torch.zeros_like(neg))


def timed(step, steps, warmup):
    """Median ms of step() (HIP events around each call) and its last return value."""
    ms, out = [], None
    for k in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = step()
        b.record()
        b.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(out)


def device_subgraphs(sgs, dev):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    return [([t(x, torch.int32) for x in n], [t(x, torch.int32) for x in e], [t(x, torch.float64) for x in s])
            for n, e, s in sgs]


def hip_step_fn(model, opt, roots, dsg, dev):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    src, dst, fake = (t(x, torch.long) for x in roots[:3])
    cut, e_idx = t(roots[3], torch.float64), t(roots[4], torch.long)

    def step():
        opt.zero_grad()
        pos, neg = model.contrast(src, dst, fake, cut, e_idx, *dsg, explain_weights=None, edge_attr=None)
        loss = bce(pos, neg)
        loss.backward()
        opt.step()
        model.memory.detach_memory()
        return loss.detach()
    return step


def torch_step_fn(model, roots, dsg, dev, lr, p_drop, N):
    import tgn_train_ref as TR
    H = model.embedding_module.attention_models[0].multi_head_target.n_head
    ref = TR.RefTGN(model.state_dict(), H, torch.float32, dev, exact_time=False)
    opt = torch.optim.Adam(list(ref.trainable().values()), lr=lr)
    batch = (roots[0], roots[1], roots[2], roots[3], roots[4], *dsg)
    R1 = 3 * len(roots[0])
    scale = 1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0

    def step():
        ref.zero_grad()
        keep = model.draw_keep_masks(R1, N) if p_drop > 0 else None
        loss = bce(*ref.step(batch, keep, scale))
        loss.backward()
        opt.step()
        return loss.detach()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-sizes", type=str, default="100,512")
    ap.add_argument("--dim", type=int, default=172)
    ap.add_argument("--edge-dim", type=int, default=32)
    ap.add_argument("--n-degree", type=int, default=20)
    ap.add_argument("--n-head", type=int, default=2)
    ap.add_argument("--drop-out", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--skip-torch", action="store_true", help="time the hip path only")
    args = ap.parse_args()
    from tempme_amd import _lib as L
    from tempme_amd.tgn import TGN
    dev = L.require_device(torch.device("cuda", 0))
    N, dn, de, H = args.n_degree, args.dim, args.edge_dim, args.n_head
    results = []
    for B in (int(x) for x in args.batch_sizes.split(",")):
        nf, ef, roots, sgs = make_inputs(B, N, dn, de)
        dsg = device_subgraphs(sgs, dev)
        torch.manual_seed(0)
        m = TGN(nf, ef, n_neighbors=N, device=dev, n_layers=2, n_heads=H, dropout=args.drop_out).to(dev).train()
        out = {"B": B, "N": N, "d_node": dn, "d_edge": de, "d_time": dn, "H": H, "dropout": args.drop_out,
               "steps": args.steps, "warmup": args.warmup}
        torch_step = None if args.skip_torch else torch_step_fn(m, roots, dsg, dev, args.lr, args.drop_out, N)
        m.train_on_hip()
        opt = torch.optim.Adam(m.parameters(), lr=args.lr)
        hip_step = hip_step_fn(m, opt, roots, dsg, dev)
        if args.profile:
            timed(hip_step, 2, args.warmup)
            L.profile_enable(True)
            timed(hip_step, args.steps, 0)
            prof = L.profile_read()
            L.profile_enable(False)
            out["hip_kernels_ms_per_step"] = {k: round(v[0] / args.steps, 4) for k, v in sorted(prof.items())}
            out["hip_launches_per_step"] = {k: v[1] / args.steps for k, v in sorted(prof.items())}
        m._tgn_train_key = None
        out["hip_ms"], out["hip_last_loss"] = (round(x, 5) for x in timed(hip_step, args.steps, args.warmup))
        assert m._tgn_train_key == (3 * B, N, args.drop_out > 0), "the HIP training path did not run"
        m.check_errors()
        if torch_step is not None:
            out["torch_ms"], out["torch_last_loss"] = (round(x, 5) for x in timed(torch_step, args.steps, args.warmup))
            out["hip_over_torch"] = round(out["hip_ms"] / out["torch_ms"], 4)
        print(json.dumps(out), flush=True)
        results.append(out)
    print(json.dumps({"metric": "base_tgn_train_step_ms", "unit": "ms",
                      "shapes": {str(r["B"]): {k: r[k] for k in ("hip_ms", "torch_ms", "hip_over_torch") if k in r}
                                 for r in results}}), flush=True)


if __name__ == "__main__":
    main()
