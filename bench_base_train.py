"""Base-GraphMixer training-step time (learn_base.py with --base_type graphmixer; tempme_amd/learn_base.py).

    python bench_base_train.py [--steps 20 --warmup 5 --batch-sizes 100,512 --cpu-steps 20 --profile]

One step = learn_base.py:223-237 on a prepared batch (subgraphs pre-sampled): zero_grad, contrast,
BCEWithLogits(pos, 1) + BCEWithLogits(neg, 0), backward, torch.optim.Adam step.  Shapes: C = T = 172, N = 30,
L = 3, dropout 0.5 (learn_base.py's defaults at BASELINE configs[4]'s dims), B = 100 and B = 512 (--bs).
Synthetic features and subgraphs (padding neighbours at rate 0.25), nothing read from disk.  Three paths:

  hip    GraphMixer.train_on_hip(): tm_gm_train_fwd / tm_gm_train_bwd (csrc/graphmixer_train.hip)
  torch  the same model with train_on_hip(False): the torch formulation with autograd on the same device
  cpu    the torch formulation on the host cores (torch's own thread count)

hip and torch are timed with HIP events around each step, cpu with the wall clock; each figure is the median over
the timed steps after the warm-up.  Prints one JSON line per shape and a final summary line.  --profile adds the
per-kernel totals of the hip path (tm_profile_*: HIP events around every launch of the library).
"""
import argparse
import copy
import json
import time

import numpy as np
import torch
import torch.nn.functional as F


def make_inputs(B, N, C, seed=0):
    rng = np.random.default_rng(seed)
    V, E = 2000, 20000
    nf = rng.uniform(0, 1, (V, C)).astype(np.float32)
    ef = rng.uniform(0, 1, (E + 1, C)).astype(np.float32)
    nf[0] = ef[0] = 0
    cut = np.floor(rng.uniform(5e7, 1e8, B))
    sgs = []
    for _ in range(3):
        node = rng.integers(1, V, (B, N))
        node[rng.uniform(size=node.shape) < 0.25] = 0
        eid = np.where(node > 0, rng.integers(1, E + 1, node.shape), 0)
        ts = np.where(node > 0, np.floor(cut[:, None] - rng.uniform(0, 5e7, node.shape)), 0.0)
        sgs.append((node, eid, ts))
    src, dst, fake = (rng.integers(1, V, B) for _ in range(3))
    return nf, ef, (src, dst, fake, cut), sgs


def bce(pos, neg):
    crit = F.binary_cross_entropy_with_logits
    return crit(pos, torch.ones_like(pos)) + crit(neg, torch.zeros_like(neg))


def device_steps(model, opt, roots, sgs, dev, steps, warmup):
    """Median ms of a training step on the device (HIP events), the inputs already there."""
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    src, dst, fake = (t(x, torch.long) for x in roots[:3])
    cut = t(roots[3], torch.float64)
    dsg = [([t(n, torch.long), None], [t(e, torch.long), None], [t(s, torch.float64), None]) for n, e, s in sgs]
    ms = []
    for k in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        opt.zero_grad()
        pos, neg = model.contrast(src, dst, fake, cut, None, *dsg, explain_weights=None, edge_attr=None)
        loss = bce(pos, neg)
        loss.backward()
        opt.step()
        b.record()
        b.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(loss.detach())


def cpu_embeddings(m, node_ids, cut, nid, eid, times):
    """GraphMixer.node_embeddings' torch formulation on the host (the module's own layers, dropout active)."""
    valid = nid != 0
    ef = m.e_feat_th[eid] * valid.unsqueeze(-1)
    tf = m.time_encoder.encode((cut.reshape(-1, 1) - times).float()) * valid.unsqueeze(-1)
    x = m.projection_layer(torch.cat([ef, tf], dim=-1))
    for mixer in m.mlp_mixers:
        x = mixer(x, None)
    x = (x * valid.unsqueeze(-1)).mean(dim=1)
    scores = torch.softmax(torch.where(valid, 1.0, -1e10).to(torch.float32), dim=1)
    agg = (m.n_feat_th[nid] * scores.unsqueeze(-1)).mean(dim=1)
    return m.output_layer(torch.cat([x, agg + m.n_feat_th[node_ids]], dim=1))


def cpu_steps(model, roots, sgs, steps, warmup, lr):
    m = copy.deepcopy(model).cpu().train()
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    B = len(roots[0])
    node = torch.from_numpy(np.concatenate(roots[:3])).long()
    cut = torch.from_numpy(np.tile(roots[3], 3))
    nid, eid, ts = (torch.from_numpy(np.concatenate([sg[k] for sg in sgs])) for k in range(3))
    nid, eid = nid.long(), eid.long()
    ms = []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        opt.zero_grad()
        emb = cpu_embeddings(m, node, cut, nid, eid, ts)
        s, d, n = emb[:B], emb[B:2 * B], emb[2 * B:]
        score = m.affinity(torch.cat([s, s], dim=0), torch.cat([d, n])).squeeze(dim=0)
        loss = bce(score[:B], score[B:])
        loss.backward()
        opt.step()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-steps", type=int, default=20)
    ap.add_argument("--batch-sizes", type=str, default="100,512")
    ap.add_argument("--dim", type=int, default=172)
    ap.add_argument("--n-degree", type=int, default=30)
    ap.add_argument("--n-layer", type=int, default=3)
    ap.add_argument("--drop-out", type=float, default=0.5)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    from tempme_amd import _lib as L
    from tempme_amd.graphmixer import GraphMixer
    dev = L.require_device(torch.device("cuda", 0))
    N, C = args.n_degree, args.dim
    results = []
    for B in (int(x) for x in args.batch_sizes.split(",")):
        nf, ef, roots, sgs = make_inputs(B, N, C)
        torch.manual_seed(0)
        base = GraphMixer(nf, ef, n_neighbors=N, device=dev, num_tokens=N, num_layers=args.n_layer,
                          dropout=args.drop_out).to(dev).train()
        out = {"B": B, "N": N, "C": C, "T": C, "L": args.n_layer, "dropout": args.drop_out, "steps": args.steps,
               "warmup": args.warmup, "cpu_threads": torch.get_num_threads()}
        for name, flag in (("hip", True), ("torch", False)):
            m = copy.deepcopy(base).train_on_hip(flag)
            m._gm_train_key = None
            opt = torch.optim.Adam(m.parameters(), lr=args.lr)
            if name == "hip" and args.profile:
                device_steps(m, opt, roots, sgs, dev, 2, args.warmup)
                L.profile_enable(True)
                device_steps(m, opt, roots, sgs, dev, args.steps, 0)
                prof = L.profile_read()
                L.profile_enable(False)
                out["hip_kernels_ms_per_step"] = {k: round(v[0] / args.steps, 4) for k, v in sorted(prof.items())}
                out["hip_launches_per_step"] = {k: v[1] / args.steps for k, v in sorted(prof.items())}
            ms, loss = device_steps(m, opt, roots, sgs, dev, args.steps, args.warmup)
            assert (m._gm_train_key is not None) == flag, "the wrong training path ran"
            out[f"{name}_ms"], out[f"{name}_last_loss"] = round(ms, 4), round(loss, 5)
        out["cpu_ms"] = round(cpu_steps(base, roots, sgs, args.cpu_steps, 2, args.lr), 3) if args.cpu_steps > 0 else None
        out["hip_over_torch"] = round(out["hip_ms"] / out["torch_ms"], 4)
        print(json.dumps(out), flush=True)
        results.append(out)
    print(json.dumps({"metric": "base_graphmixer_train_step_ms", "unit": "ms",
                      "shapes": {str(r["B"]): {k: r[k] for k in ("hip_ms", "torch_ms", "cpu_ms", "hip_over_torch")}
                                 for r in results}}), flush=True)


if __name__ == "__main__":
    main()
