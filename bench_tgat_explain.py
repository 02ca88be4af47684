"""Explainer training-step and evaluation-batch time over a TGAT base (BASELINE.json configs[2]: full Enron + TGAT).

    python bench_tgat_explain.py [--steps 20 --warmup 5 --legs dropin,train_step,graphed,eval --count-kernels]

bench_train.py's workload shape (full-Enron-shaped synthetic graph, V = 184, E = 125,235, B = 100 target events,
N = 20, the pack sampled on the device before timing) with a TGAT base (2 layers, 2 heads, random init) and a
random-init TempME in training mode (dropout, Beta rsample), torch.optim.Adam(lr=1e-3, capturable=True).  One step
= temp_exp_main.py:593-632.  Three formulations, each on its own explainer from the same seed:

  dropin      the eager per-side composition: contrast(test=True, if_explain=False) under no_grad, three
              TempME.forward calls, three retrieve_edge_imp_node calls, contrast(exp_weights=[[s, t], [s, b]]),
              three kl_loss calls.  Written with calls that predate the drivers' TGAT support, so the same leg
              runs on an older tree (--legs dropin).
  train_step  tempme_amd.train.train_step, eager (one batch per step)
  graphed     tempme_amd.train.GraphedTrainStep (the step captured once as a HIP graph, replayed per batch)

and, with the leg ``eval``, tempme_amd.evaluate.eval_batch (if_bern off, threshold_test on) with the host metrics
and with device_metrics.  The base's last bias is shifted by minus the median original logit first, so y_ori has both
classes (a one-class batch has no AUC).  Training legs are timed with HIP events around each step, the eval legs with
the host clock around a synchronised call (the host path reads scalars back); each figure is the median over
--steps calls after --warmup.  Prints one JSON line.
"""
import argparse
import json
import time
from types import SimpleNamespace

import numpy as np
import torch


def median_ms(step, steps, warmup, host_clock=False):
    ms = []
    for k in range(warmup + steps):
        if host_clock:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(k)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(k)
            b.record()
            b.synchronize()
            dt = a.elapsed_time(b)
        if k >= warmup:
            ms.append(dt)
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4), round(float(np.max(ms)), 4)


def count_kernels(step):
    """Device kernels of one call, by torch.profiler (None if the profiler gives no device events)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step(0)
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA)
    return n or None


def dropin_step(ex, base, opt, b, beta=0.5, prior_p=0.3, if_bern=True):
    """The eager per-side composition of one training step."""
    criterion = torch.nn.BCEWithLogitsLoss()
    a = (b.src, b.dst, b.fake, b.ts, b.e_idx, *b.subgraphs)
    with torch.no_grad():
        po, no = base.contrast(*a, test=True, if_explain=False)
        y_ori = torch.where(torch.cat([po, no], dim=0).sigmoid() > 0.5, 1., 0.).view(-1, 1)
    opt.zero_grad()
    gl = [ex(w, b.ts, e) for w, e in zip(b.walks, b.edges)]
    imps = [tuple(ex.retrieve_edge_imp_node(sg, g, w, training=if_bern)) for sg, g, w in zip(b.subgraphs, gl, b.walks)]
    pos, neg = base.contrast(*a, test=True, if_explain=True, exp_weights=[[imps[0], imps[1]], [imps[0], imps[2]]])
    loss = criterion(torch.cat([pos, neg], dim=0), y_ori) + beta * sum(
        ex.kl_loss(g, w, target=prior_p) for g, w in zip(gl, b.walks))
    loss.backward()
    opt.step()
    return loss.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=100)
    ap.add_argument("--n-degree", type=int, default=20)
    ap.add_argument("--n-head", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--legs", type=str, default="dropin,train_step,graphed,eval")
    ap.add_argument("--overlap-prepare", action="store_true",
                    help="graphed leg: the base's original contrast as a second graph branch")
    ap.add_argument("--count-kernels", action="store_true")
    args = ap.parse_args()
    if args.gpus != 1:
        raise SystemExit("bench_tgat_explain.py measures one GPU")
    legs = [x for x in args.legs.split(",") if x]

    import tempme_amd as tm
    from tempme_amd import _lib as L
    from tempme_amd.preprocess import sample_events
    from tempme_amd.tgat import TGAT
    from tempme_amd.train import batch_from_pack
    from tempme_amd.workload import enron_like, split

    dev = L.require_device(torch.device("cuda", 0))
    N, M, B = args.n_degree, 3, args.batch_size
    g = enron_like(n_nodes=184, n_edges=125235, alpha=1.2, seed=args.seed)             # full Enron shape
    (src, dst, ts, eidx), rows, pool = split(g, mode="train")
    finder = tm.NeighborFinder.from_edges(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows],
                                          g["n_nodes"], device=dev, seed=args.seed, split=tm.SPLIT_TRAIN)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    ev = (to(src, np.int32), to(dst, np.int32), to(ts, np.float64), to(eidx, np.int32))
    buf = sample_events(finder.graph, args.seed, tm.SPLIT_TRAIN, N, M, *ev,
                        torch.arange(len(src), dtype=torch.int32, device=dev), to(pool, np.int32))
    torch.manual_seed(args.seed)
    base = TGAT(g["n_feat"], g["e_feat"], N, num_layers=2, n_head=args.n_head).to(dev).eval()

    n_calls = args.warmup + args.steps
    perm = torch.randperm(len(src) - 1, generator=torch.Generator().manual_seed(args.seed)).to(dev)
    rows = [perm[k * B:(k + 1) * B] for k in range(n_calls + 1)]
    with torch.no_grad():                    # both classes in y_ori: centre the original logits
        b0 = batch_from_pack(buf, *ev, rows[0])
        po, no = base.contrast(b0.src, b0.dst, b0.fake, b0.ts, b0.e_idx, *b0.subgraphs, test=True, if_explain=False)
        base.affinity_score.fc2.bias -= torch.cat([po, no]).median()

    def explainer():
        torch.manual_seed(args.seed + 1)
        ex = tm.TempME(base, "tgat", "enron", out_dim=40, hid_dim=64, device=dev,
                       null_model={k: 1.0 / 12 for k in range(1, 13)}).to(dev)
        return ex, torch.optim.Adam(ex.parameters(), lr=1e-3, capturable=True)

    out = {"metric": "explainer training step over a TGAT base (full-Enron-shaped graph)", "unit": "ms",
           "B": B, "N": N, "n_head": args.n_head, "steps": args.steps, "warmup": args.warmup,
           "train_events": int(len(src)), "figures": "median (min, max) over the timed calls"}
    counts = {}

    def leg(name, step, host_clock=False):
        out[name + "_ms"], lo, hi = median_ms(step, args.steps, args.warmup, host_clock)
        out[name + "_min_max_ms"] = [lo, hi]
        if args.count_kernels:
            try:
                counts[name] = count_kernels(step)
            except Exception as exc:      # the profiler is optional equipment
                counts[name] = repr(exc)

    if "dropin" in legs:
        ex, opt = explainer()
        ex.train()
        last = {}

        def step(k):
            last["loss"] = dropin_step(ex, base, opt, batch_from_pack(buf, *ev, rows[k]))
        leg("dropin", step)
        out["dropin_last_loss"] = round(float(last["loss"]), 5)
    if "train_step" in legs:
        from tempme_amd.train import train_step
        ex, opt = explainer()
        ex.train()
        last = {}

        def step(k):
            last["loss"] = train_step(ex, base, opt, batch_from_pack(buf, *ev, rows[k]))["loss"]
        leg("train_step", step)
        out["train_step_last_loss"] = round(float(last["loss"]), 5)
        assert ex._hip_ok() and base._pack_cache is not None, "the HIP path did not run"
    if "graphed" in legs:
        from tempme_amd.train import GraphedTrainStep
        ex, opt = explainer()
        ex.train()
        graphed = GraphedTrainStep(ex, base, opt, buf, *ev, rows[:2], overlap_prepare=args.overlap_prepare)
        last = {}

        def step(k):
            last["loss"] = graphed(rows[k])["loss"]
        leg("graphed", step)
        out["graphed_last_loss"] = round(float(last["loss"]), 5)
        out["graphed_overlap_prepare"] = bool(args.overlap_prepare)
    if "eval" in legs:
        from tempme_amd.evaluate import eval_batch
        ex, _ = explainer()
        ex.eval()
        eargs = SimpleNamespace(test_bs=B, if_bern=False, beta=0.5, prior_p=0.3, test_threshold=True, base_type="tgat",
                                n_degree=N, ratios=[0.01, 0.05, 0.1, 0.2, 0.3])
        batches = [batch_from_pack(buf, *ev, r) for r in rows[:n_calls]]
        for name, dm in (("eval_batch_host_metrics", False), ("eval_batch_device_metrics", True)):
            leg(name, lambda k, dm=dm: eval_batch(eargs, base, ex, batches[k], device_metrics=dm), host_clock=True)
    torch.cuda.synchronize()
    base.check_errors()
    if counts:
        out["device_kernels_per_call"] = counts
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
