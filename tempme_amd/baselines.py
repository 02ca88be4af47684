"""Baseline explainers on the device: what the base model gives for free, in the form the fidelity harness takes.

The TempME paper compares the trained explainer against the base model's own attention weights (ATTN), the gradient
of the prediction with respect to the edge weights (Grad-CAM / saliency) and random scores.  Every function here
returns an explanation as ``fidelity.threshold_test``, ``fidelity.kept_edges`` and ``ranked_edges`` take it:

    TGN, TGAT     [e1 [3B, N], e2 [3B, N^2]]      (TGAT's per-side six-list: ``train.split_stacked_weights(flat=True)``)
    GraphMixer    [e1 [3B, N]]

fp32 on the device, non-negative, rows in the order src, tgt, bgd, and every slot whose node record is 0 exactly 0
(as ``retrieve_explanation`` masks padded slots).

``batch``: a ``train.Batch`` (``src``, ``dst``, ``fake``, ``ts``, ``e_idx`` and the three sides' ``subgraphs``).

  * ``attention_explanation``: the mean over the heads of ``base_model.attention_weights`` (tm_*_attn_probs on the two
    descriptors the frozen embedding pass builds); hop-1 from the top layer, hop-2 from the first.
  * ``saliency_explanation``: |dL/dw| at w = 1 of L = pos.sum() + neg.sum() of one explained contrast, through the
    kernels the explainer trains through (attn_bwd_kernel, gm_bwd_kernel); the base model's parameters get no .grad.
  * ``random_explanation``: uniform scores from a seeded generator.
  * ``threshold_rows``: ``fidelity.threshold_test``'s five figures per method against one original contrast, to put
    beside the ratio figures ``evaluate.eval_batch`` gives for the trained explainer.
"""
import torch

from .attn_op import as_dev

METHODS = ("attention", "saliency", "random")


def _hops(args):
    if args.base_type not in ("tgn", "tgat", "graphmixer"):
        raise NotImplementedError(f"baselines for base_type {args.base_type!r}: tgn, tgat and graphmixer are built")
    return 1 if args.base_type == "graphmixer" else 2


def node_records(batch, dev, hops=2):
    """[hop-1 [3B, N], hop-2 [3B, N^2]][:hops] int32 node records of the sides src, tgt, bgd on ``dev``."""
    return [torch.cat([as_dev(sg[0][h], dev, torch.int32) for sg in batch.subgraphs], dim=0) for h in range(hops)]


def _masked(scores, nodes):
    """The scores with every padded slot (node record 0) exactly 0, as the explainer's own output."""
    return [s.reshape(n.shape) * (n != 0).to(s.dtype) for s, n in zip(scores, nodes)]


def _sides(batch):
    return (batch.src, batch.dst, batch.fake, batch.ts) + tuple(batch.subgraphs)


def attention_explanation(base_model, batch, prepared=None):
    """[e1 [3B, N], e2 [3B, N^2]]: the base model's attention probabilities averaged over the heads -- the roots over
    their hop-1 neighbours (top layer) and the hop-1 nodes over their hop-2 neighbours (first layer).  ``prepared``:
    the base's ``prepare_contrast`` output for this batch."""
    if not hasattr(base_model, "attention_weights"):
        raise NotImplementedError(f"{type(base_model).__name__} has no attention to read: use the 'saliency' "
                                  "baseline (saliency_explanation) for this base")
    m1, m2 = base_model.attention_weights(*_sides(batch), prepared=prepared, head_mean=True)
    return _masked([m1, m2], node_records(batch, m1.device, 2))


def saliency_explanation(args, base_model, batch, prepared=None):
    """|dL/dw| at all-ones explanation weights w, L = pos.sum() + neg.sum() of one explained contrast (one forward,
    one backward through the base's explanation-weight gradient).  The base model runs in eval mode and is put back
    as it was; its parameters get no .grad (the gradient is asked for the weights alone)."""
    from .train import explained_contrast
    from .tgat import TGAT
    hops = _hops(args)
    dev = base_model._dev()
    nodes = node_records(batch, dev, hops)
    w = [torch.ones(n.shape, dtype=torch.float32, device=dev, requires_grad=True) for n in nodes]
    kw = {} if prepared is None else {"prepared": prepared}
    was_training = base_model.training
    base_model.eval()
    try:
        with torch.enable_grad():
            pos, neg = explained_contrast(base_model, batch, w, kw, isinstance(base_model, TGAT))
            grads = torch.autograd.grad(pos.sum() + neg.sum(), w)
    finally:
        base_model.train(was_training)
    return _masked([g.detach().abs() for g in grads], nodes)


def random_explanation(batch, seed, hops=2, device=None):
    """Uniform [0, 1) scores from a generator on ``device`` seeded with ``seed`` (default device: where the batch's
    events live, else the CPU); the same seed gives the same scores."""
    if device is None:
        device = batch.src.device if torch.is_tensor(batch.src) else torch.device("cpu")
    device = torch.device(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    nodes = node_records(batch, device, hops)
    return _masked([torch.rand(n.shape, generator=gen, dtype=torch.float32, device=device) for n in nodes], nodes)


def baseline_explanation(method, args, base_model, batch, prepared=None):
    """The explanation of ``method`` ("attention", "saliency" or "random") for ``args.base_type``; "random" reads
    ``args.seed`` (default 0)."""
    if method not in METHODS:
        raise ValueError(f"baseline_explanation: unknown method {method!r}; the baselines are {', '.join(METHODS)}")
    hops = _hops(args)
    if method == "attention":
        return attention_explanation(base_model, batch, prepared)
    if method == "saliency":
        return saliency_explanation(args, base_model, batch, prepared)
    return random_explanation(batch, getattr(args, "seed", 0), hops, base_model._dev())


def threshold_rows(args, base_model, batch, methods=METHODS, device_metrics=False):
    """{method: threshold_test's five figures (evaluate.RATIO_FIGURES)} of the baselines ``methods`` on one batch:
    the original contrast (pos_out_ori, neg_out_ori, y_ori) is computed once, as ``evaluate.eval_batch`` computes
    it, and every method's explanation goes through ``fidelity.threshold_test`` (``device_metrics``: each row a
    float64 device tensor [5])."""
    from . import fidelity
    from .tgat import TGAT
    from .train import prepare_step, split_stacked_weights
    for m in methods:
        if m not in METHODS:
            raise ValueError(f"threshold_rows: unknown method {m!r}; the baselines are {', '.join(METHODS)}")
    kw, pos_out_ori, neg_out_ori, y_ori = prepare_step(base_model, batch)
    rows = {}
    for m in methods:
        expl = baseline_explanation(m, args, base_model, batch, kw.get("prepared"))
        if isinstance(base_model, TGAT):
            expl = split_stacked_weights(*expl, flat=True)
        rows[m] = fidelity.threshold_test(args, expl, base_model, batch.src, batch.dst, batch.fake, batch.ts,
                                          batch.e_idx, pos_out_ori, neg_out_ori, y_ori, *batch.subgraphs,
                                          device_metrics=device_metrics)
    return rows


__all__ = ["METHODS", "attention_explanation", "saliency_explanation", "random_explanation", "baseline_explanation",
           "threshold_rows", "node_records"]
