"""Ranked motif instances on the device: which temporal motifs explain a prediction, best first.

``TempME.forward`` and ``ExplainPipeline.run`` score every sampled walk ([3, B, W], W = N M), one motif instance of
three events each.  Walks are sampled with replacement, so one instance -- one ordered triple of edge ids -- sits in
several of a row's walks and again in the other side's row of the same pair: the scores are not a list of motifs.
``ranked_motifs`` gives every distinct instance of a prediction once -- its score the maximum over its live walks, the
walk it is first met in, how many walks carry it, its category -- ordered by score descending and the triple
ascending, together with the prediction's profile over the 12 motif categories, in one launch of
``tm_ranked_motifs`` (csrc/ranked_motifs.hip), one workgroup per prediction.  The kernel only compares (the category
sums are fp64 additions in a fixed order): there is no tolerance, and two launches give the same bits.  Nothing here
waits for the device.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from .attn_op import as_dev

MAX_ENTRIES = 1024
N_CATS = 12

RankedMotifs = namedtuple("RankedMotifs", "eid score cat node ts walk mult count cat_n cat_max cat_sum")
RankedMotifs.__doc__ = """Device tensors; the per-instance fields are padded past min(count, k):
eid int32 [..., k, 3] the instance's edge ids (0); score float32 [..., k] the maximum over its live walks (0);
cat int32 [..., k] its category 0..11 (-1); node int32 [..., k, 6] / ts float64 [..., k, 3] the node and time records
of the walk it is first met in (0); walk int32 [..., k] that walk's entry index p W + w in the prediction (-1);
mult int32 [..., k] the live walks carrying it (0); count int32 [...] the distinct live instances (may exceed k);
cat_n int32 / cat_max float32 / cat_sum float64 [..., 12]: per category the prediction's live walks, their maximum
score and the sum of their non-NaN scores."""

_DTYPES = (torch.int32, torch.int32, torch.float32, torch.int32)
_TAILS = ((6,), (3,), (3,), ())


def _stage_walks(walks, dev):
    """(node6 [rows, W, 6] int32, eid3 [rows, W, 3] int32, ts3 [rows, W, 3] float32, cat [rows, W] int32) on ``dev``
    from the three sides' (node6, eid3, ts3, cat[, marginal]) tuples -- device tensors, or the reference's host
    arrays of one shape, staged in the dtypes TempME._enhance_stage stages them in -- or from one 4-tuple of
    side-major [3, B, W, ...] tensors (EventBuffers), which stays a view."""
    walks = list(walks)
    stacked = len(walks) == 4 and all(torch.is_tensor(x) for x in walks) and walks[1].dim() == 4
    if not stacked and (len(walks) != 3 or any(not isinstance(s, (list, tuple)) or len(s) < 4 for s in walks)):
        raise TypeError("ranked_motifs: walks is the three sides' (node6, eid3, ts3, cat) tuples, or one tuple of "
                        "[3, B, W, ...] tensors")
    shape = tuple(walks[1].shape[1:3]) if stacked else tuple(np.shape(walks[0][1])[:2])
    if len(shape) != 2:
        raise ValueError("ranked_motifs: the walks' edge ids have shape [B, W, 3]")
    B, W = shape
    out = []
    for i, (dt, tail) in enumerate(zip(_DTYPES, _TAILS)):
        xs = [walks[i]] if stacked else [s[i] for s in walks]
        if any(torch.is_tensor(x) and x.device != dev for x in xs):
            raise RuntimeError(f"ranked_motifs: walks on {[x.device for x in xs if torch.is_tensor(x)][0]} and imp on "
                               f"{dev}; the hot path has no CPU fallback")
        n_el = (3 if stacked else 1) * B * W * int(np.prod(tail, dtype=np.int64))
        if any(int(np.prod(np.shape(x), dtype=np.int64)) != n_el for x in xs):
            raise ValueError(f"ranked_motifs: a walk record of shape {[tuple(np.shape(x)) for x in xs]} does not "
                             f"hold [{B}, {W}{''.join(', %d' % t for t in tail)}] per side")
        xs = [as_dev(x, dev, dt).reshape((-1, W) + tail) for x in xs]
        out.append((xs[0] if stacked else torch.cat(xs, dim=0)).contiguous())
    return out


def ranked_motifs(imp, walks, k, *, pairs=True, groups=None, check=False):
    """RankedMotifs of every prediction, launched on the current stream of ``imp``'s device.

    imp: [3, B, W] or [3B, W] float32 walk scores (TempME.forward's, the three sides stacked).  walks: the three
    sides' (node6, eid3, ts3, cat) device tensors as TempME.forward takes them (the reference's five-tuples of host
    arrays are staged), or one tuple of side-major [3, B, W, ...] tensors.
    pairs=True: outputs [2, B, ...]; prediction (0, i) merges rows src_i and tgt_i (the positive one), (1, i) merges
    src_i and bgd_i (the negative one).  pairs=False: one prediction per row, [3B, ...].
    groups: int32 [G, 1 or 2] device tensor of row indices (-1: no row) instead of ``pairs``: outputs [G, ...].
    check=True reads the kernel's error flag (a row index or a category out of range) and raises; it waits for the
    device."""
    if not torch.is_tensor(imp):
        raise TypeError("ranked_motifs: imp is a torch tensor")
    dev = L.require_device(imp.device)
    if imp.dtype != torch.float32:
        raise TypeError(f"ranked_motifs: imp is {imp.dtype}; the scores are compared as float32 values")
    if imp.dim() not in (2, 3) or (imp.dim() == 3 and imp.shape[0] != 3):
        raise ValueError(f"ranked_motifs: imp has shape {tuple(imp.shape)}, expected [3, B, W] or [3B, W]")
    W = int(imp.shape[-1])
    if W < 1:
        raise ValueError("ranked_motifs: W must be positive")
    imp = imp.reshape(-1, W).contiguous()
    rows = imp.shape[0]
    node6, eid3, ts3, cat = _stage_walks(walks, dev)
    if tuple(eid3.shape) != (rows, W, 3):
        raise ValueError(f"ranked_motifs: the walks hold {tuple(eid3.shape[:2])} rows and walks, imp {(rows, W)}")
    if groups is not None:
        if not torch.is_tensor(groups) or groups.device != dev:
            raise RuntimeError("ranked_motifs: groups must be a tensor on imp's device; the hot path has no CPU "
                               "fallback")
        if groups.dim() != 2 or groups.shape[1] not in (1, 2):
            raise ValueError(f"ranked_motifs: groups has shape {tuple(groups.shape)}, expected [G, 1] or [G, 2]")
        grp = groups.to(torch.int32).contiguous()
        out_shape = (grp.shape[0],)
    elif pairs:
        if rows % 3:
            raise ValueError(f"ranked_motifs: pairs need the src, tgt and bgd sides, {rows} rows are not 3 B")
        B = rows // 3
        i = torch.arange(2 * B, dtype=torch.int32, device=dev)
        grp = torch.stack([i % max(B, 1), i + B], dim=1)              # (src_i, tgt_i) for every i, then (src_i, bgd_i)
        out_shape = (2, B)
    else:
        grp = torch.arange(rows, dtype=torch.int32, device=dev).reshape(rows, 1)
        out_shape = (rows,)
    G, R = grp.shape
    k = int(k)
    if R * W > MAX_ENTRIES:
        raise NotImplementedError(f"ranked_motifs: {R} rows of {W} walks are {R * W} entries per prediction; the "
                                  f"kernel holds {MAX_ENTRIES}")
    if not 1 <= k <= R * W:
        raise ValueError(f"ranked_motifs: k = {k} is outside [1, {R * W}], the entries of a prediction")

    i32 = dict(dtype=torch.int32, device=dev)
    eid = torch.empty((G, k, 3), **i32)
    score = torch.empty((G, k), dtype=torch.float32, device=dev)
    walk, mult, mcat, count = (torch.empty((G, k), **i32), torch.empty((G, k), **i32), torch.empty((G, k), **i32),
                               torch.empty((G,), **i32))
    cat_n = torch.empty((G, N_CATS), **i32)
    cat_max = torch.empty((G, N_CATS), dtype=torch.float32, device=dev)
    cat_sum = torch.empty((G, N_CATS), dtype=torch.float64, device=dev)
    err = torch.zeros(1, **i32)
    L.check(L.lib().tm_ranked_motifs(L.ptr(eid3), L.ptr(cat), L.ptr(imp), rows, W, L.ptr(grp), G, R, k, L.ptr(eid),
                                     L.ptr(score), L.ptr(walk), L.ptr(mult), L.ptr(mcat), L.ptr(count), L.ptr(cat_n),
                                     L.ptr(cat_max), L.ptr(cat_sum), L.ptr(err), L.stream_ptr(dev)), "ranked_motifs")
    if check:
        L.raise_device_error(int(err.item()), "ranked_motifs")

    # what the walk says about the instance: torch gathers from the walk records (padded positions give 0)
    valid = walk >= 0
    wl = walk.clamp(min=0).long()
    p = torch.div(wl, W, rounding_mode="floor")
    flat = grp.long().gather(1, p).clamp_(0, max(rows - 1, 0)) * W + (wl - p * W)
    node = torch.where(valid.unsqueeze(-1), node6.reshape(-1, 6)[flat], 0)
    ts = torch.where(valid.unsqueeze(-1), ts3.reshape(-1, 3)[flat].double(), 0.0)
    sh = lambda x, *t: x.view(*out_shape, *t)                          # noqa: E731
    return RankedMotifs(sh(eid, k, 3), sh(score, k), sh(mcat, k), sh(node, k, 6), sh(ts, k, 3), sh(walk, k),
                        sh(mult, k), count.view(*out_shape), sh(cat_n, N_CATS), sh(cat_max, N_CATS),
                        sh(cat_sum, N_CATS))


__all__ = ["ranked_motifs", "RankedMotifs", "MAX_ENTRIES"]
