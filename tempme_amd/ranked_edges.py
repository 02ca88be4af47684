"""Ranked explanation edges on the device: which past interactions explain a prediction, best first.

``retrieve_explanation``, ``ExplainPipeline.run`` and ``explain_sides`` return one weight per subgraph slot ([3B, N]
hop-1, [3B, N^2] hop-2).  The same edge id sits in several slots of a row and again in the other side's row of the
same pair, so slots are not edges.  ``ranked_edges`` gives every distinct edge of a prediction once -- its score the
maximum over its live slots, the slot it is first met in, how many slots carry it -- ordered by score descending and
edge id ascending, in one launch of ``tm_ranked_edges`` (csrc/ranked_edges.hip), one workgroup per prediction.  The
kernel only compares: there is no tolerance, and two launches give the same bits.  Nothing here waits for the device.
"""
from collections import namedtuple

import torch

from . import _lib as L
from .attn_layer import cat_rows, stack_sides
from .attn_op import as_dev

MAX_ENTRIES = 8192

RankedEdges = namedtuple("RankedEdges", "eid score node center ts hop mult count")
RankedEdges.__doc__ = """Device tensors of shape [..., k] (count: [...]), padded with 0 past min(count, k):
eid int32 edge ids; score float32 (the maximum over the edge's live slots); node int32 / center int64 the slot's
neighbour node and the node it hangs off (the root for a hop-1 slot, the hop-1 node j for hop-2 slot (j, .));
ts float64 the slot's time; hop int32 1 or 2; mult int32 live slots carrying the edge; count int32 the distinct
live edges of the prediction (may exceed k)."""


def _stack_explanation(explanation, dev):
    """[hop-1 [rows, N]] or [hop-1, hop-2 [rows, N^2]] float32 contiguous; the TGAT per-side six-list is stacked
    as fidelity.masked_contrast_tgat stacks it."""
    ex = list(explanation)
    if not ex or not all(torch.is_tensor(x) for x in ex):
        raise TypeError("ranked_edges: explanation is a list of torch tensors")
    for x in ex:
        if x.device != dev:
            raise RuntimeError(f"ranked_edges: explanation tensors on {x.device} and {dev}; the hot path has no CPU "
                               "fallback")
        if x.dtype != torch.float32:
            raise TypeError(f"ranked_edges: explanation is {x.dtype}; the scores are compared as float32 values")
    if len(ex) == 6:
        ex = [torch.cat([ex[2 * s + h] for s in range(3)], dim=0) for h in (0, 1)]
    if len(ex) not in (1, 2):
        raise ValueError(f"ranked_edges: explanation has {len(ex)} tensors, expected [hop-1], [hop-1, hop-2] or the "
                         "per-side six-list")
    return [x.contiguous() for x in ex]


def _stack_times(dev, subgraphs, hops):
    """The sides' time records stacked like stack_sides stacks them, but in the dtype they come in (one dtype for
    all hops): only the k gathered times of a prediction are widened to fp64, not the records."""
    out = []
    for h in range(hops):
        xs = [sg[2][h] for sg in subgraphs]
        if all(torch.is_tensor(x) and x.device == dev for x in xs):
            out.append(cat_rows(xs))
        else:
            out.append(torch.cat([as_dev(x, dev, torch.float64) for x in xs]))
    if len({x.dtype for x in out}) > 1:
        out = [x.double() for x in out]
    return out


def ranked_edges(explanation, subgraphs, roots, k, *, pairs=True, node_records=None, groups=None, check=False):
    """RankedEdges of every prediction, launched on the current stream of the explanation's device.

    explanation: [hop-1 [3B, N], hop-2 [3B, N^2]] float32, [hop-1] alone for a one-hop (GraphMixer) base, or the
    TGAT per-side six-list.  subgraphs, roots: the sides' (node, eid, time) records and root ids as
    ``attn_layer.stack_sides`` takes them.
    pairs=True: outputs [2, B, k]; prediction (0, i) merges rows src_i and tgt_i (the positive one), (1, i) merges
    src_i and bgd_i (the negative one).  pairs=False: one prediction per row, [3B, k].
    node_records: int32 [rows, ne] replacing the node records that decide which slots are live (for example one
    ratio's slice of fidelity._masked_nodes); the gathered node / center still come from ``subgraphs``.
    groups: int32 [G, 1 or 2] device tensor of row indices (-1: no row) instead of ``pairs``: outputs [G, k].
    check=True reads the kernel's error flag (a row index out of range) and raises; it waits for the device."""
    ex0 = explanation[0] if isinstance(explanation, (list, tuple)) and len(explanation) else explanation
    if not torch.is_tensor(ex0):
        raise TypeError("ranked_edges: explanation is a list of torch tensors")
    dev = L.require_device(ex0.device)
    imp = _stack_explanation(explanation, dev)
    hops = len(imp)
    if imp[0].dim() != 2:
        raise ValueError(f"ranked_edges: hop-1 explanation has shape {tuple(imp[0].shape)}, expected [rows, N]")
    rows, n = imp[0].shape
    if n < 1:
        raise ValueError("ranked_edges: N must be positive")
    shapes = [(rows, n), (rows, n * n)][:hops]
    ne = n + n * n if hops == 2 else n
    if hops == 2 and tuple(imp[1].shape) != shapes[1]:
        raise ValueError(f"ranked_edges: hop-2 explanation has shape {tuple(imp[1].shape)}, expected {shapes[1]}")
    n0, nodes, eids, _ = stack_sides(dev, roots, subgraphs, hops=hops, times=False)
    times = _stack_times(dev, subgraphs, hops)
    for name, xs in (("node", nodes), ("edge-id", eids), ("time", times)):
        for h in range(hops):
            if tuple(xs[h].shape) != shapes[h]:
                raise ValueError(f"ranked_edges: hop-{h + 1} {name} records have shape {tuple(xs[h].shape)}, the "
                                 f"explanation {shapes[h]}")
    if n0.shape[0] != rows:
        raise ValueError(f"ranked_edges: {n0.shape[0]} roots for {rows} explanation rows")
    nodes = [x.contiguous() for x in nodes]
    eids = [x.contiguous() for x in eids]
    live = nodes
    if node_records is not None:
        if not torch.is_tensor(node_records) or node_records.device != dev:
            raise RuntimeError("ranked_edges: node_records must be a tensor on the explanation's device; the hot "
                               "path has no CPU fallback")
        if tuple(node_records.shape) != (rows, ne):
            raise ValueError(f"ranked_edges: node_records has shape {tuple(node_records.shape)}, expected "
                             f"{(rows, ne)}")
        nr = node_records.to(torch.int32)
        live = [nr[:, :n].contiguous(), nr[:, n:].contiguous()][:hops]
    if groups is not None:
        if not torch.is_tensor(groups) or groups.device != dev:
            raise RuntimeError("ranked_edges: groups must be a tensor on the explanation's device; the hot path has "
                               "no CPU fallback")
        if groups.dim() != 2 or groups.shape[1] not in (1, 2):
            raise ValueError(f"ranked_edges: groups has shape {tuple(groups.shape)}, expected [G, 1] or [G, 2]")
        grp = groups.to(torch.int32).contiguous()
        out_shape = (grp.shape[0],)
    elif pairs:
        if rows % 3:
            raise ValueError(f"ranked_edges: pairs need the src, tgt and bgd sides, {rows} rows are not 3 B")
        B = rows // 3
        i = torch.arange(2 * B, dtype=torch.int32, device=dev)
        grp = torch.stack([i % max(B, 1), i + B], dim=1)                 # (src_i, tgt_i) for every i, then (src_i, bgd_i)
        out_shape = (2, B)
    else:
        grp = torch.arange(rows, dtype=torch.int32, device=dev).reshape(rows, 1)
        out_shape = (rows,)
    G, R = grp.shape
    k = int(k)
    if R * ne > MAX_ENTRIES:
        raise NotImplementedError(f"ranked_edges: {R} rows of {ne} slots are {R * ne} entries per prediction; the "
                                  f"kernel holds {MAX_ENTRIES}")
    if not 1 <= k <= R * ne:
        raise ValueError(f"ranked_edges: k = {k} is outside [1, {R * ne}], the entries of a prediction")

    i32 = dict(dtype=torch.int32, device=dev)
    eid = torch.empty((G, k), **i32)
    score = torch.empty((G, k), dtype=torch.float32, device=dev)
    slot, mult, count = torch.empty((G, k), **i32), torch.empty((G, k), **i32), torch.empty((G,), **i32)
    err = torch.zeros(1, **i32)
    hop2 = [imp[1], live[1], eids[1]] if hops == 2 else [None] * 3
    L.check(L.lib().tm_ranked_edges(L.ptr(imp[0]), L.ptr(hop2[0]), L.ptr(live[0]), L.ptr(hop2[1]),
                                    L.ptr(eids[0]), L.ptr(hop2[2]), rows, n, hops, L.ptr(grp), G, R, k,
                                    L.ptr(eid), L.ptr(score), L.ptr(slot), L.ptr(mult), L.ptr(count), L.ptr(err),
                                    L.stream_ptr(dev)), "ranked_edges")
    if check:
        L.raise_device_error(int(err.item()), "ranked_edges")

    # what the slot says about the edge: torch gathers from the stacked records (padded positions give 0)
    valid = slot >= 0
    sl = slot.clamp(min=0).long()
    p = torch.div(sl, ne, rounding_mode="floor")
    s = sl - p * ne
    base = grp.long().gather(1, p).clamp_(0, max(rows - 1, 0))
    center = n0[base]
    base = base * ne
    node_cat = (nodes[0] if hops == 1 else torch.cat(nodes, dim=1)).reshape(-1)
    ts_cat = (times[0] if hops == 1 else torch.cat(times, dim=1)).reshape(-1)
    flat = base + s
    node = torch.where(valid, node_cat[flat], 0)
    ts = torch.where(valid, ts_cat[flat].double(), 0.0)
    hop = valid.int()
    if hops == 2:
        second = s >= n
        j = torch.div(s - n, n, rounding_mode="floor").clamp_(min=0)
        center = torch.where(second, node_cat[base + j].long(), center)
        hop = hop + (second & valid).int()
    center = torch.where(valid, center, 0)
    sh = lambda x: x.view(*out_shape, k)                          # noqa: E731
    return RankedEdges(sh(eid), sh(score), sh(node), sh(center), sh(ts), sh(hop), sh(mult), count.view(*out_shape))


__all__ = ["ranked_edges", "RankedEdges", "MAX_ENTRIES"]
