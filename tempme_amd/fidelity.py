"""Fidelity evaluation of an explanation on the base model: ``threshold_test``
(temp_exp_main.py:153-272, tgn, graphmixer and tgat branches) on the HIP device.

For each sparsity ratio the reference keeps the top ``ceil(ratio * (N + N^2))`` subgraph entries by
explanation score, zeroes the node ids of the rest (torch.topk(largest=False) + np.put_along_axis),
re-runs ``contrast`` without explanation weights and scores the result against the original
predictions (AP, AUC, accuracy, fidelity of probabilities and logits), then averages over ratios.

Here the masks of all ratios come from one launch of ``mask_least_kernel`` (tm_mask_least_important,
which reproduces the CPU top-k's tie order), and all ratios go through ONE batched contrast
(``TGN.node_embeddings(..., n_segments=len(ratios))``) instead of one call per ratio.  AP and AUC
are computed with scikit-learn on the host, as the reference does, from the 2B predictions per ratio; with
``device_metrics=True`` all ratios' score vectors go through one ``metrics.rank_metrics`` launch instead and the
five figures come back as a device tensor, with no copy to the host.
"""
import math

import numpy as np
import torch
from sklearn.metrics import average_precision_score, roc_auc_score

from . import _lib as L
from .attn_layer import stack_sides
from .attn_op import as_dev


def _masked_nodes(explanation, subgraphs, N, ratios, dev, hops=2):
    """[G, 3B, ne] int32 node records with the least important entries of each ratio set to 0;
    hops=2: [hop-1 | hop-2] records, ne = N + N^2 (tgn / tgat branches); hops=1: hop-1 records,
    ne = N (graphmixer branch)."""
    ne = N + N * N if hops == 2 else N
    imp = torch.cat(list(explanation[:hops]), dim=1).to(dev, torch.float32).contiguous()
    nodes = torch.cat([torch.cat([as_dev(sg[0][h], dev, torch.int32) for h in range(hops)], dim=1)
                       for sg in subgraphs], dim=0).contiguous()
    rows = nodes.shape[0]
    if imp.shape != (rows, ne):
        raise AssertionError(f"explanation rows {tuple(imp.shape)} do not match the subgraphs ({rows}, {ne})")
    ks = [ne - min(max(math.ceil(r * ne), 1), ne) for r in ratios]      # temp_exp_main.py:158-168
    k_dev = torch.tensor(ks, dtype=torch.int32, device=dev)
    out = torch.empty((len(ratios), rows, ne), dtype=torch.int32, device=dev)
    L.check(L.lib().tm_mask_least_important(L.ptr(imp), rows, ne, L.ptr(k_dev), len(ratios), L.ptr(nodes),
                                            L.ptr(out), L.stream_ptr(dev)), "threshold_test masks")
    return out


def _pair_scores(base_model, emb, G, B):
    """(pos [G, B], neg [G, B]) from the [G 3B, d] embeddings of every ratio's src, tgt, bgd sides."""
    emb = emb.view(G, 3, B, -1)
    s, d, n = emb[:, 0], emb[:, 1], emb[:, 2]
    x1 = torch.cat([s, s], dim=1).reshape(G * 2 * B, -1)
    x2 = torch.cat([d, n], dim=1).reshape(G * 2 * B, -1)
    score = base_model.affinity(x1, x2).view(G, 2 * B)
    return score[:, :B], score[:, B:]


def _contrast_nodes(base_model, masked, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, sgs, N, side_segments=False):
    """(pos [G, B], neg [G, B]) logits of contrast without weights on G masked copies of the batch, all in one
    batch: ``masked`` [G, 3B, N + N^2] int32 node records ([hop-1 | hop-2]); edge ids and times are the batch's own.
    ``side_segments`` (tgat): every (copy, side) is one forward_msg call of B rows, a segment of its own; else (tgn)
    a copy's three sides are one segment."""
    dev = base_model._dev()
    B, G = len(src_l_cut), masked.shape[0]
    roots, _, eids, times = stack_sides(dev, (src_l_cut, dst_l_cut, dst_l_fake), sgs, nodes=False)
    n1 = masked[:, :, :N].reshape(G * 3 * B, N)
    n2 = masked[:, :, N:].reshape(G * 3 * B, N * N)
    emb = base_model.node_embeddings([roots.repeat(G), n1, n2], [x.repeat(G, 1) for x in eids],
                                     [x.repeat(G, 1) for x in times], ts_l_cut,
                                     n_segments=3 * G if side_segments else G)
    return _pair_scores(base_model, emb, G, B)


def _contrast_nodes_graphmixer(base_model, masked, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, sgs, N):
    """_contrast_nodes for the one-hop GraphMixer base: ``masked`` [G, 3B, N] hop-1 node records."""
    dev = base_model._dev()
    B, G = len(src_l_cut), masked.shape[0]
    masked = masked.reshape(G * 3 * B, N)
    roots, _, (eid,), (t,) = stack_sides(dev, (src_l_cut, dst_l_cut, dst_l_fake), sgs, nodes=False, hops=1,
                                         idx_dtype=torch.long)
    cut = as_dev(ts_l_cut, dev, torch.float64).reshape(-1).repeat(3 * G)
    emb = base_model.node_embeddings(roots.repeat(G), cut, masked, eid.repeat(G, 1), t.repeat(G, 1))
    return _pair_scores(base_model, emb, G, B)


def masked_contrast(base_model, explanation, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, subgraph_src, subgraph_tgt,
                    subgraph_bgd, n_degree, ratios, side_segments=False):
    """(pos [G, B], neg [G, B]) logits of contrast on the masked subgraph of every ratio: [hop-1 | hop-2] records
    masked, then contrast without weights, all ratios in one batch.  ``explanation``: (hop-1 [3B, N], hop-2
    [3B, N^2]).  ``side_segments`` (tgat): every (ratio, side) is one forward_msg call of B rows, a segment of its
    own; else (tgn) a ratio's three sides are one segment."""
    sgs = (subgraph_src, subgraph_tgt, subgraph_bgd)
    masked = _masked_nodes(explanation, sgs, n_degree, ratios, base_model._dev())     # [G, 3B, ne]
    return _contrast_nodes(base_model, masked, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, sgs, n_degree,
                           side_segments)


def masked_contrast_graphmixer(base_model, explanation, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, subgraph_src,
                               subgraph_tgt, subgraph_bgd, n_degree, ratios):
    """graphmixer branch (temp_exp_main.py:186-206): hop-1 records masked, all ratios in one batch."""
    sgs = (subgraph_src, subgraph_tgt, subgraph_bgd)
    masked = _masked_nodes(explanation, sgs, n_degree, ratios, base_model._dev(), hops=1)
    return _contrast_nodes_graphmixer(base_model, masked, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, sgs, n_degree)


def masked_contrast_tgat(base_model, explanation, *batch):
    """tgat branch (temp_exp_main.py:216-250): masked_contrast for the per-side 6-list explanation
    [src0, src1, tgt0, tgt1, bgd0, bgd1], every (ratio, side) a segment."""
    dev = base_model._dev()
    stacked = [torch.cat([explanation[2 * s + h].to(dev) for s in range(3)], dim=0) for h in (0, 1)]
    return masked_contrast(base_model, stacked, *batch, side_segments=True)


def kept_edges(args, explanation, subgraph_src, subgraph_tgt, subgraph_bgd, roots, ratio, k, pairs=True):
    """The ranked edges (ranked_edges.RankedEdges) of exactly the subgraph ``threshold_test`` scores at sparsity
    ``ratio``: the entries ``_masked_nodes`` keeps for that ratio are the live ones, no other selection rule.
    ``roots``: (src_l_cut, dst_l_cut, dst_l_fake); ``explanation`` as threshold_test takes it for args.base_type."""
    from .ranked_edges import _stack_explanation, ranked_edges
    if args.base_type not in ("tgn", "graphmixer", "tgat"):
        raise NotImplementedError(f"kept_edges for base_type {args.base_type!r}: tgn, graphmixer and tgat are built")
    ex0 = explanation[0]
    if not torch.is_tensor(ex0):
        raise TypeError("kept_edges: explanation is a list of torch tensors")
    dev = L.require_device(ex0.device)
    hops = 1 if args.base_type == "graphmixer" else 2
    imp = _stack_explanation(explanation, dev)[:hops]
    sgs = (subgraph_src, subgraph_tgt, subgraph_bgd)
    masked = _masked_nodes(imp, sgs, args.n_degree, [ratio], dev, hops=hops)[0]
    return ranked_edges(imp, sgs, roots, k, pairs=pairs, node_records=masked)


def threshold_test(args, explanation, base_model, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, e_l_cut,
                   pos_out_ori, neg_out_ori, y_ori, subgraph_src, subgraph_tgt, subgraph_bgd, device_metrics=False):
    """temp_exp_main.py:153-272 -> (aps_AUC, auc_AUC, acc_AUC, fid_prob_AUC, fid_logit_AUC): five floats, or with
    ``device_metrics`` a float64 device tensor [5] (AP and AUC of every ratio from one rank_metrics launch against
    the shared y_ori, the means over ratios taken on the device; nothing waits for the device)."""
    fns = {"tgn": masked_contrast, "graphmixer": masked_contrast_graphmixer, "tgat": masked_contrast_tgat}
    if args.base_type not in fns:
        raise NotImplementedError(f"threshold_test for base_type {args.base_type!r}: tgn, graphmixer and tgat "
                                  "are built")
    with torch.no_grad():
        pos, neg = fns[args.base_type](base_model, explanation, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut,
                                       subgraph_src, subgraph_tgt, subgraph_bgd, args.n_degree, list(args.ratios))
        fid_prob, fid_logit, y_pred, y, acc = _fidelity_terms(pos, neg, pos_out_ori, neg_out_ori, y_ori)
        if device_metrics:
            from .metrics import rank_metrics
            m = rank_metrics(y.reshape(-1), y_pred).mean(0)
            return torch.cat([m, torch.stack([acc.mean(), fid_prob.mean(), fid_logit.mean()]).double()])
        y_pred_h, y_h = y_pred.cpu().numpy(), y_ori.reshape(-1).cpu().numpy()
    aps = [average_precision_score(y_h, p) for p in y_pred_h]
    auc = [roc_auc_score(y_h, p) for p in y_pred_h]
    return (float(np.mean(aps)), float(np.mean(auc)), float(acc.mean().item()), float(fid_prob.mean().item()),
            float(fid_logit.mean().item()))


def _fidelity_terms(pos, neg, pos_out_ori, neg_out_ori, y_ori):
    """The per-copy terms of threshold_test's figures from the logits (pos, neg) [G, B] of G masked copies:
    (fid_prob [G], fid_logit [G], y_pred [G, 2B], y [1, 2B], acc [G]), float32 on the logits' device."""
    po = pos_out_ori.reshape(1, -1).to(pos.device, torch.float32)
    no = neg_out_ori.reshape(1, -1).to(pos.device, torch.float32)
    fid_prob = torch.cat([pos.sigmoid() - po.sigmoid(), no.sigmoid() - neg.sigmoid()], dim=1).mean(1)
    fid_logit = torch.cat([pos - po, no - neg], dim=1).mean(1)
    y_pred = torch.cat([pos, neg], dim=1).sigmoid()
    pred_label = torch.where(y_pred > 0.5, 1., 0.)
    y = y_ori.reshape(1, -1).to(pos.device, torch.float32)
    acc = (pred_label == y).float().mean(1)
    return fid_prob, fid_logit, y_pred, y, acc


def _fidelity_rows(pos, neg, pos_out_ori, neg_out_ori, y_ori, device_metrics=False):
    """threshold_test's five figures (AP, AUC, accuracy, fidelity of probabilities and of logits) of every masked
    copy on its own, float64 [G, 5]: a device tensor with ``device_metrics`` (one rank_metrics launch, nothing waits
    for the device), else numpy with AP and AUC from scikit-learn."""
    fid_prob, fid_logit, y_pred, y, acc = _fidelity_terms(pos, neg, pos_out_ori, neg_out_ori, y_ori)
    tail = torch.stack([acc, fid_prob, fid_logit], dim=1).double()
    if device_metrics:
        from .metrics import rank_metrics
        return torch.cat([rank_metrics(y.reshape(-1), y_pred), tail], dim=1)
    y_pred_h, y_h = y_pred.cpu().numpy(), y_ori.reshape(-1).cpu().numpy()
    rank = [[average_precision_score(y_h, p), roc_auc_score(y_h, p)] for p in y_pred_h]
    return np.concatenate([np.asarray(rank, np.float64).reshape(-1, 2), tail.cpu().numpy()], axis=1)


def motif_masked_nodes(ranked_rows, subgraphs, n_degree, m_list, hops=2):
    """[Gm, 3B, ne] int32 node records that keep only the events of each row's top m motifs, for every m of
    ``m_list``: one launch of ``tm_motif_mask``.  ``ranked_rows``: the per-row ranking
    ``ranked_motifs(imp, walks, k, pairs=False)`` with k >= max(m_list); ``subgraphs``: the three sides' (node, eid,
    time) records; hops=2: [hop-1 | hop-2] records, ne = N + N^2 (tgn, tgat), hops=1: ne = N (graphmixer).  A slot
    keeps its node id iff its edge id is one of the ids of the first min(m, count) triples of its row."""
    eid3, count = ranked_rows.eid, ranked_rows.count
    dev = L.require_device(eid3.device)
    if eid3.dim() != 3 or eid3.shape[-1] != 3 or count.dim() != 1:
        raise ValueError(f"motif_masked_nodes: ranked_rows is a per-row ranking (pairs=False), eid "
                         f"{tuple(eid3.shape)} is not [rows, k, 3]")
    N = int(n_degree)
    ne = N + N * N if hops == 2 else N
    rec = lambda i: torch.cat([torch.cat([as_dev(sg[i][h], dev, torch.int32) for h in range(hops)], dim=1)  # noqa: E731
                               for sg in subgraphs], dim=0).contiguous()
    nodes, eids = rec(0), rec(1)
    rows, k = eid3.shape[0], eid3.shape[1]
    if tuple(nodes.shape) != (rows, ne) or tuple(eids.shape) != (rows, ne):
        raise ValueError(f"motif_masked_nodes: subgraph records {tuple(nodes.shape)} do not match the ranking's "
                         f"({rows}, {ne})")
    ms = [int(m) for m in m_list]
    if not ms or min(ms) < 1 or max(ms) > k:
        raise ValueError(f"motif_masked_nodes: m_list {ms} is outside [1, {k}], the ranked motifs of a row")
    m_host = np.asarray(ms, dtype=np.int32)
    out = torch.empty((len(ms), rows, ne), dtype=torch.int32, device=dev)
    L.check(L.lib().tm_motif_mask(L.ptr(eid3.contiguous()), L.ptr(count.contiguous()), rows, k, L.ptr(nodes),
                                  L.ptr(eids), ne, m_host.ctypes.data, len(ms), L.ptr(out), L.stream_ptr(dev)),
            "motif_masked_nodes")
    return out


def motif_masked_contrast(args, imp, walks, base_model, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, subgraph_src,
                          subgraph_tgt, subgraph_bgd, m_list, k=None):
    """(pos [Gm, B], neg [Gm, B]) logits of contrast on the subgraphs that keep only the events of every row's top m
    motifs, all m of ``m_list`` in one batch (as masked_contrast* does for ratios): the rows are ranked
    (``ranked_motifs(imp, walks, k, pairs=False)``, k = max(m_list) by default), masked (``motif_masked_nodes``) and
    scored without weights."""
    from .ranked_motifs import ranked_motifs
    if args.base_type not in ("tgn", "graphmixer", "tgat"):
        raise NotImplementedError(f"motif_threshold_test for base_type {args.base_type!r}: tgn, graphmixer and tgat "
                                  "are built")
    ms = [int(m) for m in m_list]
    sgs = (subgraph_src, subgraph_tgt, subgraph_bgd)
    hops = 1 if args.base_type == "graphmixer" else 2
    ranked = ranked_motifs(imp, walks, max(ms) if k is None else int(k), pairs=False)
    masked = motif_masked_nodes(ranked, sgs, args.n_degree, ms, hops)
    batch = (src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, sgs, args.n_degree)
    if hops == 1:
        return _contrast_nodes_graphmixer(base_model, masked, *batch)
    return _contrast_nodes(base_model, masked, *batch, side_segments=args.base_type == "tgat")


def motif_threshold_test(args, imp, walks, base_model, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, e_l_cut,
                         pos_out_ori, neg_out_ori, y_ori, subgraph_src, subgraph_tgt, subgraph_bgd, m_list, k=None,
                         device_metrics=False):
    """threshold_test at the motif level: for every m of ``m_list`` only the events of each row's top m motif
    instances stay in the subgraphs and the base model is scored again against its original predictions.  Returns
    threshold_test's five figures (AP, AUC, accuracy, fidelity of probabilities and of logits) per m, not averaged:
    float64 [Gm, 5], a device tensor with ``device_metrics``, else numpy.  ``imp``, ``walks``: the walk scores and
    the walks as ``ranked_motifs`` takes them; the batch arguments are threshold_test's."""
    with torch.no_grad():
        pos, neg = motif_masked_contrast(args, imp, walks, base_model, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut,
                                         subgraph_src, subgraph_tgt, subgraph_bgd, m_list, k)
        return _fidelity_rows(pos, neg, pos_out_ori, neg_out_ori, y_ori, device_metrics)
