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


def masked_contrast(base_model, explanation, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, subgraph_src, subgraph_tgt,
                    subgraph_bgd, n_degree, ratios, side_segments=False):
    """(pos [G, B], neg [G, B]) logits of contrast on the masked subgraph of every ratio: [hop-1 | hop-2] records
    masked, then contrast without weights, all ratios in one batch.  ``explanation``: (hop-1 [3B, N], hop-2
    [3B, N^2]).  ``side_segments`` (tgat): every (ratio, side) is one forward_msg call of B rows, a segment of its
    own; else (tgn) a ratio's three sides are one segment."""
    dev = base_model._dev()
    B, N, G = len(src_l_cut), n_degree, len(ratios)
    sgs = (subgraph_src, subgraph_tgt, subgraph_bgd)
    masked = _masked_nodes(explanation, sgs, N, ratios, dev)                          # [G, 3B, ne]
    roots, _, eids, times = stack_sides(dev, (src_l_cut, dst_l_cut, dst_l_fake), sgs, nodes=False)
    n1 = masked[:, :, :N].reshape(G * 3 * B, N)
    n2 = masked[:, :, N:].reshape(G * 3 * B, N * N)
    emb = base_model.node_embeddings([roots.repeat(G), n1, n2], [x.repeat(G, 1) for x in eids],
                                     [x.repeat(G, 1) for x in times], ts_l_cut,
                                     n_segments=3 * G if side_segments else G)
    return _pair_scores(base_model, emb, G, B)


def masked_contrast_graphmixer(base_model, explanation, src_l_cut, dst_l_cut, dst_l_fake, ts_l_cut, subgraph_src,
                               subgraph_tgt, subgraph_bgd, n_degree, ratios):
    """graphmixer branch (temp_exp_main.py:186-206): hop-1 records masked, all ratios in one batch."""
    dev = base_model._dev()
    B, N, G = len(src_l_cut), n_degree, len(ratios)
    sgs = (subgraph_src, subgraph_tgt, subgraph_bgd)
    masked = _masked_nodes(explanation, sgs, N, ratios, dev, hops=1).reshape(G * 3 * B, N)
    roots, _, (eid,), (t,) = stack_sides(dev, (src_l_cut, dst_l_cut, dst_l_fake), sgs, nodes=False, hops=1,
                                         idx_dtype=torch.long)
    cut = as_dev(ts_l_cut, dev, torch.float64).reshape(-1).repeat(3 * G)
    emb = base_model.node_embeddings(roots.repeat(G), cut, masked, eid.repeat(G, 1), t.repeat(G, 1))
    return _pair_scores(base_model, emb, G, B)


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
        po = pos_out_ori.reshape(1, -1).to(pos.device, torch.float32)
        no = neg_out_ori.reshape(1, -1).to(pos.device, torch.float32)
        fid_prob = torch.cat([pos.sigmoid() - po.sigmoid(), no.sigmoid() - neg.sigmoid()], dim=1).mean(1)
        fid_logit = torch.cat([pos - po, no - neg], dim=1).mean(1)
        y_pred = torch.cat([pos, neg], dim=1).sigmoid()
        pred_label = torch.where(y_pred > 0.5, 1., 0.)
        y = y_ori.reshape(1, -1).to(pos.device, torch.float32)
        acc = (pred_label == y).float().mean(1)
        if device_metrics:
            from .metrics import rank_metrics
            m = rank_metrics(y.reshape(-1), y_pred).mean(0)
            return torch.cat([m, torch.stack([acc.mean(), fid_prob.mean(), fid_logit.mean()]).double()])
        y_pred_h, y_h = y_pred.cpu().numpy(), y_ori.reshape(-1).cpu().numpy()
    aps = [average_precision_score(y_h, p) for p in y_pred_h]
    auc = [roc_auc_score(y_h, p) for p in y_pred_h]
    return (float(np.mean(aps)), float(np.mean(auc)), float(acc.mean().item()), float(fid_prob.mean().item()),
            float(fid_logit.mean().item()))
