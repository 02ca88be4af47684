"""TEST INFRASTRUCTURE ONLY -- torch restatement of the base GraphMixer's TRAINING forward (GraphM/graphmixer.py
:142-193, :244-315 under model.train(), explain_weights = None, edge_attr = None, as learn_base.py:228-232 calls
it), with the dropout keep masks as inputs and plain autograd for the gradients: what tm_gm_train_fwd /
tm_gm_train_bwd are checked against.  The eval-mode restatement is oracle/graphmixer_ref.py; this one differs by
the four dropouts of every mixer layer (FeedForwardNet: after the GELU and after the second Linear, in the token
and the channel FFN) and by running the three sides as one batch of R = 3B rows, the unit the masks are laid out in.

keep (uint8, or None for no dropout) holds, for each layer in order, tok_h [R][C][HT], tok_o [R][C][N],
ch_h [R][N][HC], ch_o [R][N][C]; 1 = kept, a kept value is scaled by keep_scale = 1 / (1 - p).
"""
import numpy as np
import torch
import torch.nn.functional as F


def split_keep(keep, n_layers, R, N, C, HT, HC):
    """The flat mask array -> per layer (tok_h [R,C,HT], tok_o [R,C,N], ch_h [R,N,HC], ch_o [R,N,C])."""
    if keep is None:
        return [(None, None, None, None)] * n_layers
    keep = torch.as_tensor(keep).reshape(-1).cpu()
    sizes = [(R, C, HT), (R, C, N), (R, N, HC), (R, N, C)]
    out, o = [], 0
    for _ in range(n_layers):
        parts = []
        for sh in sizes:
            n = int(np.prod(sh))
            parts.append(keep[o:o + n].reshape(sh))
            o += n
        out.append(tuple(parts))
    assert o == keep.numel()
    return out


def _drop(x, k, scale):
    return x if k is None else x * (k.to(x.dtype) * scale)


def _lin(p, name, x):
    return F.linear(x, p[name + ".weight"], p[name + ".bias"])


def node_embeddings(p, n_layers, node_ids, cut, nid, eid, times, keep=None, keep_scale=1.0):
    """p: {name: tensor} (parameters as leaves of the wanted dtype, the two feature tables and the time encoder
    included) -> compute_node_temporal_embeddings for R rows [R, d]."""
    dtype = p["projection_layer.weight"].dtype
    nf, ef_tab = p["n_feat_th"].to(dtype), p["e_feat_th"].to(dtype)
    nid_np = np.asarray(nid)
    nid_t = torch.as_tensor(nid_np).long()
    pad = torch.from_numpy(nid_np == 0)
    ef = ef_tab[torch.as_tensor(np.asarray(eid)).long()].clone()
    delta = np.asarray(cut, dtype=np.float64).reshape(-1, 1) - np.asarray(times, dtype=np.float64)
    w = p["time_encoder.w.weight"].reshape(-1).double()
    b = p["time_encoder.w.bias"].double()
    arg = (torch.from_numpy(delta).float().double().unsqueeze(-1) * w + b).float()   # one rounding of t*w+b
    tf = torch.cos(arg.double()).to(dtype)
    tf[pad] = 0.0
    ef[pad] = 0.0
    x = _lin(p, "projection_layer", torch.cat([ef, tf], dim=-1))
    R, N, C = x.shape
    HT = p["mlp_mixers.0.token_feedforward.ffn.0.weight"].shape[0] if n_layers else 0
    HC = p["mlp_mixers.0.channel_feedforward.ffn.0.weight"].shape[0] if n_layers else 0
    masks = split_keep(keep, n_layers, R, N, C, HT, HC)
    for i in range(n_layers):
        pre = f"mlp_mixers.{i}."
        th, to, ch, co = masks[i]
        h = F.layer_norm(x.permute(0, 2, 1), (N,), p[pre + "token_norm.weight"], p[pre + "token_norm.bias"], 1e-5)
        h = _drop(F.gelu(_lin(p, pre + "token_feedforward.ffn.0", h)), th, keep_scale)
        h = _drop(_lin(p, pre + "token_feedforward.ffn.3", h), to, keep_scale).permute(0, 2, 1)
        out = h + x
        h = F.layer_norm(out, (C,), p[pre + "channel_norm.weight"], p[pre + "channel_norm.bias"], 1e-5)
        h = _drop(F.gelu(_lin(p, pre + "channel_feedforward.ffn.0", h)), ch, keep_scale)
        h = _drop(_lin(p, pre + "channel_feedforward.ffn.3", h), co, keep_scale)
        x = h + out
    x = x * (~pad).to(dtype).unsqueeze(-1)
    x = torch.mean(x, dim=1)
    valid = torch.from_numpy((nid_np > 0).astype(np.float32)).to(dtype)
    valid[valid == 0] = -1e10
    scores = torch.softmax(valid, dim=1)
    agg = torch.mean(nf[nid_t] * scores.unsqueeze(-1), dim=1)
    out = agg + nf[torch.as_tensor(np.asarray(node_ids)).long()]
    return _lin(p, "output_layer", torch.cat([x, out], dim=1))


def leaves(sd, dtype):
    """state_dict -> {name: leaf tensor of `dtype`}: float parameters require grad, the frozen tensors do not."""
    frozen = ("n_feat_th", "e_feat_th", "node_raw_features.weight", "edge_raw_features.weight", "time_encoder.w.weight",
              "time_encoder.w.bias")
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(k not in frozen) for k, v in sd.items()}


def contrast(p, n_layers, src_idx, tgt_idx, bgd_idx, cut_time, subgraph_src, subgraph_tgt, subgraph_bgd, keep=None,
             keep_scale=1.0):
    """GraphMixer.contrast in training mode -> (pos [B,1], neg [B,1])."""
    B = len(src_idx)
    sgs = (subgraph_src, subgraph_tgt, subgraph_bgd)
    roots = np.concatenate([np.asarray(x).reshape(-1) for x in (src_idx, tgt_idx, bgd_idx)])
    cut = np.tile(np.asarray(cut_time, dtype=np.float64).reshape(-1), 3)
    nid, eid, ts = (np.concatenate([np.asarray(sg[k][0]) for sg in sgs]) for k in range(3))
    emb = node_embeddings(p, n_layers, roots, cut, nid, eid, ts, keep, keep_scale)
    s, d, n = emb[:B], emb[B:2 * B], emb[2 * B:]
    x = torch.cat([torch.cat([s, s], 0), torch.cat([d, n], 0)], dim=1)
    score = _lin(p, "affinity_score.fc2", F.relu(_lin(p, "affinity_score.fc1", x)))
    return score[:B], score[B:]


def loss_and_grads(sd, n_layers, batch, keep=None, keep_scale=1.0, dtype=torch.float64):
    """learn_base.py:233-236: BCEWithLogits(pos, 1) + BCEWithLogits(neg, 0), backward.
    batch = (src, dst, fake, cut, sg_src, sg_tgt, sg_bgd) -> (loss, pos, neg, {name: grad})."""
    p = leaves(sd, dtype)
    pos, neg = contrast(p, n_layers, *batch, keep=keep, keep_scale=keep_scale)
    crit = torch.nn.BCEWithLogitsLoss()
    loss = crit(pos, torch.ones_like(pos)) + crit(neg, torch.zeros_like(neg))
    loss.backward()
    grads = {k: v.grad for k, v in p.items() if v.requires_grad and v.grad is not None}
    return loss.detach(), pos.detach(), neg.detach(), grads
