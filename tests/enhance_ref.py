"""Torch restatement of the motif-enhanced link predictor (models/explainer_new.py:203-306), dtype-parametric, for
the enhance tests and the golden generator's fp32 envelopes.

Functional (no nn.Module) on a state dict ``sd`` with the reference's key names; everything computes in the
dtype of ``sd``'s tensors (fp32: what the reference computes; fp64: the envelope's yardstick), except what the
reference forms in fp32 from its inputs whatever the model's dtype: the walk times, the time encoder's argument
(two roundings, explainer_new.py:56-58) and the cut times.

  walk_importance     :260-306  ``reduce64``: the three group reductions (two unbiased stds, one mean) as fp64
                                sums of the fp32 elements rounded to fp32, elementwise arithmetic in fp32 -- what
                                tm_walk_importance computes (include/tempme.h)
  attention_out       :222-245  event features, event_gcn x2, (temporal-aware) attention -> [B, W, h]
  predict_walks       :221-258  sum_w wgt * attention_out, then the node-level category histogram
  predict_agg         :203-213  pairs through affinity_score (_MergeLayer :62-76) -> (pos, neg)
"""
import numpy as np
import torch
import torch.nn.functional as F


def _lin(sd, name, x):
    return F.linear(x, sd[name + ".weight"], sd[name + ".bias"])


def _f32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).float()


def _long(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long)


def walk_importance(node_degree, ts, node, cut, dtype=torch.float32, reduce64=False):
    """[B, W] walk weights of one reference call.  dtype: the arithmetic's (fp32 or fp64); reduce64 (with
    fp32): the group std / mean / std as fp64 sums of the fp32 elements, rounded to fp32."""
    t, cut, node = _f32(ts).to(dtype), _f32(cut).to(dtype), _long(node)
    W = t.shape[1]
    deg = torch.as_tensor(node_degree).to(dtype)

    def std(x):
        return x.double().std().to(x.dtype) if reduce64 else x.std()

    def mean(x):
        return x.double().mean().to(x.dtype) if reduce64 else x.mean()

    diff = torch.abs(cut.unsqueeze(1) - t.max(dim=-1)[0])
    rec = torch.exp(-diff / (std(diff) + 1e-6))
    valid = node > 0
    d = torch.where(valid, deg[node], torch.zeros((), dtype=dtype))
    avg = d.sum(dim=-1) / (valid.sum(dim=-1).to(dtype) + 1e-6)
    dw = torch.sigmoid((avg - mean(avg)) / (std(avg) + 1e-6))
    imp = 0.5 * rec + 0.5 * dw
    return imp / (imp.sum(dim=-1, keepdim=True) / W + 1e-6)


def avg_degree_std(node_degree, node):
    """The group std of the walks' mean degree (fp64): far above the 1e-6 added to it, or the degree weights are
    rounding noise."""
    node = _long(node)
    valid = node > 0
    d = torch.where(valid, torch.as_tensor(node_degree).double()[node], torch.zeros((), dtype=torch.float64))
    avg = d.sum(dim=-1) / (valid.sum(dim=-1).double() + 1e-6)
    return float(avg.std())


def time_encode(sd, t):
    w, ph = sd["time_encoder.basis_freq"], sd["time_encoder.phase"]
    m = t.float().unsqueeze(-1) * w.float()
    m = m + ph.float()
    return torch.cos(m.to(w.dtype))


def attention_out(sd, n_feat, e_feat, node, eid, ts, cut, edge_count, temporal=True):
    """``self.attention(updated_feature, ...)`` of enhance_predict_walks -> [B, W, h] in sd's dtype."""
    node, eid, t, cut = _long(node), _long(eid), _f32(ts), _f32(cut)
    dty = sd["event_conv.lin_event.weight"].dtype
    cnt = _f32(edge_count).to(dty)
    n_feat, e_feat = n_feat.to(dty), e_feat.to(dty)
    B, W = eid.shape[0], eid.shape[1]
    dt = t[:, :, 2:3] - t
    tf = time_encode(sd, dt.reshape(B, -1)).reshape(B, W, 3, -1)
    ev = torch.cat([e_feat[eid], cnt.reshape(B, W, 3, 3), tf], dim=-1)
    xs, xt = n_feat[node[:, :, [0, 2, 4]]], n_feat[node[:, :, [1, 3, 5]]]
    lev = _lin(sd, "event_conv.lin_event", ev)

    def mlp(x):
        return _lin(sd, "event_conv.MLP.2", torch.relu(_lin(sd, "event_conv.MLP.0", x)))
    f = torch.cat([mlp(xs + torch.relu(xt + lev)), mlp(xt + torch.relu(xs + lev))], dim=-1)
    src = f[:, :, 2, :]
    wq = _lin(sd, "attention.W2", f[:, :, 0:2, :])
    scores = (_lin(sd, "attention.W1", src).unsqueeze(2) * wq).sum(-1)
    if temporal:
        diff = torch.abs(cut.view(B, 1, 1) - t[:, :, :2])
        scores = scores * (1.0 - 0.3 + 0.3 * torch.exp(-diff / (diff.std() + 1e-6)).to(dty))
    alpha = torch.softmax(scores, dim=-1)
    hid = torch.relu(_lin(sd, "attention.MLP.0", src + (alpha.unsqueeze(-1) * wq).sum(2)))
    return _lin(sd, "attention.MLP.3" if "attention.MLP.3.weight" in sd else "attention.MLP.2", hid)


def predict_walks(sd, n_feat, e_feat, node_degree, walks, cut, edge_count, temporal=True, if_cat=True, wgt=None):
    """walks = (node [B,W,6], eid [B,W,3], ts [B,W,3], cat [B,W(,1)]) -> [B, h (+ 12)]."""
    node, eid, ts, cat = walks[:4]
    dty = sd["event_conv.lin_event.weight"].dtype
    out = attention_out(sd, n_feat, e_feat, node, eid, ts, cut, edge_count, temporal)
    if wgt is None:
        wgt = walk_importance(node_degree, ts, node, cut, dtype=dty)
    x = (out * wgt.to(dty).unsqueeze(-1)).sum(1)
    if if_cat:
        B, W = out.shape[0], out.shape[1]
        x = torch.cat([x, F.one_hot(_long(cat).reshape(B, W), 12).sum(1).to(dty)], dim=-1)
    return x


def affinity(sd, x1, x2):
    h = torch.relu(_lin(sd, "affinity_score.fc1", torch.cat([x1, x2], dim=-1)))
    return _lin(sd, "affinity_score.fc2", h)


def predict_agg(sd, n_feat, e_feat, node_degree, cut, sides, gats, temporal=True, if_cat=True):
    """sides = three (walks, edge_count) for src / tgt / bgd, gats = their base embeddings [B, node_dim]
    -> (pos [B, 1], neg [B, 1], the three walk embeddings)."""
    dty = sd["event_conv.lin_event.weight"].dtype
    emb = [predict_walks(sd, n_feat, e_feat, node_degree, w, cut, c, temporal, if_cat) for w, c in sides]
    full = [torch.cat([e, g.to(dty)], dim=-1) for e, g in zip(emb, gats)]
    return affinity(sd, full[0], full[1]), affinity(sd, full[0], full[2]), emb
