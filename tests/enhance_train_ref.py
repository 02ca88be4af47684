"""Torch restatement of enhance_predict_walks (models/explainer_new.py:221-258) in training, dtype-parametric, for
the pooled encoder's training tests: tests/enhance_ref.py's formulas with the attention's two dropouts given as
keep-masks (alpha :839, attention.MLP's hidden layer :780), plus seeded small inputs and the fp32 / fp64 autograd
gradients the tolerances come from.

Everything computes in the dtype of the state dict's tensors, except what the reference forms in fp32 whatever the
model's dtype (walk times, the time encoder's argument, cut times), as in enhance_ref.  The walk weights are
constants (enhance_ref.walk_importance in the same dtype): they get no gradient."""
import numpy as np
import torch
import torch.nn.functional as F

import enhance_ref as XR
from enhance_ref import _f32, _lin, _long

# tm_encoder_pool_wgrad's 16 gradients (include/tempme.h), as parameter names; attention.MLP's last Linear is
# MLP.3 in TemporalAwareAttention and MLP.2 in the plain Attention
POOL_PARAMS = ("event_conv.lin_event.weight", "event_conv.lin_event.bias", "event_conv.MLP.0.weight",
               "event_conv.MLP.0.bias", "event_conv.MLP.2.weight", "event_conv.MLP.2.bias", "attention.W1.weight",
               "attention.W1.bias", "attention.W2.weight", "attention.W2.bias", "attention.MLP.0.weight",
               "attention.MLP.0.bias", "attention.MLP.3.weight", "attention.MLP.3.bias", "time_encoder.basis_freq",
               "time_encoder.phase")
SCORING_PARAMS = tuple(f"MLP.{i}.{k}" for i in (0, 3, 5) for k in ("weight", "bias"))


def pool_params(temporal=True):
    return POOL_PARAMS if temporal else tuple(k.replace("attention.MLP.3", "attention.MLP.2") for k in POOL_PARAMS)


def attention_out(sd, n_feat, e_feat, node, eid, ts, cut, edge_count, temporal=True, keep=None, scale=1.0):
    """enhance_ref.attention_out with keep-masks: keep [B, W, >= 2 + h] (columns 0..1 alpha, the next h
    attention.MLP's hidden layer; kept values times scale), None = no dropout.  The plain Attention has none."""
    node, eid, t, cut = _long(node), _long(eid), _f32(ts), _f32(cut)
    dty = sd["event_conv.lin_event.weight"].dtype
    cnt = _f32(edge_count).to(dty)
    n_feat, e_feat = n_feat.to(dty), e_feat.to(dty)
    B, W = eid.shape[0], eid.shape[1]
    dt = t[:, :, 2:3] - t
    tf = XR.time_encode(sd, dt.reshape(B, -1)).reshape(B, W, 3, -1)
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
    use = temporal and keep is not None
    if use:
        keep = torch.as_tensor(keep).reshape(B, W, -1).to(dty) * scale
        alpha = alpha * keep[:, :, :2]
    hid = torch.relu(_lin(sd, "attention.MLP.0", src + (alpha.unsqueeze(-1) * wq).sum(2)))
    if use:
        hid = hid * keep[:, :, 2:2 + hid.shape[-1]]
    return _lin(sd, "attention.MLP.3" if temporal else "attention.MLP.2", hid)


def predict_walks(sd, n_feat, e_feat, node_degree, walks, cut, edge_count, temporal=True, if_cat=True, keep=None,
                  scale=1.0):
    """walks = (node [B,W,6], eid [B,W,3], ts [B,W,3], cat [B,W]) -> [B, h (+ 12)] of one reference call."""
    node, eid, ts, cat = walks[:4]
    dty = sd["event_conv.lin_event.weight"].dtype
    out = attention_out(sd, n_feat, e_feat, node, eid, ts, cut, edge_count, temporal, keep, scale)
    wgt = XR.walk_importance(node_degree, ts, node, cut, dtype=dty)
    x = (out * wgt.unsqueeze(-1)).sum(1)
    if if_cat:
        B, W = out.shape[0], out.shape[1]
        x = torch.cat([x, F.one_hot(_long(cat).reshape(B, W), 12).sum(1).to(dty)], dim=-1)
    return x


def seeded_inputs(seed, G, B, W, n_nodes=40, n_edges=90, dn=172, de=32, zero_nodes=False):
    """Feature tables, node degrees and G groups of random walks [G, B, W, ...] (numpy), ids inside the tables,
    one padding walk entry."""
    rng = np.random.default_rng(seed)
    n_feat = np.zeros((n_nodes, dn), np.float32) if zero_nodes else rng.uniform(0, 1, (n_nodes, dn)).astype(np.float32)
    d = dict(n_feat=torch.from_numpy(n_feat), e_feat=torch.from_numpy(rng.uniform(0, 1, (n_edges, de)).astype(np.float32)),
             deg=rng.integers(1, 30, n_nodes).astype(np.float32), G=G, B=B, W=W)
    node = rng.integers(0, n_nodes, (G, B, W, 6))
    node[:, :, :, 4:6] = rng.integers(1, n_nodes, (G, B, W, 2))
    node[0, 0, 1, 0:2] = 0
    d["node"], d["eid"] = node, rng.integers(1, n_edges, (G, B, W, 3))
    d["cut"] = np.floor(rng.uniform(50, 60, B))                       # one batch: the groups share the cut times
    d["ts"] = np.sort(np.floor(rng.uniform(0, 50, (G, B, W, 3))), axis=-1)
    d["cnt"] = rng.integers(0, 4, (G, B, W, 3, 3)).astype(np.float64)
    d["cat"] = rng.integers(0, 12, (G, B, W))
    return d


def groups(sd, d, temporal, if_cat, keep=None, scale=1.0):
    """[G, B, h (+ 12)]: predict_walks per group (one reference call each); keep [G*B*W, cols] or None."""
    G, B, W = d["G"], d["B"], d["W"]
    k = None if keep is None else torch.as_tensor(keep).reshape(G, B, W, -1)
    return torch.stack([predict_walks(sd, d["n_feat"], d["e_feat"], d["deg"],
                                      (d["node"][g], d["eid"][g], d["ts"][g], d["cat"][g]), d["cut"], d["cnt"][g],
                                      temporal, if_cat, None if k is None else k[g], scale) for g in range(G)])


def forward_and_grads(sd, d, d_emb, temporal, if_cat, keep=None, scale=1.0, dtype=torch.float64):
    """The embeddings [G, B, h (+ 12)] and the gradients of sum(emb * d_emb) w.r.t. every parameter of sd, by
    autograd in `dtype` (None where a parameter takes no part)."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    emb = groups(p, d, temporal, if_cat, keep, scale)
    names = list(p)
    gs = torch.autograd.grad((emb * d_emb.to(dtype)).sum(), [p[k] for k in names], allow_unused=True)
    return emb.detach(), dict(zip(names, gs))
