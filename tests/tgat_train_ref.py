"""TEST INFRASTRUCTURE ONLY -- torch restatement of the base TGAT's TRAINING step in the reference's own shape
(TGAT/TGAT.py: contrast :461-481 -> forward_msg :607-619 -> AttnModel :362-386 -> MultiHeadAttention :110-137 ->
ScaledDotProductAttention :64-80, under model.train() with if_explain = False, as learn_base.py:227-229 calls it),
with the two dropouts as given keep masks and plain autograd for the gradients: what TGAT.train_on_hip
(tm_tgat_attn_train_fwd / tm_tgat_attn_train_bwd) is checked against, in any dtype.

Nothing is folded here: w_qs / w_ks / w_vs project every key, the scores are a bmm, padding is
masked_fill(-1e10), the mask is .repeat(n_head, 1, 1) (head-major), each side runs its three attention passes on
its own B rows.  The one departure from the reference is the time feature: a custom autograd.Function forms the
argument dt * basis_freq + phase in fp32 with the reference's two roundings and promotes it to the working dtype
before the cosine (backward -sin(u) * (dt, 1)), so that an fp64 run takes the cosine of the same arguments as the
fp32 model and the kernels.

keep = [attn pass 1, attn pass 2, attn pass 3, fc pass 1, fc pass 2, fc pass 3] for the R = 3B stacked rows
(src, tgt, bgd), uint8, 1 = kept, a kept value scaled by keep_scale = 1 / (1 - p); None = no dropout.  An attention
mask is flat, the byte of (row, head, neighbour) at (row H + head) N + neighbour: the reference's dropped tensor
[B*N_src*n_head, 1, N] of each side, the sides one after the other.  An fc mask is [rows, model_dim].
"""
import numpy as np
import torch
import torch.nn.functional as F

FROZEN = ("n_feat_th", "e_feat_th", "edge_raw_embed.weight", "node_raw_embed.weight")


class TimeFeature(torch.autograd.Function):
    """cos(u), u = fl32(fl32(dt * freq) + phase) promoted to the dtype of freq; d/dfreq = -sin(u) dt, d/dphase = -sin(u)."""

    @staticmethod
    def forward(ctx, dt32, freq, phase):
        u = dt32.float().unsqueeze(-1) * freq.detach().float()
        u = u + phase.detach().float()
        u = u.to(freq.dtype)
        ctx.save_for_backward(u, dt32)
        return torch.cos(u)

    @staticmethod
    def backward(ctx, g):
        u, dt32 = ctx.saved_tensors
        s = -torch.sin(u) * g
        dims = tuple(range(s.dim() - 1))
        return None, (s * dt32.to(u.dtype).unsqueeze(-1)).sum(dims), s.sum(dims)


def leaves(sd, dtype, device="cpu"):
    """state_dict -> {name: leaf tensor of `dtype` on `device`}: parameters require grad, the feature tables do not."""
    return {k: v.detach().to(device, dtype).clone().requires_grad_(k not in FROZEN) for k, v in sd.items()}


def _lin(p, name, x, bias=True):
    return F.linear(x, p[name + ".weight"], p[name + ".bias"] if bias else None)


def attn_model(p, pre, H, src, src_t, seq, seq_t, seq_e, mask, akeep, fkeep, scale):
    """AttnModel.forward: src [B, Ns, D], src_t [B, Ns, Dt], seq / seq_t / seq_e [B, Ns N, .], mask [B, Ns N] (True
    = padding), akeep [B Ns H N] / fkeep [B Ns, dm] uint8 or None -> [B, Ns, D]."""
    B, Ns, _ = src.shape
    dtype = src.dtype
    q = torch.cat([src, torch.zeros((B, Ns, seq_e.shape[2]), dtype=dtype, device=src.device), src_t], dim=2)
    k = torch.cat([seq, seq_e, seq_t], dim=2)
    dm = q.shape[2]
    dk = dm // H
    N = k.shape[1] // Ns
    mh = pre + "multi_head_target."
    residual = q
    qp = _lin(p, mh + "w_qs", q, False).view(B, Ns, 1, H, dk)
    kp = _lin(p, mh + "w_ks", k, False).view(B, Ns, N, H, dk)
    vp = _lin(p, mh + "w_vs", k, False).view(B, Ns, N, H, dk)
    qp = qp.transpose(2, 3).contiguous().view(B * Ns * H, 1, dk)
    kp = kp.transpose(2, 3).contiguous().view(B * Ns * H, N, dk)
    vp = vp.transpose(2, 3).contiguous().view(B * Ns * H, N, dk)
    m = mask.view(B * Ns, 1, N).repeat(H, 1, 1)
    attn = torch.bmm(qp, kp.transpose(-1, -2)) / float(np.power(dk, 0.5))
    attn = attn.masked_fill(m, -1e10)
    attn = torch.softmax(attn, dim=2)
    if akeep is not None:
        attn = attn * (akeep.reshape(B * Ns * H, 1, N).to(dtype) * scale)
    out = torch.bmm(attn, vp).view(B, Ns, H * dk)
    out = _lin(p, mh + "fc", out)
    if fkeep is not None:
        out = out * (fkeep.reshape(B, Ns, dm).to(dtype) * scale)
    out = F.layer_norm(out + residual, (dm,), p[mh + "layer_norm.weight"], p[mh + "layer_norm.bias"], 1e-5)
    mg = pre + "merger."
    return _lin(p, mg + "fc22", F.relu(_lin(p, mg + "fc12", src))) + _lin(p, mg + "fc21", F.relu(_lin(p, mg + "fc11", out)))


def prepare_side(roots, cut, sg, device=None):
    """One side's indices and time deltas as tensors on `device` (retrieve_time_features :653-666 forms the deltas
    in fp64 and rounds them to fp32)."""
    nodes, eids, ts = sg
    B = len(roots)

    def arr(x, dtype):
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        return x.astype(dtype)
    n1 = arr(nodes[0], np.int64).reshape(B, -1)
    N = n1.shape[1]
    cut = arr(cut, np.float64).reshape(B, 1)
    t1 = arr(ts[0], np.float64).reshape(B, N)
    t2 = arr(ts[1], np.float64).reshape(B, N, N)
    dts = [np.zeros((B, 1)), cut - t1, (t1[:, :, None] - t2).reshape(B, N * N)]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)  # noqa: E731
    return dict(B=B, N=N, roots=t(arr(roots, np.int64).reshape(B, 1)), n1=t(n1), n2=t(arr(nodes[1], np.int64).reshape(B, N * N)),
                e1=t(arr(eids[0], np.int64).reshape(B, N)), e2=t(arr(eids[1], np.int64).reshape(B, N * N)),
                dts=[t(d.astype(np.float32)) for d in dts])


def forward_msg(p, H, side, keep, scale):
    """forward_msg with num_layers = 2 for one prepared side -> [B, D].  keep: this side's six masks or None."""
    dtype = p["affinity_score.fc1.weight"].dtype
    nf, ef = p["n_feat_th"].to(dtype), p["e_feat_th"].to(dtype)
    freq, phase = p["time_encoder.basis_freq"], p["time_encoder.phase"]
    tf = [TimeFeature.apply(d, freq, phase) for d in side["dts"]]
    hid = [nf[side["roots"]], nf[side["n1"]], nf[side["n2"]]]
    edge = [ef[side["e1"]], ef[side["e2"]]]
    masks = [side["n1"] == 0, side["n2"] == 0]
    k = keep if keep is not None else [None] * 6
    a0, a1 = "attn_model_list.0.", "attn_model_list.1."
    h0 = attn_model(p, a0, H, hid[0], tf[0], hid[1], tf[1], edge[0], masks[0], k[0], k[3], scale)
    h1 = attn_model(p, a0, H, hid[1], tf[1], hid[2], tf[2], edge[1], masks[1], k[1], k[4], scale)
    out = attn_model(p, a1, H, h0, tf[0], h1, tf[1], edge[0], masks[0], k[2], k[5], scale)
    return out.squeeze(1)


def side_keep(keep, s, device=None):
    """The six stacked masks -> side s's part (the sides are consecutive blocks of rows)."""
    if keep is None:
        return None
    out = []
    for m in keep:
        m = torch.as_tensor(m).to(device)
        flat = m.reshape(3, -1) if m.dim() == 1 else m.reshape(3, m.shape[0] // 3, -1)
        out.append(flat[s])
    return out


def prepare(src, dst, fake, cut, sg_src, sg_tgt, sg_bgd, device=None):
    return [prepare_side(r, cut, sg, device) for r, sg in ((src, sg_src), (dst, sg_tgt), (fake, sg_bgd))]


def contrast_prepared(p, H, sides, keep=None, keep_scale=1.0):
    """TGAT.contrast(if_explain=False) in training mode on prepared sides -> (pos [B, 1], neg [B, 1])."""
    dev = p["affinity_score.fc1.weight"].device
    emb = [forward_msg(p, H, side, side_keep(keep, s, dev), keep_scale) for s, side in enumerate(sides)]

    def aff(x1, x2):
        return _lin(p, "affinity_score.fc2", F.relu(_lin(p, "affinity_score.fc1", torch.cat([x1, x2], dim=1))))
    return aff(emb[0], emb[1]), aff(emb[0], emb[2])


def contrast(p, H, src, dst, fake, cut, sg_src, sg_tgt, sg_bgd, keep=None, keep_scale=1.0):
    dev = p["affinity_score.fc1.weight"].device
    return contrast_prepared(p, H, prepare(src, dst, fake, cut, sg_src, sg_tgt, sg_bgd, dev), keep, keep_scale)


def loss_of(p, H, batch, keep=None, keep_scale=1.0):
    pos, neg = contrast(p, H, *batch, keep=keep, keep_scale=keep_scale)
    crit = torch.nn.BCEWithLogitsLoss()
    return crit(pos, torch.ones_like(pos)) + crit(neg, torch.zeros_like(neg)), pos, neg


def loss_and_grads(sd, H, batch, keep=None, keep_scale=1.0, dtype=torch.float64):
    """learn_base.py:233-236: BCEWithLogits(pos, 1) + BCEWithLogits(neg, 0), backward.
    batch = (src, dst, fake, cut, sg_src, sg_tgt, sg_bgd) -> (loss, pos, neg, {name: grad})."""
    p = leaves(sd, dtype)
    loss, pos, neg = loss_of(p, H, batch, keep, keep_scale)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items() if v.requires_grad}
    return loss.detach(), pos.detach(), neg.detach(), grads
