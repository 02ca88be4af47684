"""fp64 torch restatement of what the attention kernels compute in their TGAT flavour (csrc/attn_kernels.h), for the C-ABI tests.

``attn`` is one attention pass in the folded form: keys [node | edge | cos(fl(fl(dt w) + b))], scores
qf_h . key / T, masked scores -1e10, softmax, times the explanation weight, weighted key sum; the mask /
weight row of pair (r, h) is (r n_head + h) % rows when head-major (MultiHeadAttention's
.repeat(n_head, 1, 1), TGAT.py:128-130).  The time argument is formed in fp32 with two roundings, as the
reference's TimeEncode and the kernel do; everything after it is fp64.
``tail`` is the layer tail: LayerNorm(z G^T + fc_b + query), then the two-branch MergeLayer.
"""
import torch


def pair_rows(R, H, head_major):
    r = torch.arange(R).view(R, 1)
    h = torch.arange(H).view(1, H)
    return ((r * H + h) % R) if head_major else r.expand(R, H)


def keys(node, edge, dt, time_w, time_b):
    """node [R, N, dn], edge [R, N, de], dt [R, N] (fp32), time_w / time_b [d_time] (fp32) -> [R, N, dk] fp64."""
    arg = dt.float().unsqueeze(-1) * time_w.float()       # rounded
    arg = arg + time_b.float()                            # rounded again
    return torch.cat([node.double(), edge.double(), torch.cos(arg.double())], dim=-1)


def attn(qf, key, mask_node, ew, temperature, head_major=True):
    """qf [R, H, dk], key [R, N, dk], mask_node [R, N] (0 = masked), ew [R, N] or None -> z [R, H, dk]."""
    R, H, _ = qf.shape
    m = pair_rows(R, H, head_major)                                    # [R, H]
    s = torch.einsum("rhc,rjc->rhj", qf.double(), key) / temperature
    s = s.masked_fill(mask_node[m] == 0, -1e10)
    p = torch.softmax(s, dim=-1)
    if ew is not None:
        p = p * ew.double()[m]
    return torch.einsum("rhj,rjc->rhc", p, key)


def tail(z, query, w, feat):
    """w: dict of fp64 tensors G [dk, K1], fcb, lnw, lnb, w11 [feat, dk], b11, w12, b12, w21, b21, w22, b22
    (nn.Linear layout) -> [rows, feat]."""
    lin = torch.nn.functional.linear
    u = lin(z, w["G"], w["fcb"]) + query
    h = torch.nn.functional.layer_norm(u, (u.shape[1],), w["lnw"], w["lnb"], 1e-5)
    x1 = lin(torch.relu(lin(h, w["w11"], w["b11"])), w["w21"], w["b21"])
    x2 = lin(torch.relu(lin(query[:, :feat], w["w12"], w["b12"])), w["w22"], w["b22"])
    return x2 + x1
