"""fp64 restatement of the attention probabilities (csrc/attn_probs.h: tm_tgn_attn_probs / tm_tgat_attn_probs), the
comparator of tests/test_attn_probs_cpu.py and tests/test_gpu_attn_probs.py, and the loader of the reference's own
probabilities (tests/golden/attn_probs_uslegis.npz, make_attn_probs_goldens.py).

``probs``: keys [node | edge | cos(u)] with u formed in fp32 as each flavour forms it -- TGAT two roundings
(tgat_ref.keys), TGN one fma (tgn_train_ref.time_arg) -- scores qf_h . key / T in fp64, masked scores -1e10 with the
mask row of pair (r, h) from tgat_ref.pair_rows inside each segment of seg_rows rows, then softmax over j.  The
explanation weight plays no part: the forward multiplies by it after the softmax.
"""
import os

import numpy as np
import torch

import tgat_ref as R
import tgn_inputs as TI
import tgn_train_ref as TR


def keys(flavour, node, edge, dt, time_w, time_b):
    """node [R, N, dn], edge [R, N, de], dt [R, N] (fp32), time_w / time_b [d_time] (fp32) -> [R, N, dk] fp64."""
    if flavour == "tgat":
        return R.keys(node, edge, dt, time_w, time_b)
    if flavour != "tgn":
        raise ValueError(flavour)
    return torch.cat([node.double(), edge.double(), torch.cos(TR.time_arg(dt.float(), time_w.float(), time_b.float()))],
                     dim=-1)


def pair_rows(rows, H, head_major, seg_rows=0):
    """Mask row of pair (r, h): tgat_ref.pair_rows inside each segment of seg_rows rows (0: one segment)."""
    seg = seg_rows or rows
    if rows % seg:
        raise ValueError("rows must be a multiple of seg_rows")
    one = R.pair_rows(seg, H, head_major)
    return torch.cat([one + s * seg for s in range(rows // seg)], dim=0) if rows else one[:0]


def probs(qf, key, mask_node, temperature, head_major=True, seg_rows=0):
    """qf [R, H, dk], key [R, N, dk] (fp64), mask_node [R, N] (0 = masked) -> softmax(masked scores) [R, H, N]."""
    Rr, H, _ = qf.shape
    m = pair_rows(Rr, H, head_major, seg_rows)
    s = torch.einsum("rhc,rjc->rhj", qf.double(), key.double()) / temperature
    s = s.masked_fill(mask_node[m] == 0, -1e10)
    return torch.softmax(s, dim=-1)


def head_mean32(p):
    """The kernel's ``mean`` from its own ``probs`` [R, H, N] (fp32 numpy): added in head order, divided by H."""
    p = np.asarray(p, dtype=np.float32)
    acc = np.zeros(p[:, 0].shape, dtype=np.float32)
    for h in range(p.shape[1]):
        acc = acc + p[:, h]
    return acc / np.float32(p.shape[1])


# ------------------------------------------------------------------ the reference's probabilities
GOLDEN_B = 8


def golden():
    return np.load(os.path.join(TI.G, "attn_probs_uslegis.npz"))


def golden_tol(g, name):
    """10 x the reference's own fp32-vs-fp64 distance on ``name`` ("tgn_hop1", ...), at least 1e-6."""
    env = float(np.abs(g[name + "_32"].astype(np.float64) - g[name + "_64"].astype(np.float64)).max())
    return max(10.0 * env, 1e-6)


def golden_batch():
    """The golden's batch: the first 8 events of tgn_inputs.load_batch() as their own batch."""
    return TI.load_batch(bsz=GOLDEN_B)


def _stack(d, i, h):
    return np.concatenate([d["sg_" + s][i][h] for s in TI.SIDES], axis=0)


def hop2_inputs(flavour, model, d, node_table):
    """What the hop-2 pass of ``model`` (the hop-1 nodes over their raw hop-2 neighbours; tempme_amd's TGN or TGAT on
    the CPU) hands the kernel, from the batch ``d`` and the node table [n_nodes, d] the pass gathers from (TGN:
    updated memory + features, TGAT: features): (qf [R, H, dk] fp64, key [R, N, dk] fp64, mask [R, N], T, seg_rows)
    with R = 3B N rows.  The folded projection is attn_layer.fold's, in fp64."""
    from tempme_amd import attn_layer as AL
    B, N = d["B"], d["N"]
    n1 = torch.from_numpy(_stack(d, 0, 0)).long().reshape(-1)                    # [3B N]
    n2 = torch.from_numpy(_stack(d, 0, 1)).long().reshape(3 * B * N, N)
    e2 = torch.from_numpy(_stack(d, 1, 1)).long().reshape(3 * B * N, N)
    t1 = torch.from_numpy(_stack(d, 2, 0)).double().reshape(3 * B * N, 1)
    t2 = torch.from_numpy(_stack(d, 2, 1)).double().reshape(3 * B * N, N)
    cut = torch.from_numpy(np.tile(d["ts_cut"], 3)).double().reshape(3 * B, 1)
    dt1 = (cut - t1.reshape(3 * B, N)).float().reshape(-1)                       # the hop-1 rows' own time offset
    dt2 = (t1 - t2).float()
    tab = node_table.double()
    ef = model.e_feat_th.detach().double()
    if flavour == "tgn":
        mh = model.embedding_module.attention_models[0].multi_head_target
        tw, tb = model.time_encoder.w.weight.detach().reshape(-1), model.time_encoder.w.bias.detach()
        query = torch.cat([tab[n1], torch.cos(tb.float()).double().expand(n1.shape[0], -1)], dim=1)
        seg = 0
    else:
        mh = model.attn_model_list[0].multi_head_target
        tw, tb = model.time_encoder.basis_freq.detach(), model.time_encoder.phase.detach()
        src_t = torch.cos((dt1.reshape(-1, 1) * tw.float() + tb.float()).double())      # two roundings
        query = torch.cat([tab[n1], tab.new_zeros((n1.shape[0], ef.shape[1])), src_t], dim=1)
        seg = B * N
    P, _ = AL.fold(mh, torch.float64, torch.device("cpu"))
    H = mh.n_head
    qf = (query @ P.t()).reshape(n1.shape[0], H, -1)
    key = keys(flavour, tab[n2], ef[e2], dt2, tw, tb)
    return qf, key, n2.to(torch.int32), float(mh.temperature), seg
