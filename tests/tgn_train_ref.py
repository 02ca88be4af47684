"""The base TGN's stateful training step (TGN/tgn.py:100-278, learn_base.py:201-266) as a CPU / torch formulation
in the reference's shape: unfolded q / k / v projections, ``bmm``, ``masked_fill``, the head-major ``.repeat`` of
the masks, both dropouts of MultiHeadAttention as injected keep masks (in the reference's tensor shapes), and the
memory without the dict of lists: per node the last raw message, its timestamp and a flag (all the ``last``
aggregator reads), written with the reference's ordering rules.  Runs in fp32 or fp64 from a ``state_dict``.

Also ``attn_closed_form``: the fp64 closed form of one attention pass's forward and backward (the formulas of
csrc/attn_train.h and csrc/tgn_train.hip), with the gradient of a gathered node table, which the kernel tests compare against.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F


class TimeFeature(torch.autograd.Function):
    """cos(u), u = fma(t, w, b): TimeEncode is cos(Linear(1, d)), whose CPU addmm rounds t*w + b once.  The fp64
    product of two fp32 numbers is exact, so rounding the fp64 sum gives the fma.  t [...], w / b [d] -> [..., d]."""

    @staticmethod
    def forward(ctx, t, w, b):
        u = (t.double().unsqueeze(-1) * w.double() + b.double()).to(w.dtype)
        ctx.save_for_backward(t, u)
        return torch.cos(u)

    @staticmethod
    def backward(ctx, g):
        t, u = ctx.saved_tensors
        gs = -torch.sin(u) * g
        lead = tuple(range(gs.dim() - 1))
        return None, (gs * t.to(gs.dtype).unsqueeze(-1)).sum(lead), gs.sum(lead)


def _t(x, dtype, device=None):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(device=device, dtype=dtype)


class RefTGN:
    """Parameters from a state_dict (``n_heads`` heads), state as tensors.  ``step`` is one stateful contrast."""

    def __init__(self, sd, n_heads, dtype=torch.float32, device="cpu", exact_time=True):
        self.dtype, self.H, self.device = dtype, n_heads, torch.device(device)
        # exact_time: TimeEncode's argument as the CPU reference rounds it (TimeFeature, through fp64); False is
        # the plain torch expression cos(t * w + b), what a timing comparison on a device should run
        self.time = TimeFeature.apply if exact_time else (lambda t, w, b: torch.cos(t.to(w.dtype).unsqueeze(-1) * w + b))
        frozen = ("n_feat_th", "e_feat_th", "features.weight", "memory.memory", "memory.last_update")
        self.p = {}
        for k, v in sd.items():
            v = v.detach().to(self.device).clone()
            if not k.endswith(frozen):
                v = v.to(dtype).requires_grad_(True)
            self.p[k] = v
        self.nf, self.ef = self.p["n_feat_th"].to(dtype), self.p["e_feat_th"].to(dtype)
        self.n_nodes, self.dn = self.nf.shape
        self.de = self.ef.shape[1]
        self.raw_dim = 3 * self.dn + self.de
        self.memory = self.p["memory.memory"].to(dtype).clone()
        self.last_update = self.p["memory.last_update"].float().clone()     # timestamps are fp32 in the reference
        self.msg_raw = torch.zeros(self.n_nodes, self.raw_dim, dtype=dtype, device=self.device)
        self.msg_ts = torch.zeros(self.n_nodes, device=self.device)
        self.msg_flag = torch.zeros(self.n_nodes, dtype=torch.bool, device=self.device)

    # -------------------------------------------------------------- parameters
    def trainable(self):
        return {k: v for k, v in self.p.items() if v.requires_grad}

    def zero_grad(self):
        for v in self.p.values():
            v.grad = None

    def backup(self):
        return tuple(x.clone() for x in (self.memory, self.last_update, self.msg_raw, self.msg_ts, self.msg_flag))

    def restore(self, b):
        self.memory, self.last_update, self.msg_raw, self.msg_ts, self.msg_flag = (x.clone() for x in b)

    # -------------------------------------------------------------- memory
    def updated_memory(self):
        """get_updated_memory: M' = memory.data.clone(); M'[v] = GRUCell(mlp(raw_last[v]), memory[v]) for every
        node with a pending message."""
        M = self.memory.clone()
        nodes = torch.nonzero(self.msg_flag).reshape(-1)
        if len(nodes) == 0:
            return M
        return M.index_put((nodes,), self.cell(nodes))

    def cell(self, nodes):
        """GRUCell(mlp(raw_last[nodes]), memory[nodes]) (message_function.compute_message, memory_updater)."""
        p = self.p
        raw = self.msg_raw[nodes]
        msg = F.linear(F.relu(F.linear(raw, p["message_function.mlp.0.weight"], p["message_function.mlp.0.bias"])),
                       p["message_function.mlp.2.weight"], p["message_function.mlp.2.bias"])
        h = self.memory[nodes]
        u = "memory_updater.memory_updater."
        # nn.GRUCell's own kernel (r, z gates, n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h)
        return torch._VF.gru_cell(msg, h, p[u + "weight_ih"], p[u + "weight_hh"], p[u + "bias_ih"], p[u + "bias_hh"])

    # -------------------------------------------------------------- embedding
    def layer(self, li, src_feat, ngh_feat, edge, tfeat, mask, akeep, fkeep, scale):
        """TemporalAttentionLayer.forward -> MultiHeadAttention.forward -> ScaledDotProductAttention.forward."""
        p, H = self.p, self.H
        pre = f"embedding_module.attention_models.{li}."
        mh = pre + "multi_head_target."
        R, N = mask.shape
        cosb = torch.cos(p["time_encoder.w.bias"])            # time_encoder(zeros): cos(0 * w + b)
        q = torch.cat([src_feat, cosb.expand(R, -1)], dim=1).unsqueeze(1)                  # [R, 1, dq]
        k = torch.cat([ngh_feat, edge, tfeat], dim=2)                                      # [R, N, dk]
        dk = k.shape[2]
        residual = q
        qp = F.linear(q, p[mh + "w_qs.weight"]).view(R, 1, 1, H, dk)
        kp = F.linear(k, p[mh + "w_ks.weight"]).view(R, 1, N, H, dk)
        vp = F.linear(k, p[mh + "w_vs.weight"]).view(R, 1, N, H, dk)
        qp = qp.transpose(2, 3).contiguous().view(R * H, 1, dk)
        kp = kp.transpose(2, 3).contiguous().view(R * H, N, dk)
        vp = vp.transpose(2, 3).contiguous().view(R * H, N, dk)
        mask_r = mask.unsqueeze(1).repeat(H, 1, 1)                                        # head-major pairing
        attn = torch.bmm(qp, kp.transpose(-1, -2)) / float(np.power(dk, 0.5))
        attn = torch.softmax(attn.masked_fill(mask_r, -1e10), dim=2)
        if akeep is not None:
            attn = attn * (akeep.reshape(R * H, 1, N).to(attn.dtype) * scale)              # attention dropout
        out = torch.bmm(attn, vp).view(R, 1, H * dk)
        out = F.linear(out, p[mh + "fc.weight"], p[mh + "fc.bias"])
        if fkeep is not None:
            out = out * (fkeep.reshape(R, 1, -1).to(out.dtype) * scale)                    # dropout on fc(output)
        out = F.layer_norm(out + residual, (out.shape[2],), p[mh + "layer_norm.weight"], p[mh + "layer_norm.bias"],
                           1e-5).squeeze(1)
        x = torch.cat([out, src_feat], dim=1)
        h = F.relu(F.linear(x, p[pre + "merger.fc1.weight"], p[pre + "merger.fc1.bias"]))
        return F.linear(h, p[pre + "merger.fc2.weight"], p[pre + "merger.fc2.bias"])

    def embed(self, M, batch, keep=None, scale=1.0):
        src, dst, fake, ts, _, sgs = batch[0], batch[1], batch[2], batch[3], batch[4], batch[5:8]
        dt_, dev = self.dtype, self.device
        n0 = torch.cat([_t(x, torch.long, dev).reshape(-1) for x in (src, dst, fake)])
        R1 = len(n0)

        def cat(i, h, dtype):
            return torch.cat([_t(sg[i][h], dtype, dev) for sg in sgs])
        n1 = cat(0, 0, torch.long)
        N = n1.shape[1]
        n2 = cat(0, 1, torch.long).reshape(R1 * N, N)
        e1, e2 = cat(1, 0, torch.long), cat(1, 1, torch.long).reshape(R1 * N, N)
        t1, t2 = cat(2, 0, torch.float64), cat(2, 1, torch.float64).reshape(R1, N, N)
        cut = _t(ts, torch.float64, dev).reshape(-1).repeat(3)
        dt1 = (cut.view(R1, 1) - t1).float()
        dt2 = (t1.view(R1, N, 1) - t2).float().reshape(R1 * N, N)
        tab = M + self.nf
        w, b = self.p["time_encoder.w.weight"].reshape(-1), self.p["time_encoder.w.bias"]
        keep = keep if keep is not None else [None] * 4
        y0 = self.layer(0, tab[n1.reshape(-1)], tab[n2], self.ef[e2], self.time(dt2, w, b), n2 == 0,
                        keep[0], keep[2], scale)
        return self.layer(1, tab[n0], y0.view(R1, N, -1), self.ef[e1], self.time(dt1, w, b),
                          n1 == 0, keep[1], keep[3], scale).to(dt_)

    # -------------------------------------------------------------- one stateful contrast
    def step(self, batch, keep=None, scale=1.0):
        """contrast with forbidden_memory_update=False -> (pos, neg) [B, 1]; the state moves on."""
        p = self.p
        src, dst, ts, e_idx = (np.asarray(batch[i]) for i in (0, 1, 3, 4))
        B = len(src)
        M = self.updated_memory()
        emb = self.embed(M, batch, keep, scale)
        s, d, n = emb[:B], emb[B:2 * B], emb[2 * B:]
        x = torch.cat([torch.cat([s, s]), torch.cat([d, n])], dim=1)
        score = F.linear(F.relu(F.linear(x, p["affinity_score.fc1.weight"], p["affinity_score.fc1.bias"])),
                         p["affinity_score.fc2.weight"], p["affinity_score.fc2.bias"])
        with torch.no_grad():
            self._advance(s.detach(), d.detach(), src, dst, ts, e_idx)
        return score[:B], score[B:]

    def frozen(self, batch):
        """contrast with forbidden_memory_update=True on the current state -> (pos, neg); nothing moves."""
        p = self.p
        B = len(batch[0])
        with torch.no_grad():
            emb = self.embed(self.updated_memory(), batch)
            s, d, n = emb[:B], emb[B:2 * B], emb[2 * B:]
            x = torch.cat([torch.cat([s, s]), torch.cat([d, n])], dim=1)
            score = F.linear(F.relu(F.linear(x, p["affinity_score.fc1.weight"], p["affinity_score.fc1.bias"])),
                             p["affinity_score.fc2.weight"], p["affinity_score.fc2.bias"])
        return score[:B], score[B:]

    def _advance(self, s, d, src, dst, ts, e_idx):
        dev = self.device
        src_t, dst_t = _t(src, torch.long, dev), _t(dst, torch.long, dev)
        positives = torch.unique(torch.cat([src_t, dst_t]))
        had = positives[self.msg_flag[positives]]
        # update_memory(positives): the cell once more, over the positives alone as the reference runs it (the
        # updated table's rows up to the rounding of another GEMM shape); last_update takes the applied message's
        # timestamp
        if len(had):
            self.memory[had] = self.cell(had)
            self.last_update[had] = self.msg_ts[had]
        self.msg_flag[positives] = False                                   # clear_messages(positives)
        ts32 = _t(ts, torch.float64, dev).float()                          # torch.from_numpy(edge_times).float()
        ef = self.ef[_t(e_idx, torch.long, dev)]
        w, b = self.p["time_encoder.w.weight"].detach().reshape(-1), self.p["time_encoder.w.bias"].detach()
        src_msg = torch.cat([s, d, ef, self.time(ts32 - self.last_update[src_t], w, b)], dim=1)
        dst_msg = torch.cat([d, s, ef, self.time(ts32 - self.last_update[dst_t], w, b)], dim=1)
        # all source-role messages in batch order, then all destination-role ones; the ``last`` aggregator reads
        # a node's last one: the entry with the largest index in [src | dst], found on the host
        order = np.concatenate([src, dst]).astype(np.int64)
        nodes, first_rev = np.unique(order[::-1], return_index=True)
        last = _t(len(order) - 1 - first_rev, torch.long, dev)
        nodes = _t(nodes, torch.long, dev)
        self.msg_raw[nodes] = torch.cat([src_msg, dst_msg])[last]
        self.msg_ts[nodes] = torch.cat([ts32, ts32])[last]
        self.msg_flag[nodes] = True


def bce(pos, neg):
    crit = F.binary_cross_entropy_with_logits
    return crit(pos, torch.ones_like(pos)) + crit(neg, torch.zeros_like(neg))


def train_steps(model, batches, keeps=None, scale=1.0):
    """Per batch: zero_grad, step, the loss of learn_base.py:233-235, backward (no optimizer step; the state is
    detached by construction).  -> list of (loss, pos, neg, {name: grad or None})."""
    out = []
    for i, batch in enumerate(batches):
        model.zero_grad()
        pos, neg = model.step(batch, None if keeps is None else keeps[i], scale)
        loss = bce(pos, neg)
        loss.backward()
        out.append((loss.detach(), pos.detach(), neg.detach(),
                    {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in model.trainable().items()}))
    return out


# ------------------------------------------------------------------ one attention pass in closed form (fp64)
def pair_rows(Rr, H, seg):
    """Mask / weight row of pair (r, h): base + ((r - base) H + h) % seg inside the row's segment."""
    seg = seg or Rr
    r = torch.arange(Rr).view(Rr, 1)
    h = torch.arange(H).view(1, H)
    base = r - r % seg
    return base + ((r - base) * H + h) % seg


def time_arg(dt, tw, tb):
    """u = fma(dt, w, b) in fp32, as the kernel's key build forms it -> fp64 [..., d_time]."""
    return (dt.double().unsqueeze(-1) * tw.double() + tb.double()).float().double()


def attn_closed_form(x, keep, scale):
    """x: node [R, N, dn] (the rows the keys read), edge [R, N, de], dt [R, N], tw / tb [d_time], qf / gz [R, H, dk],
    mask [R, N], ew [R, N] or None, T, seg; node_idx [R, N] and node_rows when the node table is gathered.  keep:
    uint8 [R H N] or None.  Returns z, d_ew [R, H, N], d_node [R, N, dn], d_qf, d_time [2, d_time], the magnitude
    sums d_time's bound is taken from, the per-(slot, head) scalars a and b, and d_tab [node_rows, dn] (the slots'
    d_node rows added per table row) when gathered."""
    Rr, N, dn = x.node.shape
    de, H = x.edge.shape[2], x.qf.shape[1]
    u = time_arg(x.dt, x.tw, x.tb)
    key = torch.cat([x.node.double(), x.edge.double(), torch.cos(u)], dim=-1)
    m = pair_rows(Rr, H, x.seg)
    qf, gz = x.qf.double(), x.gz.double()
    s = torch.einsum("rhc,rjc->rhj", qf, key) / x.T
    masked = x.mask[m] == 0
    p = torch.softmax(s.masked_fill(masked, -1e10), dim=-1)
    kf = torch.ones(Rr, H, N, dtype=torch.float64) if keep is None else keep.view(Rr, H, N).double() * scale
    e = kf if x.ew is None else x.ew.double()[m] * kf
    z = torch.einsum("rhj,rjc->rhc", p * e, key)
    c = torch.einsum("rhc,rjc->rhj", gz, key)
    S = (p * e * c).sum(-1, keepdim=True)
    live = (~masked).double()
    ds = p * (e * c - S) * live
    a, b = p * e, ds / x.T
    dk = torch.einsum("rhj,rhc->rjc", a, gz) + torch.einsum("rhj,rhc->rjc", b, qf)
    d_qf = torch.einsum("rhj,rjc->rhc", ds, key) / x.T
    sin_u = -torch.sin(u)
    dkt = dk[..., dn + de:]
    d_time = torch.stack([(sin_u * x.dt.double().unsqueeze(-1) * dkt).sum((0, 1)), (sin_u * dkt).sum((0, 1))])
    cabs = torch.einsum("rhc,rjc->rhj", gz.abs(), key.abs())
    Sabs = (p * e.abs() * cabs).sum(-1, keepdim=True)
    mag = torch.einsum("rhj,rhc->rjc", p * e.abs(), gz.abs()) + \
        torch.einsum("rhj,rhc->rjc", p * (e.abs() * cabs + Sabs) * live / x.T, qf.abs())
    magt = mag[..., dn + de:]
    mag_time = torch.stack([(x.dt.double().abs().unsqueeze(-1) * magt).sum((0, 1)), magt.sum((0, 1))])
    out = SimpleNamespace(z=z, d_ew=p * c * kf, d_node=dk[..., :dn], d_qf=d_qf, d_time=d_time, mag_time=mag_time,
                          a=a.transpose(1, 2), b=b.transpose(1, 2), d_tab=None)
    if getattr(x, "node_idx", None) is not None:
        out.d_tab = torch.zeros(x.node_rows, dn, dtype=torch.float64).index_add_(
            0, x.node_idx.reshape(-1).long(), out.d_node.reshape(-1, dn))
    return out
