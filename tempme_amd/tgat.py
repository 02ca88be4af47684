"""Drop-in base ``TGAT`` (TGAT/TGAT.py) for the consumer side of the explanation path.

With ``--base_type tgat`` TempME's loops hand per-side explanation weights to the frozen base model:
``base_model.contrast(src, dst, fake, ts, e_idx, sg_src, sg_tgt, sg_bgd, test=True, if_explain=True,
exp_weights=[[imp_src, imp_tgt], [imp_src, imp_bgd]])`` (temp_exp_main.py:609-616), every ``imp`` a
``(hop-1 [B, N], hop-2 [B, N^2])`` pair.  This module keeps the reference's constructor, parameter names
(a reference ``state_dict`` loads as is), construction order (``torch.manual_seed(s); TGAT(...)`` draws the
reference's initial weights) and the ``contrast`` / ``get_node_emb`` / ``grab_subgraph`` signatures.

What the reference computes per side with ``num_layers = 2`` (forward_msg :607-619):
  1. ``attn_model_list[0]``: the B roots over their raw hop-1 neighbours, weights exp[0]      -> h0'
  2. ``attn_model_list[0]``: the B*N hop-1 nodes over their raw hop-2 neighbours, weights exp[1] -> h1'
  3. ``attn_model_list[1]``: h0' over h1' (dense), hop-1 edge and time features, weights exp[0] again.
The query of a pass is ``[src | 0 (d_edge) | src_t]`` with src_t = TimeEncode(0) for roots and
TimeEncode(cut - t1) for the hop-1 rows of pass 2.

Here every pass is one launch of the attention forward (csrc/attn_kernels.h, shared with TGN, in its TGAT
instances; C ABI ``tm_tgat_attn_fwd``, autograd wrapper ``attn_op.AttnFn``) over the rows of all sides,
the sides being segments of ``seg_rows`` = B (or B*N) rows so the reference's head-major mask / weight
pairing stays inside one forward_msg call.  The per-neighbour projections fold into per-row ones
(qf = W_k^T W_q query before the kernel, G = fc W_v after it, as tgn.py).  The layer tail (G z + residual,
LayerNorm, the two-branch MergeLayer) runs as torch ops on the device (differentiable); with
``model.fused_tail = True`` a contrast that needs no gradient runs it as one fused fp32-MFMA kernel
(``tm_tgat_merge_fwd``) instead, which is built and tested but slower at the metric's shape, so off by default.  Gradients reach the explanation weights of all
three passes: ``tm_tgat_attn_bwd`` returns d ew, the gradient of the dense neighbour table (h1') and the
gradient of the folded query (through h0').  On these paths the base model is frozen: its parameters get no .grad.

For the explainer's drivers (train.py, evaluate.py) ``prepare_contrast`` builds the inputs a contrast derives from
its batch once (``contrast(..., prepared=...)`` shares them between the original and the explained contrast of a step)
and ``contrast(..., stacked_weights=(hop-1 [3B, N], hop-2 [3B, N^2]))`` takes the three sides' weights as the two
tensors ``explain_groups`` returns: ``exp_weights=[[s, t], [s, b]]`` of their views without a split and a cat.

Training the base itself (learn_base.py) is opt-in: after ``model.train_on_hip()``, ``model.train()`` calls of
``contrast(..., if_explain=False)`` / ``get_node_emb`` with gradients enabled run ``tm_tgat_attn_train_fwd`` /
``tm_tgat_attn_train_bwd`` (csrc/attn_train.h, ``attn_op.TrainAttnFn``): the attention dropout as a keep mask
inside the kernels, fc's dropout in the torch tail, P = W_k^T W_q and G = fc W_v folded in fp32 from the live
parameters under autograd (so d qf and d z reach w_qs, w_ks, w_vs and fc), the query-side time features as
differentiable torch ops and the key-side time gradient from the kernel's d_time.  ``loss.backward()`` then fills
.grad on all 36 trainable parameters.

The layer around the op is attn_layer.py's, shared with tgn.py (``fold``: this module multiplies by contiguous
P^T / G^T -- the packs transpose the fp64 pair, the training step asks for the transposed products).  TGAT's own: the
two-branch merger with its optional fused ``merge_fwd``, the time features ``cos(dt * freq + phase)`` (two roundings),
``keep_mask_shapes`` and the query cache of ``prepare_contrast``.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import attn_layer as AL
from .attn_op import AttnFn, TrainAttnFn, attn_probs


# ------------------------------------------------------------------ modules (parameter layout)
class MergeLayer(nn.Module):
    """TGAT.py:9-34: fc21(relu(fc11(x1))) + fc22(relu(fc12(x2)))."""

    def __init__(self, dim1, dim2, dim3, dim4, non_linear=True):
        super().__init__()
        self.fc11 = nn.Linear(dim1, dim3)
        self.fc12 = nn.Linear(dim2, dim3)
        self.fc21 = nn.Linear(dim3, dim4)
        self.fc22 = nn.Linear(dim3, dim4)
        self.act = nn.ReLU()
        nn.init.xavier_normal_(self.fc11.weight)
        nn.init.xavier_normal_(self.fc21.weight)
        nn.init.xavier_normal_(self.fc12.weight)
        nn.init.xavier_normal_(self.fc22.weight)

    def forward(self, x1, x2):
        return self.fc22(self.act(self.fc12(x2))) + self.fc21(self.act(self.fc11(x1)))


class MergeLayer_final(nn.Module):
    """TGAT.py:37-52: fc2(relu(fc1([x1 | x2])))."""

    def __init__(self, dim1, dim2, dim3, dim4):
        super().__init__()
        self.fc1 = nn.Linear(dim1 + dim2, dim3)
        self.fc2 = nn.Linear(dim3, dim4)
        self.act = nn.ReLU()
        nn.init.xavier_normal_(self.fc1.weight)
        nn.init.xavier_normal_(self.fc2.weight)

    def forward(self, x1, x2):
        return self.fc2(self.act(self.fc1(torch.cat([x1, x2], dim=1))))


class MultiHeadAttention(nn.Module):
    """Parameters of TGAT.py:83-107 (d_k = d_v = d_model // n_head, no projection bias)."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.1):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = nn.Linear(d_model, n_head * d_k, bias=False)
        self.w_ks = nn.Linear(d_model, n_head * d_k, bias=False)
        self.w_vs = nn.Linear(d_model, n_head * d_v, bias=False)
        nn.init.normal_(self.w_qs.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_k)))
        nn.init.normal_(self.w_ks.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_k)))
        nn.init.normal_(self.w_vs.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_v)))
        self.temperature = float(np.power(d_k, 0.5))
        self.layer_norm = nn.LayerNorm(d_model)
        self.fc = nn.Linear(n_head * d_v, d_model)
        nn.init.xavier_normal_(self.fc.weight)
        self.dropout = nn.Dropout(dropout)


class TimeEncode(nn.Module):
    """TGAT.py:220-241: cos(ts * basis_freq + phase), the multiply and the add rounded separately."""

    def __init__(self, expand_dim, factor=5):
        super().__init__()
        self.time_dim = expand_dim
        self.factor = factor
        self.basis_freq = nn.Parameter(torch.from_numpy(1 / 10 ** np.linspace(0, 9, self.time_dim)).float())
        self.phase = nn.Parameter(torch.zeros(self.time_dim).float())

    def forward(self, ts):
        map_ts = ts.unsqueeze(-1) * self.basis_freq.view(1, 1, -1)
        map_ts = map_ts + self.phase.view(1, 1, -1)
        return torch.cos(map_ts)


class AttnModel(nn.Module):
    """TGAT.py:317-360 (attn_mode 'prod')."""

    def __init__(self, feat_dim, edge_dim, time_dim, model_dim, attn_mode="prod", n_head=2, drop_out=0.1):
        super().__init__()
        self.feat_dim, self.edge_dim, self.time_dim, self.model_dim = feat_dim, edge_dim, time_dim, model_dim
        self.merger = MergeLayer(self.model_dim, feat_dim, feat_dim, feat_dim)
        assert self.model_dim % n_head == 0
        self.attn_mode = attn_mode
        self.multi_head_target = MultiHeadAttention(n_head, d_model=self.model_dim, d_k=self.model_dim // n_head,
                                                    d_v=self.model_dim // n_head, dropout=drop_out)


# ------------------------------------------------------------------ the layer tail (the attention op: attn_op.py)
def merge_fwd(z, query, lw, feat):
    """The fused layer tail (tm_tgat_merge_fwd) on a packed attention model ``lw`` -> [rows, feat]."""
    dev = z.device
    R, dk = query.shape
    m = L.TgatMerge()
    m.rows, m.n_head, m.d_key, m.feat = R, lw["H"], dk, feat
    z, query = z.contiguous(), query.contiguous()
    m.z, m.query = z.data_ptr(), query.data_ptr()
    for f, k in (("gt", "Gt"), ("fc_b", "fcb"), ("ln_w", "lnw"), ("ln_b", "lnb"), ("w11t", "w11t"), ("b11", "b11"),
                 ("w12t", "w12t"), ("b12", "b12"), ("w21t", "w21t"), ("b21", "b21"), ("w22t", "w22t"), ("b22", "b22")):
        setattr(m, f, lw[k].data_ptr())
    out = torch.empty((R, feat), dtype=torch.float32, device=dev)
    L.check(L.lib().tm_tgat_merge_fwd(L.C.byref(m), L.ptr(out), L.stream_ptr(dev)), "TGAT layer tail")
    return out


def merge_torch(z, query, lw, feat):
    """The same tail as torch ops (differentiable; the reference's order of operations)."""
    h = AL.mha_tail(z, query, lw["Gt"], lw["fcb"], lw["lnw"], lw["lnb"])
    x1 = torch.addmm(lw["b21"], F.relu(torch.addmm(lw["b11"], h, lw["w11t"])), lw["w21t"])
    x2 = torch.addmm(lw["b22"], F.relu(torch.addmm(lw["b12"], query[:, :feat], lw["w12t"])), lw["w22t"])
    return x2 + x1


def pack_attn_model(am, dev):
    """Folded, device-resident weights of one AttnModel: P = W_k^T W_q and G = fc W_v per head, folded in
    fp64 and stored in fp32; the tail's matrices transposed ([in][out]) as tm_tgat_merge_fwd reads them."""
    f32 = torch.float32
    mh, mg = am.multi_head_target, am.merger
    P, G = AL.fold(mh, torch.float64, dev)           # qf = P query [H*dm], fc(...) = G z
    H, dm = mh.n_head, P.shape[1]

    def t(lin):
        return lin.weight.detach().to(dev, f32).t().contiguous()

    def b(lin):
        return lin.bias.detach().to(dev, f32).contiguous()
    return dict(Pt=P.t().to(f32).contiguous(), Gt=G.t().to(f32).contiguous(), fcb=b(mh.fc),
                lnw=mh.layer_norm.weight.detach().to(dev, f32).contiguous(),
                lnb=mh.layer_norm.bias.detach().to(dev, f32).contiguous(),
                w11t=t(mg.fc11), b11=b(mg.fc11), w12t=t(mg.fc12), b12=b(mg.fc12),
                w21t=t(mg.fc21), b21=b(mg.fc21), w22t=t(mg.fc22), b22=b(mg.fc22),
                H=H, dk=dm, temperature=mh.temperature)


# ------------------------------------------------------------------ the model
class TGAT(AL.HipTraining, nn.Module):
    """TGAT/TGAT.py:389-423 constructor (same arguments, parameter names and initialisation order).

    ``train_on_hip()`` (attn_layer.HipTraining) opts in to the HIP training step: ``train()`` calls of contrast /
    get_node_emb with gradients enabled and ``if_explain`` false run tm_tgat_attn_train_fwd /
    tm_tgat_attn_train_bwd, and ``loss.backward()`` fills ``.grad`` on all 36 trainable parameters."""
    _label = "TGAT"
    _param_error = "TGAT.train_on_hip: parameters must be contiguous fp32 on the HIP device"

    def __init__(self, n_feat, e_feat, num_neighbors, attn_mode="prod", use_time="time", attn_agg_method="attn",
                 num_layers=3, n_head=4, drop_out=0.1, verbosity=1):
        super().__init__()
        if attn_agg_method != "attn":
            raise NotImplementedError(f"attn_agg_method {attn_agg_method!r}: only 'attn' is built (the LSTM and "
                                      "mean pools ignore the explanation weights)")
        if attn_mode != "prod":
            raise NotImplementedError(f"attn_mode {attn_mode!r}: only 'prod' is built (the map-based attention "
                                      "takes no explanation weight in the reference)")
        if use_time != "time":
            raise NotImplementedError(f"use_time {use_time!r}: only the harmonic 'time' encoder is built")
        if num_layers != 2:
            raise NotImplementedError(f"num_layers {num_layers}: the explanation path samples 2-hop subgraphs, "
                                      "so only num_layers=2 is built")
        if n_head > 4:
            raise NotImplementedError(f"n_head {n_head}: the attention kernels hold at most 4 heads")
        self.verbosity = verbosity
        self.num_neighbors, self.num_layers = num_neighbors, num_layers
        self.ngh_finder = None
        self.n_feat_th = nn.Parameter(torch.from_numpy(np.asarray(n_feat).astype(np.float32)), requires_grad=False)
        self.e_feat_th = nn.Parameter(torch.from_numpy(np.asarray(e_feat).astype(np.float32)), requires_grad=False)
        self.feat_dim = self.n_feat_th.shape[1]
        self.e_feat_dim = self.e_feat_th.shape[1]
        self.time_dim = self.feat_dim
        self.model_dim = self.feat_dim + self.e_feat_dim + self.time_dim
        if self.model_dim > 576:
            raise NotImplementedError(f"model_dim {self.model_dim}: the attention kernels hold keys of at most 576")
        self.dropout_p = drop_out
        self.edge_raw_embed = nn.Embedding.from_pretrained(self.e_feat_th, padding_idx=0, freeze=True)
        self.node_raw_embed = nn.Embedding.from_pretrained(self.n_feat_th, padding_idx=0, freeze=True)
        self.time_encoder = TimeEncode(expand_dim=self.time_dim)
        self.attn_model_list = nn.ModuleList([AttnModel(self.feat_dim, self.e_feat_dim, self.time_dim, self.model_dim,
                                                        attn_mode=attn_mode, n_head=n_head, drop_out=drop_out)
                                              for _ in range(self.num_layers)])
        self.affinity_score = MergeLayer_final(self.feat_dim, self.feat_dim, self.feat_dim, 1)
        # the reference pairs attention rows with mask / explanation rows head-major through
        # .repeat(n_head, 1, 1) (TGAT.py:128-130); False pairs row r with row r
        self.head_major_rows = True
        # the layer tail of a contrast that needs no gradient: True = the fused MFMA kernel (tm_tgat_merge_fwd),
        # False = the torch ops.  The torch ops are the default: at the metric's shape the fused kernel measured
        # 0.51 ms against 0.15 ms for the 6,000-row pass (DESIGN.md "TGAT contrast")
        self.fused_tail = False
        self._pack_cache = None
        self._pack_key = None

    # -------------------------------------------------------------- device pack
    def _dev(self):
        p = self.n_feat_th
        return L.require_device(p.device if p.device.type == "cuda" else None)

    def _pack(self):
        """Device-resident tables and folded per-model weights, rebuilt when a parameter changes."""
        dev = self._dev()
        key = (dev, tuple((t.data_ptr(), t._version) for t in self.parameters()))
        if self._pack_cache is not None and self._pack_key == key:
            return self._pack_cache
        f32 = torch.float32
        with torch.no_grad():
            freq = self.time_encoder.basis_freq.detach().to(dev, f32).contiguous()
            phase = self.time_encoder.phase.detach().to(dev, f32).contiguous()
            aff = self.affinity_score
            pack = dict(dev=dev, tab=self.n_feat_th.detach().to(dev, f32).contiguous(),
                        etab=self.e_feat_th.detach().to(dev, f32).contiguous(), freq=freq, phase=phase,
                        t0=torch.cos(torch.zeros_like(freq) * freq + phase),      # TimeEncode(0)
                        models=[pack_attn_model(am, dev) for am in self.attn_model_list],
                        a1w=aff.fc1.weight.detach().to(dev, f32), a1b=aff.fc1.bias.detach().to(dev, f32),
                        a2w=aff.fc2.weight.detach().to(dev, f32), a2b=aff.fc2.bias.detach().to(dev, f32),
                        err=torch.zeros(1, dtype=torch.int32, device=dev))
        self._pack_cache, self._pack_key = pack, key
        return pack

    # -------------------------------------------------------------- forward pieces
    def _query(self, lw, src, src_t, R):
        """The query rows [src | 0 (d_edge) | src_t] of a pass and their folded projection."""
        query = torch.cat([src, src.new_zeros((R, self.e_feat_dim)), src_t], dim=1)      # [R, dk]
        return query, (query @ lw["Pt"]).contiguous()                                    # [R, H*dk]

    def _attn_pass(self, pk, mi, src, src_t, R, N, node_idx, ngh_dense, edge_idx, dt, mask_node, ew, seg, q=None,
                   tap=None):
        """One AttnModel.forward (TGAT.py:362-386) over R source rows -> [R, feat]; ``q``: ``_query``'s pair
        for these rows when it is already built.  ``tap`` (a list, ``attention_weights``): the pass's attention
        probabilities and their head mean are appended to it, from one more launch on the forward's descriptor."""
        lw = pk["models"][mi]
        H, dk, fd = lw["H"], lw["dk"], self.feat_dim
        query, qf = q if q is not None else self._query(lw, src, src_t, R)
        spec = AL.attn_spec("tgat", R, N, H, dk, fd, self.time_dim, lw["temperature"], self.head_major_rows, seg,
                            node_tab=pk["tab"], node_idx=node_idx, edge_tab=pk["etab"], edge_idx=edge_idx, dt=dt,
                            time_w=pk["freq"], time_b=pk["phase"], mask_node=mask_node, err=pk["err"])
        if tap is not None:
            tap.append(attn_probs(spec, qf, ngh_dense))
        z = AttnFn.apply(qf, ngh_dense, ew, spec)
        if self.fused_tail and not (torch.is_grad_enabled() and (z.requires_grad or query.requires_grad)):
            return merge_fwd(z, query, lw, fd)
        return merge_torch(z, query, lw, fd)

    def _check_mode(self, weights=None):
        if weights is None and self._train_hip_ok():
            return
        if self.training and self.dropout_p > 0:
            raise NotImplementedError("TGAT in training mode with drop_out > 0: the attention and fc dropout of "
                                      "the reference are not built (the frozen base model runs in eval mode)")

    def node_embeddings(self, nodes, eids, times, cut_time, explain_weights=None, n_segments=1):
        """forward_msg (TGAT.py:607-619) for stacked calls: nodes = [n0 [R], n1 [R, N], n2 [R, N^2]],
        eids / times = [hop-1, hop-2], explain_weights = (hop-1 [R, N], hop-2 [R, N^2]) or None -> [R, feat].
        The R rows are ``n_segments`` independent forward_msg calls of R / n_segments rows each (the sides
        of a contrast, times the ratios of a threshold_test): every row gives the same result as in its own
        call, the head-major pairing stays inside its segment.  cut_time: one time per row, or per row of
        one segment (repeated)."""
        return self._embed(self._prep_inputs(nodes, eids, times, cut_time, n_segments), explain_weights)

    def _prep_inputs(self, nodes, eids, times, cut_time, n_segments=1):
        """What node_embeddings derives from its inputs before any weight is read: the node, edge-id and time
        tensors on the device in the kernels' dtypes and the two time offsets (a dict)."""
        return AL.prep_inputs(self._dev(), nodes, eids, times, cut_time, n_segments)

    def _embed(self, x, explain_weights=None, tap=None):
        """The three passes of node_embeddings on ``_prep_inputs``' dict ``x``.  ``tap``: ``_attn_pass``'s, filled by
        pass 2 and then pass 3 (the frozen model only: ``attention_weights`` runs under no_grad)."""
        train = explain_weights is None and self._train_hip_ok()
        self._check_mode(explain_weights)
        R, N, seg = x["R"], x["N"], x["seg"]
        n0, n1, n2, e1, e2, dt1, dt2 = (x[k] for k in ("n0", "n1", "n2", "e1", "e2", "dt1", "dt2"))
        if train:
            return self._embed_train(x["dev"], R, N, seg, n0, n1, n2, e1, e2, dt1, dt2)
        pk = self._pack()
        dev = pk["dev"]
        ew1 = ew2 = None
        if explain_weights is not None:
            ew1 = explain_weights[0].to(dev, torch.float32).reshape(R, N).contiguous()
            ew2 = explain_weights[1].to(dev, torch.float32).reshape(R * N, N).contiguous()
        tab, freq, phase = pk["tab"], pk["freq"], pk["phase"]
        t_root = pk["t0"].expand(R, -1)
        # the queries of passes 1 and 2 depend on the batch and the frozen pack only: prepare_contrast's dict
        # keeps them, so the contrasts that share it (without and with weights) fold them once
        cache = x.get("cache")
        if cache is not None and cache.get("pack") is pk:
            q0, q1 = cache["q"]
        else:
            t_hop1 = torch.cos(dt1.reshape(-1, 1) * freq + phase)         # two roundings (mul, then add)
            lw = pk["models"][0]
            q0 = self._query(lw, tab[n0], t_root, R)
            q1 = self._query(lw, tab[n1.long()], t_hop1, R * N)
            if cache is not None:
                cache["pack"], cache["q"] = pk, (q0, q1)
        h0 = self._attn_pass(pk, 0, None, None, R, N, n1, None, e1, dt1, n1, ew1, seg, q0)
        h1 = self._attn_pass(pk, 0, None, None, R * N, N, n2, None, e2, dt2, n2, ew2, seg * N, q1, tap)
        return self._attn_pass(pk, 1, h0, t_root, R, N, None, h1.contiguous(), e1, dt1, n1, ew1, seg, None, tap)

    # -------------------------------------------------------------- HIP training path (tm_tgat_attn_train_*)
    def keep_mask_shapes(self, R, N):
        """Shapes of one step's six keep masks for R stacked rows: the attention masks of the three passes
        (flat, the byte of (row, head, neighbour) at (row H + head) N + neighbour: the reference's dropped tensor
        [B*N_src*n_head, 1, N]) and the masks of fc's dropout on fc(out), [rows, model_dim]."""
        H, dm = self.attn_model_list[0].multi_head_target.n_head, self.model_dim
        return [(R * H * N,), (R * N * H * N,), (R * H * N,), (R, dm), (R * N, dm), (R, dm)]

    def draw_keep_masks(self, R, N, generator=None):
        """One step's keep masks (uint8, 1 = kept with probability 1 - drop_out) for R stacked rows, drawn on
        the device in one allocation: [attn pass 1, attn pass 2, attn pass 3, fc pass 1, fc pass 2, fc pass 3]."""
        return AL.draw_keep_masks(self.keep_mask_shapes(R, N), self.dropout_p, self._dev(), generator)

    def _train_pass(self, am, folded, src, src_t, R, N, node_idx, ngh_dense, edge_idx, dt, mask_node, seg, akeep,
                    fkeep, scale):
        """_attn_pass on the live parameters with both dropouts -> [R, feat]."""
        mh = am.multi_head_target
        Pt, Gt = folded
        te = self.time_encoder
        query = torch.cat([src, src.new_zeros((R, self.e_feat_dim)), src_t], dim=1)
        qf = (query @ Pt).contiguous()
        spec = AL.attn_spec("tgat", R, N, mh.n_head, self.model_dim, self.feat_dim, self.time_dim, mh.temperature,
                            self.head_major_rows, seg, node_tab=self.n_feat_th, node_idx=node_idx,
                            edge_tab=self.e_feat_th, edge_idx=edge_idx, dt=dt, mask_node=mask_node, err=self._train_err)
        z = TrainAttnFn.apply(qf, ngh_dense, None, te.basis_freq, te.phase, spec, akeep, scale)
        # fc's dropout: TGAT.py:134
        h = AL.mha_tail(z, query, Gt, mh.fc.bias, mh.layer_norm.weight, mh.layer_norm.bias, fkeep, scale)
        return am.merger(h, query[:, :self.feat_dim])

    def _embed_train(self, dev, R, N, seg, n0, n1, n2, e1, e2, dt1, dt2):
        """The three passes of node_embeddings on the HIP training path (no explanation weights)."""
        te = self.time_encoder
        self._live_state(dev)
        keep, scale = AL.step_keep_masks(
            getattr(self, "tgat_keep_masks", None), self.keep_mask_shapes(R, N), float(self.dropout_p), dev,
            "TGAT.tgat_keep_masks: expected draw_keep_masks(R, N)'s six uint8 masks on the device")
        tab = self.n_feat_th
        freq, phase = te.basis_freq, te.phase
        t_root = torch.cos(torch.zeros_like(freq) * freq + phase).expand(R, -1)          # TimeEncode(0)
        t_hop1 = torch.cos(dt1.reshape(-1, 1) * freq + phase)                           # two roundings (mul, then add)
        am0, am1 = self.attn_model_list
        # contiguous Pt [dm, H dm] / Gt [H dm, dm], as the pack's: folded in fp32 from the live parameters
        f0, f1 = (AL.fold(am.multi_head_target, transposed=True) for am in (am0, am1))
        h0 = self._train_pass(am0, f0, tab[n0], t_root, R, N, n1, None, e1, dt1, n1, seg, keep[0], keep[3], scale)
        h1 = self._train_pass(am0, f0, tab[n1.long()], t_hop1, R * N, N, n2, None, e2, dt2, n2, seg * N,
                              keep[1], keep[4], scale)
        out = self._train_pass(am1, f1, h0, t_root, R, N, None, h1.contiguous(), e1, dt1, n1, seg, keep[2], keep[5],
                               scale)
        self._tgat_train_key = (R, N, keep[0] is not None)   # marker: the HIP training path ran
        return out

    def _sides(self, roots, subgraphs, weights, cut_time):
        """Stack the sides of a contrast into one node_embeddings call -> list of [B, feat]."""
        self._check_mode(weights)
        dev = self._dev()
        S = len(roots)
        n0, nodes, eids, times = AL.stack_sides(dev, roots, subgraphs)
        ew = None
        if weights is not None:
            ew = [torch.cat([w[h].to(dev, torch.float32) for w in weights]) for h in (0, 1)]
        emb = self.node_embeddings([n0] + nodes, eids, times, cut_time, ew, n_segments=S)
        B = emb.shape[0] // S
        return list(emb.split(B)) if B > 0 else [emb[:0]] * S

    def prepare_contrast(self, src_idx_l, tgt_idx_l, bgd_idx_l, cut_time_l, subgraph_src, subgraph_tgt, subgraph_bgd):
        """The inputs contrast derives from its batch (the three sides' roots and subgraphs concatenated in the
        kernels' dtypes, the time offsets), built once: the training step's two contrasts of the same batch
        (without and with explanation weights, temp_exp_main.py:597, :611) share them through
        ``contrast(..., prepared=...)``.  The dict also keeps the queries of the first two passes once a contrast
        has folded them (they depend on the batch and the frozen weights only)."""
        n0, nodes, eids, times = AL.stack_sides(self._dev(), (src_idx_l, tgt_idx_l, bgd_idx_l),
                                                (subgraph_src, subgraph_tgt, subgraph_bgd))
        x = self._prep_inputs([n0] + nodes, eids, times, cut_time_l, n_segments=3)
        x["cache"] = {}
        return x

    # -------------------------------------------------------------- reference API
    def affinity(self, x1, x2):
        return AL.affinity(self._pack(), x1, x2)

    def attention_weights(self, src_idx_l, tgt_idx_l, bgd_idx_l, cut_time_l, subgraph_src, subgraph_tgt, subgraph_bgd,
                          prepared=None, head_mean=False):
        """The attention probabilities of the contrast without explanation weights, as the reference's attention
        modules return them: (hop-1 [3B, H, N], hop-2 [3B N, H, N]) fp32 device tensors, rows in the order src, tgt,
        bgd.  Hop-1 is the third pass, the roots over the hop-1 embeddings (attn_model_list[1]); hop-2 is the second
        pass, the hop-1 nodes over their hop-2 neighbours.  The frozen embedding pass runs once (the hop-1 keys are the
        first layer's output) with one ``tm_tgat_attn_probs`` launch on the descriptor of each of the two passes.  A
        padded slot carries whatever the softmax gives it (a fully padded row is uniform);
        ``baselines.attention_explanation`` zeroes them.  ``head_mean``: the means over the heads instead,
        (hop-1 [3B, N], hop-2 [3B N, N]).  ``prepared``: prepare_contrast's output for these inputs.  No gradient;
        in train() mode with drop_out > 0 it raises like every frozen call."""
        with torch.no_grad():
            x = prepared if prepared is not None else self.prepare_contrast(
                src_idx_l, tgt_idx_l, bgd_idx_l, cut_time_l, subgraph_src, subgraph_tgt, subgraph_bgd)
            tap = []
            self._embed(x, tap=tap)
        (p2, m2), (p1, m1) = tap
        return (m1, m2) if head_mean else (p1, p2)

    def _score3(self, emb, live):
        """(pos, neg) scores from the [3B, feat] embeddings of the segments src, tgt, bgd: [tgt; bgd] is emb's
        tail (no copy).  ``live``: score with the live parameters (the HIP training path)."""
        B = emb.shape[0] // 3
        s, tb = emb.split([B, 2 * B])
        score = (self.affinity_score if live else self.affinity)(torch.cat([s, s], dim=0), tb)
        return score[:B], score[B:]

    def contrast(self, src_idx_l, tgt_idx_l, bgd_idx_l, cut_time_l, e_idx_l, subgraph_src, subgraph_tgt, subgraph_bgd,
                 test=False, if_explain=False, exp_weights=None, prepared=None, stacked_weights=None):
        """TGAT.py:461-481 -> (pos_score [B, 1], neg_score [B, 1]).  The three (or four) forward_msg calls
        run as segments of one launch per pass; the src side runs once when both pairs carry the same src
        weights (the same objects, as temp_exp_main.py:613 builds them), twice otherwise.

        ``prepared``: ``prepare_contrast``'s output for these same inputs (optional; shared by the contrasts of
        one batch that run three segments).  ``stacked_weights=(hop-1 [3B, N], hop-2 [3B, N^2])``: the explanation
        weights of the sides src, tgt, bgd as two tensors (what ``explain_groups`` returns), i.e.
        ``exp_weights=[[s, t], [s, b]]`` of their per-side views without splitting and concatenating them;
        implies ``if_explain``."""
        roots = [src_idx_l, tgt_idx_l, bgd_idx_l]
        sgs = [subgraph_src, subgraph_tgt, subgraph_bgd]
        if stacked_weights is not None:
            if exp_weights is not None:
                raise ValueError("TGAT.contrast: give exp_weights or stacked_weights, not both")
            ew1, ew2 = stacked_weights
            x = prepared if prepared is not None else self.prepare_contrast(*roots, cut_time_l, *sgs)
            if ew1.shape[0] != x["R"] or ew2.shape[0] != x["R"]:
                raise ValueError(f"TGAT.contrast: stacked_weights need {x['R']} rows (src, tgt, bgd), got "
                                 f"{tuple(ew1.shape)} and {tuple(ew2.shape)}")
            return self._score3(self._embed(x, (ew1, ew2)), False)
        if not if_explain:
            if prepared is not None:
                return self._score3(self._embed(prepared), self._train_hip_ok())
            s, t, b = self._sides(roots, sgs, None, cut_time_l)
            s2 = s
        else:
            (w_s, w_t), (w_s2, w_b) = exp_weights[0], exp_weights[1]
            same = w_s is w_s2 or (len(w_s) == len(w_s2) and all(x is y for x, y in zip(w_s, w_s2)))
            if same and prepared is not None:
                dev = self._dev()
                ew = [torch.cat([w[h].to(dev, torch.float32) for w in (w_s, w_t, w_b)]) for h in (0, 1)]
                return self._score3(self._embed(prepared, ew), False)
            if same:
                s, t, b = self._sides(roots, sgs, [w_s, w_t, w_b], cut_time_l)
                s2 = s
            else:
                s, t, s2, b = self._sides([src_idx_l, tgt_idx_l, src_idx_l, bgd_idx_l],
                                          [subgraph_src, subgraph_tgt, subgraph_src, subgraph_bgd],
                                          [w_s, w_t, w_s2, w_b], cut_time_l)
        B = s.shape[0]
        if not if_explain and self._train_hip_ok():
            score = self.affinity_score(torch.cat([s, s2], dim=0), torch.cat([t, b], dim=0))   # the live parameters
        else:
            score = self.affinity(torch.cat([s, s2], dim=0), torch.cat([t, b], dim=0))
        return score[:B], score[B:]

    def get_node_emb(self, src_idx_l, tgt_idx_l, bgd_idx_l, cut_time_l, e_idx_l, subgraph_src, subgraph_tgt,
                     subgraph_bgd, test=False):
        """TGAT.py:507-519 -> (source, target, background) embeddings [B, feat] each."""
        return tuple(self._sides([src_idx_l, tgt_idx_l, bgd_idx_l], [subgraph_src, subgraph_tgt, subgraph_bgd], None,
                                 cut_time_l))

    def set_neighbor_sampler(self, neighbor_sampler):
        self.ngh_finder = neighbor_sampler

    def grab_subgraph(self, src_idx_l, cut_time_l, e_idx_l=None):
        """TGAT.py:603-605."""
        return self.ngh_finder.find_k_hop(self.num_layers, src_idx_l, cut_time_l, num_neighbors=self.num_neighbors,
                                          e_idx_l=e_idx_l)


__all__ = ["TGAT", "AttnModel", "MultiHeadAttention", "MergeLayer", "MergeLayer_final", "TimeEncode",
           "merge_fwd", "merge_torch", "pack_attn_model"]
