"""The HIP temporal-attention op of the two attention-based base models (tgn.py, tgat.py).

Both models run the same per-neighbour computation on one descriptor (``tm_attn``, include/tempme.h) through one
set of kernels (csrc/attn_kernels.h, csrc/attn_train.h); the flavour, ``spec["flavour"]`` = ``"tgn"`` or
``"tgat"``, selects the C entry points (the rounding of the time feature, and what each backward can return) and
the label of the error messages.

``spec`` is the dict of the descriptor's sizes and tensors that ``attn_layer.attn_spec`` builds (the one place that
lists its keys).  The layer the two models build around this op -- folded projections, the multi-head tail, keep
masks, the training opt-in, input preparation -- is attn_layer.py; ``as_dev`` here is the one host-or-device
conversion every module of the package uses.
"""
import numpy as np
import torch

from . import _lib as L

# label: error messages; d_qf: the frozen backward returns the gradient of the folded query; slot_ab: the training
# backward takes the per-(slot, head) scalars' output, from which spec["table_grad"] forms a gathered table's gradient
_FLAVOURS = {"tgn": dict(label="TGN", d_qf=False, slot_ab=True),
             "tgat": dict(label="TGAT", d_qf=True, slot_ab=False)}


def _entry(spec, name):
    return getattr(L.lib(), f"tm_{spec['flavour']}_attn_{name}")


def as_dev(x, device, dtype):
    """A tensor or host array on ``device`` in ``dtype`` (no copy where it already is)."""
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(device=device, dtype=dtype)


def describe(spec, qf, ngh_dense, ew):
    """tm_attn of ``spec`` for the folded queries qf, a dense neighbour table (or None: spec's node_tab) and
    explanation weights (or None)."""
    a = L.Attn()
    a.rows, a.n_ngh, a.n_head = spec["rows"], spec["n_ngh"], spec["n_head"]
    a.d_node, a.d_edge, a.d_time = spec["d_node"], spec["d_edge"], spec["d_time"]
    a.node_rows, a.edge_rows = spec["node_rows"], spec["edge_rows"]
    a.head_major_rows = 1 if spec["head_major"] else 0
    a.seg_rows = spec.get("seg_rows", 0)
    a.temperature = spec["temperature"]
    a.node_tab = (ngh_dense if ngh_dense is not None else spec["node_tab"]).data_ptr()
    a.node_idx = spec["node_idx"].data_ptr() if spec["node_idx"] is not None else None
    a.edge_tab = spec["edge_tab"].data_ptr() if spec["edge_tab"] is not None else None
    a.edge_idx = spec["edge_idx"].data_ptr() if spec["edge_idx"] is not None else None
    a.dt = spec["dt"].data_ptr()
    a.time_w, a.time_b = spec["time_w"].data_ptr(), spec["time_b"].data_ptr()
    a.mask_node = spec["mask_node"].data_ptr()
    a.ew = ew.data_ptr() if ew is not None else None
    a.qf = qf.data_ptr()
    a.err_flag = spec["err"].data_ptr()
    return a


def attn_probs(spec, qf, ngh_dense, probs=True, mean=True):
    """(probs [rows, n_head, n_ngh], mean [rows, n_ngh]) of one launch of tm_*_attn_probs on the descriptor a
    forward of ``spec`` runs on: the softmax the forward keeps to itself and its mean over the heads (None for the
    one not asked for).  No gradient; explanation weights do not enter (the forward applies them after the
    softmax)."""
    if not (probs or mean):
        raise ValueError("attn_probs: ask for probs, mean or both")
    dev = qf.device
    R, H, N = spec["rows"], spec["n_head"], spec["n_ngh"]
    desc = describe(spec, qf.detach(), None if ngh_dense is None else ngh_dense.detach(), None)
    p = torch.empty((R, H, N), dtype=torch.float32, device=dev) if probs else None
    m = torch.empty((R, N), dtype=torch.float32, device=dev) if mean else None
    if R:
        L.check(_entry(spec, "probs")(L.C.byref(desc), L.ptr(p), L.ptr(m), L.stream_ptr(dev)),
                f"{_FLAVOURS[spec['flavour']]['label']} attention probabilities")
    return p, m


class AttnFn(torch.autograd.Function):
    """z = tm_*_attn_fwd(...) of the frozen base model; backward through tm_*_attn_bwd: the explanation weights,
    the dense neighbour table (the upper layer's input) and, for TGAT, the folded query."""

    @staticmethod
    def forward(ctx, qf, ngh_dense, ew, spec):
        dev = qf.device
        R, H, dk = spec["rows"], spec["n_head"], spec["d_key"]
        desc = describe(spec, qf, ngh_dense, ew)
        z = torch.empty((R, H * dk), dtype=torch.float32, device=dev)
        stats = torch.empty((R, H, 2), dtype=torch.float32, device=dev)
        if R:
            L.check(_entry(spec, "fwd")(L.C.byref(desc), L.ptr(z), L.ptr(stats), L.stream_ptr(dev)),
                    f"{_FLAVOURS[spec['flavour']]['label']} attention")
        ctx.spec = spec
        ctx.save_for_backward(qf, ngh_dense, ew, stats)
        return z

    @staticmethod
    def backward(ctx, gz):
        qf, ngh_dense, ew, stats = ctx.saved_tensors
        spec = ctx.spec
        fl = _FLAVOURS[spec["flavour"]]
        if ctx.needs_input_grad[0] and not fl["d_qf"]:
            raise NotImplementedError(f"{fl['label']} attention: gradient with respect to the queries (base model "
                                      "is frozen)")
        R, H, N = spec["rows"], spec["n_head"], spec["n_ngh"]
        dev = gz.device
        gz = gz.contiguous().float()
        want_node = ngh_dense is not None and ctx.needs_input_grad[1]
        parts = torch.empty((R * H, N), dtype=torch.float32, device=dev)
        d_node = torch.empty_like(ngh_dense) if want_node else None
        d_qf = torch.empty_like(qf) if ctx.needs_input_grad[0] else None
        if R:
            desc = describe(spec, qf, ngh_dense, ew)
            outs = (L.ptr(parts), L.ptr(d_node)) + ((L.ptr(d_qf),) if fl["d_qf"] else ())
            L.check(_entry(spec, "bwd")(L.C.byref(desc), L.ptr(stats), L.ptr(gz), *outs, L.stream_ptr(dev)),
                    f"{fl['label']} attention backward")
        d_ew = None
        if ew is not None and ctx.needs_input_grad[2]:
            # pair q = r*H + h contributes to weight row base + ((r-base)*H + h) % seg of its segment
            seg = spec.get("seg_rows", 0) or max(R, 1)
            if spec["head_major"]:
                d_ew = parts.view(R // seg, H, seg, N).sum(1)
            else:
                d_ew = parts.view(R, H, N).sum(1)
            d_ew = d_ew.reshape(ew.shape)
        return d_qf, d_node, d_ew, None


class TrainAttnFn(torch.autograd.Function):
    """z = tm_*_attn_train_fwd(...) with the attention dropout's keep mask; backward through tm_*_attn_train_bwd:
    the folded query, TimeEncode's two vectors (tw, tb) through the keys' time features, and the keys' node
    features -- the dense neighbour rows, or (TGN, ``tab`` given) the rows of a gathered table: the backward then
    also stores slot_ab, and ``spec["table_grad"](spec, desc, slot_ab, gz, tab)`` returns the table's gradient."""

    @staticmethod
    def forward(ctx, qf, ngh_dense, tab, tw, tb, spec, keep, keep_scale):
        dev = qf.device
        R, H, dk = spec["rows"], spec["n_head"], spec["d_key"]
        spec = dict(spec, time_w=tw, time_b=tb)
        if tab is not None:
            spec["node_tab"] = tab
        desc = describe(spec, qf, ngh_dense, None)
        z = torch.empty((R, H * dk), dtype=torch.float32, device=dev)
        stats = torch.empty((R, H, 2), dtype=torch.float32, device=dev)
        L.check(_entry(spec, "train_fwd")(L.C.byref(desc), L.ptr(keep), keep_scale, L.ptr(z), L.ptr(stats),
                                          L.stream_ptr(dev)),
                f"{_FLAVOURS[spec['flavour']]['label']} training attention")
        ctx.spec, ctx.keep, ctx.keep_scale = spec, keep, keep_scale
        ctx.dense = ngh_dense is not None
        # the backward rebuilds the keys: saved, so that an in-place change between forward and backward is
        # caught by autograd's version check
        ctx.save_for_backward(qf, ngh_dense if ctx.dense else spec["node_tab"], stats, tw, tb)
        return z

    @staticmethod
    def backward(ctx, gz):
        qf, node, stats, tw, tb = ctx.saved_tensors
        spec = dict(ctx.spec, node_tab=node, time_w=tw, time_b=tb)
        fl = _FLAVOURS[spec["flavour"]]
        R, N, H, dT = spec["rows"], spec["n_ngh"], spec["n_head"], spec["d_time"]
        dev = gz.device
        gz = gz.contiguous().float()
        want_tab = not ctx.dense and ctx.needs_input_grad[2]
        d_node = torch.empty_like(node) if ctx.dense and ctx.needs_input_grad[1] else None
        d_qf = torch.empty_like(qf)
        d_time = torch.empty((2, dT), dtype=torch.float32, device=dev)
        ab = torch.empty((R, N, H, 2), dtype=torch.float32, device=dev) if want_tab else None
        ws = torch.empty(int(_entry(spec, "train_workspace_bytes")(R, dT)), dtype=torch.uint8, device=dev)
        desc = describe(spec, qf, node if ctx.dense else None, None)
        outs = (None, L.ptr(d_node), L.ptr(d_qf), L.ptr(d_time)) + ((L.ptr(ab),) if fl["slot_ab"] else ())
        L.check(_entry(spec, "train_bwd")(L.C.byref(desc), L.ptr(ctx.keep), ctx.keep_scale, L.ptr(stats), L.ptr(gz),
                                          *outs, L.ptr(ws), L.stream_ptr(dev)),
                f"{fl['label']} training attention backward")
        d_tab = spec["table_grad"](spec, desc, ab, gz, node) if want_tab else None
        return d_qf, d_node, d_tab, d_time[0], d_time[1], None, None, None


__all__ = ["AttnFn", "TrainAttnFn", "attn_probs", "describe", "as_dev"]
