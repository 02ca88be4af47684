"""The temporal-attention layer around the HIP op (attn_op.py), once for the two attention-based base models.

tgn.py and tgat.py run the same layer on a frozen pack and on the live parameters: ``fold`` the per-neighbour
projections into per-row ones, describe the launch (``attn_spec``), run the op, apply ``mha_tail``.  Around it: the
keep masks of a training step, the opt-in state of the HIP training step (``HipTraining``), ``prep_inputs`` /
``stack_sides`` for a batch's index and time tensors, and ``affinity``.  What stays with a model is what only it
knows: its merger, its time features (their order and rounding), its ``keep_mask_shapes``, the layout of the folded
matrices it multiplies by, and TGN's memory.
"""
import numpy as np
import torch
import torch.nn.functional as F

from .attn_op import as_dev


# ------------------------------------------------------------------ the layer
def fold(mh, dtype=None, device=None, transposed=False):
    """(P [H dk, dq], G [dq, H dk]) of a MultiHeadAttention ``mh`` (its w_qs, w_ks, w_vs, fc): qf = P query replaces
    the per-neighbour key projection, fc(...) = G z the per-neighbour value projection (dk: the key width).

    ``dtype`` given (the packs: fp64): from detached copies on ``device`` in that dtype.  None (training): from the
    live parameters under autograd.  ``transposed``: (P^T [dq, H dk], G^T [H dk, dq]) instead, as TGAT multiplies by
    them -- asked of einsum as its output order, not transposed afterwards: the order decides which batched
    product einsum runs and what its backward sees, so each model keeps the products it always ran."""
    ws = [m.weight for m in (mh.w_qs, mh.w_ks, mh.w_vs, mh.fc)]
    if dtype is not None:
        ws = [w.detach().to(device, dtype) for w in ws]
    wq, wk, wv, fc = ws
    H, dh, dq = mh.n_head, mh.d_k, wq.shape[1]
    kq = torch.einsum("hoi,hoq->" + ("qhi" if transposed else "hiq"), wk.view(H, dh, -1), wq.view(H, dh, dq))
    vq = torch.einsum("qho,hoi->" + ("hiq" if transposed else "qhi"), fc.view(dq, H, dh), wv.view(H, dh, -1))
    if transposed:
        return kq.reshape(dq, -1), vq.reshape(-1, dq)
    return kq.reshape(-1, dq), vq.reshape(dq, -1)           # W_k,h^T W_q,h stacked over h; fc_h W_v,h side by side


def attn_spec(flavour, rows, n_ngh, n_head, d_key, d_node, d_time, temperature, head_major, seg_rows, *, node_tab,
              node_idx, edge_tab, edge_idx, dt, mask_node, err, time_w=None, time_b=None, edge_dense=None,
              table_grad=None):
    """The ``spec`` of attn_op.describe for one launch of ``flavour`` ("tgn" / "tgat").  node_idx None: the keys'
    node features come dense (AttnFn's ngh_dense).  ``edge_dense`` [rows n_ngh, d_edge] replaces the gather
    edge_tab[edge_idx].  time_w / time_b: TimeEncode's vectors (TrainAttnFn takes the live ones as arguments).
    ``table_grad``: TrainAttnFn's hook for a gathered node table's gradient (TGN)."""
    d_edge = edge_dense.shape[-1] if edge_dense is not None else edge_tab.shape[1]
    if d_node + d_edge + d_time != d_key:
        raise AssertionError(f"key dim {d_node}+{d_edge}+{d_time} != {d_key}")
    return dict(flavour=flavour, rows=rows, n_ngh=n_ngh, n_head=n_head, d_key=d_key, d_node=d_node, d_edge=d_edge,
                d_time=d_time, node_rows=node_tab.shape[0], edge_rows=edge_tab.shape[0], head_major=head_major,
                seg_rows=seg_rows, temperature=temperature, node_tab=node_tab, node_idx=node_idx,
                edge_tab=edge_dense if edge_dense is not None else edge_tab,
                edge_idx=None if edge_dense is not None else edge_idx, dt=dt, time_w=time_w, time_b=time_b,
                mask_node=mask_node, err=err, table_grad=table_grad)


def mha_tail(z, query, Gt, fc_bias, ln_w, ln_b, fkeep=None, scale=1.0):
    """MultiHeadAttention after the attention itself: fc (folded: z G^T + bias), fc's dropout as the keep mask
    ``fkeep`` times ``scale``, the residual and the LayerNorm -> [rows, dq].  ``Gt`` goes to addmm as it is given
    (TGAT: a contiguous G^T; TGN: the transposed view of a row-major G)."""
    out = torch.addmm(fc_bias, z, Gt)
    if fkeep is not None:
        out = out * (fkeep.to(out.dtype) * scale)
    return F.layer_norm(out + query, (query.shape[1],), ln_w, ln_b, 1e-5)


def affinity(pack, x1, x2):
    """affinity_score (fc2(relu(fc1([x1 | x2])))) on a pack's frozen copies a1w, a1b, a2w, a2b."""
    h = F.relu(F.linear(torch.cat([x1, x2], dim=1), pack["a1w"], pack["a1b"]))
    return F.linear(h, pack["a2w"], pack["a2b"])


# ------------------------------------------------------------------ keep masks
def draw_keep_masks(shapes, p, dev, generator=None):
    """One step's keep masks of ``shapes`` (uint8, 1 = kept with probability 1 - p): views of one flat buffer
    drawn on the device in one ``bernoulli_``."""
    sizes = [int(np.prod(sh)) for sh in shapes]
    flat = torch.empty(sum(sizes), dtype=torch.uint8, device=dev).bernoulli_(1.0 - float(p), generator=generator)
    return [x.view(sh) for x, sh in zip(flat.split(sizes), shapes)]


def checked_keep_masks(keep, shapes, dev, message):
    """Supplied masks viewed in ``shapes``; ValueError(message) unless they are len(shapes) uint8 tensors on
    ``dev`` of the shapes' sizes."""
    if len(keep) != len(shapes) or any(k.dtype != torch.uint8 or k.device != dev or k.numel() != int(np.prod(sh))
                                       for k, sh in zip(keep, shapes)):
        raise ValueError(message)
    return [k.contiguous().view(sh) for k, sh in zip(keep, shapes)]


def step_keep_masks(supplied, shapes, p, dev, message):
    """(masks, scale) of one step with dropout p: the supplied masks (checked) or, with p > 0, drawn ones; a list
    of None without either.  scale = 1 / (1 - p)."""
    keep = supplied
    if keep is None and p > 0.0:
        keep = draw_keep_masks(shapes, p, dev)
    keep = checked_keep_masks(keep, shapes, dev, message) if keep is not None else [None] * len(shapes)
    return keep, (1.0 / (1.0 - p) if p > 0.0 else 1.0)


# ------------------------------------------------------------------ opt-in state of the HIP training step
class HipTraining:
    """Mixin of a base model (before nn.Module in the bases) for its opt-in HIP training step.  It holds plain
    attributes only -- no parameter, buffer or submodule -- so the state_dict does not know it.  The model sets
    ``_label`` (error messages) and ``_param_error``, and has ``_pack_cache``."""
    _label = _param_error = None
    _train_on_hip = False
    _params_checked = _train_err = None

    def train_on_hip(self, flag=True):
        """Opt in to (or out of) the HIP training step: with the flag set, ``model.train()`` calls with gradients
        enabled run the training kernels (attn_op.TrainAttnFn) with the reference's two dropouts on the live
        parameters, and ``loss.backward()`` fills ``.grad`` on every parameter the reference's step trains.
        Default off: every other call keeps its path."""
        self._train_on_hip = bool(flag)
        self._params_checked = None
        return self

    def _apply(self, fn, *args, **kwargs):
        self._params_checked = None         # .to() / .float() / ...: the parameters are looked at again
        return super()._apply(fn, *args, **kwargs)

    def _train_hip_ok(self):
        return self._train_on_hip and self.training and torch.is_grad_enabled()

    def _live_state(self, dev):
        """The live parameters checked (once per train_on_hip() / .to(), not per step) and the kernels' error
        flag on ``dev`` -> dev."""
        if self._params_checked != dev:
            for p in self.parameters():
                if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError(self._param_error)
            self._params_checked = dev
        if self._train_err is None or self._train_err.device != dev:
            self._train_err = torch.zeros(1, dtype=torch.int32, device=dev)
        return dev

    def check_errors(self):
        """Raise if a kernel saw an out-of-range node or edge index (synchronises)."""
        for err in ((self._pack_cache or {}).get("err"), self._train_err):
            if err is not None and int(err.item()) != 0:
                err.zero_()
                raise IndexError(f"{self._label}: node or edge index out of range of the feature tables")


# ------------------------------------------------------------------ inputs
def prep_inputs(dev, nodes, eids, times, cut_time, n_segments=1, sides=1, lone_seg_rows=True, edge_attr=None):
    """What a 2-hop embedding derives from its inputs before any weight is read (retrieve_time_features etc.), as
    a dict: R rows, N neighbours, n0 [R] int64, n1 [R N] / n2 [R N N] int32 node ids, e1 / e2 int32 edge ids (None
    with ``edge_attr``, whose two tables are then ed1 [R N, d] / ed2 [R N N, d]), dt1 = cut - t1 and dt2 = t1 - t2
    in fp32 from fp64 differences, and ``seg`` = R / n_segments, the rows of one independent segment.

    What differs between the models is an argument.  ``sides``: cut_time may give one time per row or one per row
    of a period, R / (sides n_segments) rows -- TGN's segments are whole contrasts of 3 sides, TGAT's are single
    sides.  ``lone_seg_rows`` False: seg = 0 for a single segment (TGN), which the kernels read as all rows."""
    i32, f64 = torch.int32, torch.float64
    n0 = as_dev(nodes[0], dev, torch.long).reshape(-1)
    R = n0.shape[0]
    n1 = as_dev(nodes[1], dev, i32).reshape(R, -1)
    N = n1.shape[1]
    n2 = as_dev(nodes[2], dev, i32).reshape(R * N * N)
    if R % n_segments:
        raise AssertionError("rows must split evenly into n_segments")
    cut = as_dev(cut_time, dev, f64).reshape(-1)
    periods = sides * n_segments
    if periods > 1 and cut.shape[0] * periods == R:
        cut = cut.repeat(periods)
    if cut.shape[0] != R:
        raise AssertionError("cut_time must give one time per row (or per row of one period)")
    t1 = as_dev(times[0], dev, f64).reshape(R, N)
    t2 = as_dev(times[1], dev, f64).reshape(R, N, N)
    dt1 = (cut.view(R, 1) - t1).float().contiguous()
    dt2 = (t1.view(R, N, 1) - t2).float().contiguous()
    e1 = e2 = ed1 = ed2 = None
    if edge_attr is None:
        e1 = as_dev(eids[0], dev, i32).reshape(R * N).contiguous()
        e2 = as_dev(eids[1], dev, i32).reshape(R * N * N).contiguous()
    else:
        if any(isinstance(x, torch.Tensor) and x.requires_grad for x in edge_attr):
            raise NotImplementedError("gradient with respect to edge_attr")
        ed1 = as_dev(edge_attr[0], dev, torch.float32).reshape(R * N, -1).contiguous()
        ed2 = as_dev(edge_attr[1], dev, torch.float32).reshape(R * N * N, -1).contiguous()
    seg = R // n_segments if n_segments > 1 or lone_seg_rows else 0
    return dict(dev=dev, R=R, N=N, seg=seg, n_segments=n_segments, n0=n0, n1=n1.reshape(-1).contiguous(),
                n2=n2.contiguous(), e1=e1, e2=e2, ed1=ed1, ed2=ed2, dt1=dt1.reshape(-1), dt2=dt2.reshape(-1))


def cat_rows(xs):
    """torch.cat(xs) along dim 0 -- as a view when the tensors are consecutive row blocks of one contiguous
    tensor (a gathered pack's three sides, [3, B, ...]), else a copy.  Only for tensors without autograd
    history (the view would route gradients through the first one's base)."""
    a = xs[0]
    if all(isinstance(x, torch.Tensor) for x in xs) and not any(x.requires_grad for x in xs):
        st = a.untyped_storage().data_ptr()
        adjacent = all(x.is_contiguous() and x.dtype == a.dtype and x.device == a.device and x.dim() == a.dim()
                       and x.shape[1:] == a.shape[1:] and x.untyped_storage().data_ptr() == st for x in xs)
        if adjacent:
            off = a.storage_offset()
            for x in xs:
                if x.storage_offset() != off:
                    adjacent = False
                    break
                off += x.numel()
        if adjacent:
            # explicit contiguous strides: is_contiguous() ignores the stride of a size-1 dim, so a.stride()
            # may not describe consecutive rows when a has one row
            shape = (sum(int(x.shape[0]) for x in xs),) + tuple(a.shape[1:])
            strides, acc = [], 1
            for d in reversed(shape):
                strides.append(acc)
                acc *= int(d)
            return a.as_strided(shape, tuple(reversed(strides)), a.storage_offset())
    return torch.cat(list(xs))


def stack_sides(dev, roots, subgraphs, nodes=True, eids=True, hops=2, idx_dtype=torch.int32, times=True):
    """The sides of a contrast stacked along dim 0 -> (n0 [S B] int64, node ids, edge ids, times), each of the
    three a list of ``hops`` tensors ([S B, N], [S B, N^2]) in idx_dtype / fp64, or None where not asked for.
    ``subgraphs``: per side (node ids, edge ids, times), each a list over hops."""
    n0 = torch.cat([as_dev(x, dev, torch.long).reshape(-1) for x in roots])

    def cat(i, dtype):
        out = []
        for h in range(hops):
            xs = [sg[i][h] for sg in subgraphs]
            if all(isinstance(x, torch.Tensor) and x.device == dev for x in xs):
                # the three sides of a gathered pack are consecutive rows of one tensor: one view, and one
                # dtype conversion instead of three (elementwise, so the same values as convert-then-cat)
                out.append(as_dev(cat_rows(xs), dev, dtype))
            else:
                out.append(torch.cat([as_dev(x, dev, dtype) for x in xs]))
        return out
    return (n0, cat(0, idx_dtype) if nodes else None, cat(1, idx_dtype) if eids else None,
            cat(2, torch.float64) if times else None)


__all__ = ["fold", "attn_spec", "mha_tail", "affinity", "draw_keep_masks", "checked_keep_masks", "step_keep_masks",
           "HipTraining", "prep_inputs", "cat_rows", "stack_sides"]
