"""attn_layer: the pieces of the temporal-attention layer that tgn.py and tgat.py share, each against the expression
it replaced, restated here.  No GPU and no library: everything runs on CPU tensors, bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tempme_amd import attn_layer as AL
from tempme_amd import tgat as TA
from tempme_amd import tgn as TG

CPU = torch.device("cpu")
N_FEAT, E_FEAT = np.zeros((5, 4), np.float32), np.zeros((7, 3), np.float32)


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """Tensors of a few hundred elements: a thread pool only costs (tens of milliseconds per batched product)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------ fold
def _mh(kind, H):
    torch.manual_seed(7 * H + len(kind))
    if kind == "tgn":           # d_node 4, d_edge 3: key 4 + 3 + 4 = 11, query 4 + 4 = 8
        return TG.MultiHeadAttention(n_head=H, d_emb=8, d_k=11, d_v=11)
    return TA.MultiHeadAttention(H, d_model=12, d_k=12 // H, d_v=12 // H)


def _einsum_pair(wq, wk, wv, fc, H, outs=("hiq", "qhi")):
    """The two products as the models wrote them: [H, dk, dq] W_k^T W_q and [dq, H, dk] fc W_v in ``outs`` order."""
    dq, dh = wq.shape[1], wq.shape[0] // H
    kq = torch.einsum("hoi,hoq->" + outs[0], wk.view(H, dh, -1), wq.view(H, dh, dq))
    vq = torch.einsum("qho,hoi->" + outs[1], fc.view(dq, H, dh), wv.view(H, dh, -1))
    return kq, vq


def _weights(mh, dtype=None):
    ws = [m.weight for m in (mh.w_qs, mh.w_ks, mh.w_vs, mh.fc)]
    return [w.detach().to(CPU, dtype) for w in ws] if dtype is not None else ws


@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("kind", ["tgn", "tgat"])
def test_fold_equals_the_einsum_pair(kind, H):
    mh = _mh(kind, H)
    dq = mh.w_qs.weight.shape[1]
    dk = mh.w_ks.weight.shape[1]
    for dtype in (torch.float64, torch.float32, None):
        kq, vq = _einsum_pair(*_weights(mh, dtype), H)
        P, G = AL.fold(mh, dtype, CPU)
        assert P.shape == (H * dk, dq) and G.shape == (dq, H * dk)
        assert P.dtype == (dtype or torch.float32) and (P.requires_grad is (dtype is None))
        assert torch.equal(P, kq.reshape(H * dk, dq)) and torch.equal(G, vq.reshape(dq, H * dk))
        # the transposed pair: TGAT's training step wrote it as the permuted products, reshaped
        ktq, vtq = _einsum_pair(*_weights(mh, dtype), H, ("qhi", "hiq"))
        Pt, Gt = AL.fold(mh, dtype, CPU, transposed=True)
        assert torch.equal(Pt, ktq.reshape(dq, H * dk)) and torch.equal(Gt, vtq.reshape(H * dk, dq))
        assert torch.equal(Pt, P.t()) and torch.equal(Gt, G.t())


@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("kind", ["tgn", "tgat"])
@pytest.mark.parametrize("transposed", [False, True])
def test_fold_gradients_equal_the_einsum_pair(kind, H, transposed):
    mh = _mh(kind, H)
    ws = _weights(mh)
    dq, dk = ws[0].shape[1], ws[1].shape[1]
    g = torch.Generator().manual_seed(3)
    cP, cG = torch.randn(H * dk, dq, generator=g), torch.randn(dq, H * dk, generator=g)
    if transposed:
        cP, cG = cP.t().contiguous(), cG.t().contiguous()
        kq, vq = _einsum_pair(*ws, H, ("qhi", "hiq"))
    else:
        kq, vq = _einsum_pair(*ws, H)
    want = torch.autograd.grad((kq.reshape(cP.shape) * cP).sum() + (vq.reshape(cG.shape) * cG).sum(), ws)
    P, G = AL.fold(mh, transposed=transposed)
    got = torch.autograd.grad((P * cP).sum() + (G * cG).sum(), ws)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ mha_tail
@pytest.mark.parametrize("with_keep", [False, True])
def test_mha_tail_equals_the_three_lines(with_keep):
    g = torch.Generator().manual_seed(5)
    R, dq, hk = 7, 8, 22
    z, query = torch.randn(R, hk, generator=g), torch.randn(R, dq, generator=g)
    G, fcb = torch.randn(dq, hk, generator=g), torch.randn(dq, generator=g)
    lnw, lnb = torch.randn(dq, generator=g), torch.randn(dq, generator=g)
    fkeep = (torch.rand(R, dq, generator=g) < 0.7).to(torch.uint8) if with_keep else None
    scale = 1.0 / 0.7 if with_keep else 1.0
    for Gt in (G.t(), G.t().contiguous()):            # TGN's transposed view, TGAT's contiguous G^T
        out = torch.addmm(fcb, z, Gt)
        if fkeep is not None:
            out = out * (fkeep.to(out.dtype) * scale)
        want = F.layer_norm(out + query, (dq,), lnw, lnb, 1e-5)
        assert torch.equal(AL.mha_tail(z, query, Gt, fcb, lnw, lnb, fkeep, scale), want)


def test_attn_spec_lists_every_key_and_checks_the_key_width():
    tab, etab = torch.zeros(5, 4), torch.zeros(7, 3)
    idx = torch.zeros(6, dtype=torch.int32)
    kw = dict(node_tab=tab, node_idx=idx, edge_tab=etab, edge_idx=idx, dt=tab, mask_node=idx, err=idx)
    spec = AL.attn_spec("tgn", 2, 3, 2, 11, 4, 4, 3.0, True, 0, **kw)
    assert (spec["d_edge"], spec["node_rows"], spec["edge_rows"], spec["seg_rows"]) == (3, 5, 7, 0)
    assert spec["edge_tab"] is etab and spec["edge_idx"] is idx and spec["table_grad"] is None
    dense = torch.zeros(6, 2)
    spec = AL.attn_spec("tgn", 2, 3, 2, 10, 4, 4, 3.0, True, 0, edge_dense=dense, **kw)
    assert spec["edge_tab"] is dense and spec["edge_idx"] is None and spec["d_edge"] == 2 and spec["edge_rows"] == 7
    with pytest.raises(AssertionError, match="key dim"):
        AL.attn_spec("tgat", 2, 3, 2, 12, 4, 4, 3.0, True, 0, **kw)


# ------------------------------------------------------------------ prep_inputs
def _raw_inputs(R=6, N=3, seed=11):
    rng = np.random.default_rng(seed)
    nodes = [rng.integers(1, 5, R), rng.integers(0, 5, (R, N)), rng.integers(0, 5, (R, N * N))]
    eids = [rng.integers(0, 7, (R, N)), rng.integers(0, 7, (R, N * N))]
    times = [rng.random((R, N)) * 1e6, rng.random((R, N * N)) * 1e6]
    return nodes, eids, times, rng.random(R) * 1e6 + 1e6


@pytest.mark.parametrize("n_segments", [1, 2, 3])
def test_prep_inputs_offsets_and_segments(n_segments):
    R, N = 6, 3
    nodes, eids, times, cut = _raw_inputs(R, N)
    t1, t2 = torch.from_numpy(times[0]), torch.from_numpy(times[1]).view(R, N, N)
    dt1 = (torch.from_numpy(cut).view(R, 1) - t1).float().reshape(-1)
    dt2 = (t1.view(R, N, 1) - t2).float().reshape(-1)
    tgn = AL.prep_inputs(CPU, nodes, eids, times, cut, n_segments, sides=3, lone_seg_rows=False)
    tgat = AL.prep_inputs(CPU, nodes, eids, times, cut, n_segments)
    assert tgn["seg"] == {1: 0, 2: 3, 3: 2}[n_segments] and tgat["seg"] == {1: 6, 2: 3, 3: 2}[n_segments]
    for x in (tgn, tgat):
        assert (x["R"], x["N"], x["n_segments"]) == (R, N, n_segments)
        assert torch.equal(x["dt1"], dt1) and torch.equal(x["dt2"], dt2) and x["dt1"].dtype == torch.float32
        assert x["n0"].dtype == torch.long and torch.equal(x["n0"], torch.from_numpy(nodes[0]))
        for k, src in (("n1", nodes[1]), ("n2", nodes[2]), ("e1", eids[0]), ("e2", eids[1])):
            assert x[k].dtype == torch.int32 and x[k].is_contiguous()
            assert torch.equal(x[k], torch.from_numpy(src).reshape(-1).int())
        assert x["ed1"] is None and x["ed2"] is None


def test_prep_inputs_cut_time_broadcast_and_refusals():
    R, N = 6, 3
    nodes, eids, times, cut = _raw_inputs(R, N)
    per_row = AL.prep_inputs(CPU, nodes, eids, times, cut, 1)
    # one time per row of a period: TGN's period is R / (3 n_segments) rows, TGAT's R / n_segments
    for kw, period in ((dict(n_segments=1, sides=3), 2), (dict(n_segments=2, sides=3), 1),
                       (dict(n_segments=2), 3), (dict(n_segments=3), 2)):
        full = np.tile(cut[:period], R // period)
        want = AL.prep_inputs(CPU, nodes, eids, times, full, kw["n_segments"])
        got = AL.prep_inputs(CPU, nodes, eids, times, cut[:period], **kw)
        assert torch.equal(got["dt1"], want["dt1"]) and not torch.equal(got["dt1"], per_row["dt1"])
    # one segment of single sides: nothing to repeat, so a shorter cut_time is refused
    with pytest.raises(AssertionError, match="cut_time"):
        AL.prep_inputs(CPU, nodes, eids, times, cut[:2], 1)
    with pytest.raises(AssertionError, match="cut_time"):
        AL.prep_inputs(CPU, nodes, eids, times, cut[:5], 2, sides=3)
    with pytest.raises(AssertionError, match="n_segments"):
        AL.prep_inputs(CPU, nodes, eids, times, cut, 4)


def test_prep_inputs_edge_attr():
    R, N = 6, 3
    nodes, eids, times, cut = _raw_inputs(R, N)
    ea = [torch.rand(R, N, 2), torch.rand(R, N * N, 2)]
    x = AL.prep_inputs(CPU, nodes, None, times, cut, sides=3, lone_seg_rows=False, edge_attr=ea)
    assert x["e1"] is None and x["e2"] is None
    assert torch.equal(x["ed1"], ea[0].reshape(R * N, 2)) and torch.equal(x["ed2"], ea[1].reshape(R * N * N, 2))
    assert x["ed1"].data_ptr() == ea[0].data_ptr()                 # already fp32 and contiguous: no copy
    with pytest.raises(NotImplementedError):
        AL.prep_inputs(CPU, nodes, None, times, cut, edge_attr=[ea[0].requires_grad_(), ea[1]])


# ------------------------------------------------------------------ stack_sides
def _sides(B=4, N=3, seed=2, tensors=False, adjacent=False):
    rng = np.random.default_rng(seed)
    roots = [rng.integers(1, 9, B) for _ in range(3)]
    shapes = (N, N * N)
    packs = [[rng.integers(0, 9, (3, B, w)) for w in shapes], [rng.integers(0, 99, (3, B, w)) for w in shapes],
             [rng.random((3, B, w)) * 1e6 for w in shapes]]
    if tensors:
        packs = [[torch.from_numpy(p) for p in field] for field in packs]
        if not adjacent:
            packs = [[[q.clone() for q in p] for p in field] for field in packs]      # separate storages
    return roots, [tuple([field[h][s] for h in (0, 1)] for field in packs) for s in range(3)]


def _convert_then_cat(roots, sgs, hops, idx_dtype):
    def cat(i, dtype):
        return [torch.cat([torch.as_tensor(np.asarray(sg[i][h])).to(dtype) for sg in sgs]) for h in range(hops)]
    n0 = torch.cat([torch.as_tensor(np.asarray(r)).long().reshape(-1) for r in roots])
    return n0, cat(0, idx_dtype), cat(1, idx_dtype), cat(2, torch.float64)


@pytest.mark.parametrize("layout", ["host", "tensors", "adjacent"])
def test_stack_sides_equals_convert_then_cat(layout):
    roots, sgs = _sides(tensors=layout != "host", adjacent=layout == "adjacent")
    for hops, idx_dtype in ((2, torch.int32), (1, torch.long)):
        want = _convert_then_cat(roots, sgs, hops, idx_dtype)
        got = AL.stack_sides(CPU, roots, sgs, hops=hops, idx_dtype=idx_dtype)
        assert torch.equal(got[0], want[0]) and got[0].dtype == torch.long
        for g, w, dtype in zip(got[1:], want[1:], (idx_dtype, idx_dtype, torch.float64)):
            assert len(g) == hops
            for a, b in zip(g, w):
                assert a.dtype == dtype and a.shape == b.shape and torch.equal(a, b)
    n0, nodes, eids, times = AL.stack_sides(CPU, roots, sgs, nodes=False, eids=False)
    assert nodes is None and eids is None and len(times) == 2
    if layout == "adjacent":          # consecutive rows of one tensor in the wanted dtype: a view, no copy
        assert times[0].data_ptr() == sgs[0][2][0].data_ptr()


# ------------------------------------------------------------------ keep masks
def _models():
    tgn = TG.TGN(N_FEAT, E_FEAT, 3)
    tgat = TA.TGAT(N_FEAT, E_FEAT, 3, num_layers=2, n_head=1)
    return tgn, tgat


def test_keep_masks_drawn_from_one_flat_buffer():
    for m, count in zip(_models(), (4, 6)):
        shapes = m.keep_mask_shapes(6, 3)
        assert len(shapes) == count
        keep = AL.draw_keep_masks(shapes, 0.25, CPU, torch.Generator().manual_seed(1))
        assert [tuple(k.shape) for k in keep] == [tuple(sh) for sh in shapes]
        off = keep[0].storage_offset()
        for k in keep:
            assert k.dtype == torch.uint8 and int(k.max()) <= 1 and k.is_contiguous()
            assert k.untyped_storage().data_ptr() == keep[0].untyped_storage().data_ptr()
            assert k.storage_offset() == off
            off += k.numel()
        again = AL.draw_keep_masks(shapes, 0.25, CPU, torch.Generator().manual_seed(1))
        assert all(torch.equal(a, b) for a, b in zip(keep, again))
        assert 0.5 < torch.cat([k.reshape(-1) for k in keep]).float().mean() < 0.95


def test_keep_masks_checked():
    messages = ("TGN.tgn_keep_masks: expected draw_keep_masks(R1, N)'s four uint8 masks on the device",
                "TGAT.tgat_keep_masks: expected draw_keep_masks(R, N)'s six uint8 masks on the device")
    for m, message in zip(_models(), messages):
        shapes = m.keep_mask_shapes(6, 3)
        keep = AL.draw_keep_masks(shapes, 0.25, CPU)
        flat = [k.reshape(-1) for k in keep]
        ok = AL.checked_keep_masks(flat, shapes, CPU, message)
        assert [tuple(k.shape) for k in ok] == [tuple(sh) for sh in shapes]
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(ok, keep))
        bad = [keep[:-1], [keep[0].float()] + keep[1:], [keep[0].reshape(-1)[1:]] + keep[1:]]
        for wrong in bad:                                     # count, dtype, numel
            with pytest.raises(ValueError) as e:
                AL.checked_keep_masks(wrong, shapes, CPU, message)
            assert str(e.value) == message
        with pytest.raises(ValueError):
            AL.step_keep_masks(keep[:-1], shapes, 0.25, CPU, message)
        got, scale = AL.step_keep_masks(keep, shapes, 0.25, CPU, message)
        assert scale == 1.0 / 0.75 and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, keep))
        got, scale = AL.step_keep_masks(None, shapes, 0.5, CPU, message)
        assert scale == 2.0 and [tuple(k.shape) for k in got] == [tuple(sh) for sh in shapes]
        assert AL.step_keep_masks(None, shapes, 0.0, CPU, message) == ([None] * len(shapes), 1.0)


# ------------------------------------------------------------------ the opt-in mixin
_ATTN = ("multi_head_target.w_qs.weight multi_head_target.w_ks.weight multi_head_target.w_vs.weight")
TGN_KEYS = ("""n_feat_th e_feat_th node_raw_features.weight edge_raw_features.weight time_encoder.w.weight
time_encoder.w.bias memory.memory memory.last_update message_function.mlp.0.weight message_function.mlp.0.bias
message_function.mlp.2.weight message_function.mlp.2.bias message_function.layers.0.weight
message_function.layers.0.bias message_function.layers.2.weight message_function.layers.2.bias
memory_updater.memory.memory memory_updater.memory.last_update memory_updater.layer_norm.weight
memory_updater.layer_norm.bias memory_updater.memory_updater.weight_ih memory_updater.memory_updater.weight_hh
memory_updater.memory_updater.bias_ih memory_updater.memory_updater.bias_hh embedding_module.node_features.weight
embedding_module.edge_features.weight embedding_module.time_encoder.w.weight embedding_module.time_encoder.w.bias """
            + " ".join(f"embedding_module.attention_models.{i}.{k}" for i in (0, 1) for k in (
                "merger.fc1.weight merger.fc1.bias merger.fc2.weight merger.fc2.bias " + _ATTN + " multi_head_target.fc.weight"
                " multi_head_target.fc.bias multi_head_target.layer_norm.weight multi_head_target.layer_norm.bias").split())
            + " affinity_score.fc1.weight affinity_score.fc1.bias affinity_score.fc2.weight affinity_score.fc2.bias").split()
TGAT_KEYS = ("n_feat_th e_feat_th edge_raw_embed.weight node_raw_embed.weight time_encoder.basis_freq time_encoder.phase "
             + " ".join(f"attn_model_list.{i}.{k}" for i in (0, 1) for k in (
                 "merger.fc11.weight merger.fc11.bias merger.fc12.weight merger.fc12.bias merger.fc21.weight"
                 " merger.fc21.bias merger.fc22.weight merger.fc22.bias " + _ATTN + " multi_head_target.layer_norm.weight"
                 " multi_head_target.layer_norm.bias multi_head_target.fc.weight multi_head_target.fc.bias").split())
             + " affinity_score.fc1.weight affinity_score.fc1.bias affinity_score.fc2.weight affinity_score.fc2.bias").split()


def test_mixin_adds_no_state_dict_key():
    tgn, tgat = _models()
    assert len(TGN_KEYS) == 54 and len(TGAT_KEYS) == 40
    assert list(tgn.state_dict()) == TGN_KEYS
    assert list(tgat.state_dict()) == TGAT_KEYS
    for m, keys in ((tgn, TGN_KEYS), (tgat, TGAT_KEYS)):
        assert m.train_on_hip() is m and m._train_on_hip is True
        m._params_checked = CPU
        m._live_state(CPU)                                   # creates the error flag: a plain attribute
        assert m._train_err.dtype == torch.int32 and list(m.state_dict()) == keys
        m.check_errors()
        m._train_err.fill_(1)
        with pytest.raises(IndexError, match=f"^{m._label}: node or edge index"):
            m.check_errors()
        assert int(m._train_err) == 0
        m.float()                                            # _apply: the parameters are looked at again
        assert m._params_checked is None and m._live_state(CPU) == CPU and m._params_checked == CPU
        m.half()
        with pytest.raises(RuntimeError) as e:
            m._live_state(CPU)
        assert str(e.value) == m._param_error and m._label in m._param_error
        assert m.train_on_hip(False)._train_on_hip is False
