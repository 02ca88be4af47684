"""Base-TGAT training (learn_base.py for --base_type tgat) on the CPU: the reference-shaped torch formulation of
the training step (tests/tgat_train_ref.py) against the reference's own step (tests/golden/tgat_train.npz) in fp32
and fp64, the keep masks' layout, the closed-form backward the kernel tests use against autograd, the C ABI of the
HIP training pair and learn_base's switch.

Tolerances follow tests/test_gm_train_cpu.py: logits and loss within test_graphmixer_oracle's ATOL / RTOL of the
reference's, every stored gradient within 1e-5 relative norm, every stored Frobenius norm within 1e-5 relative."""
import ctypes

import numpy as np
import pytest
import torch

import tgat_train_inputs as TT
import tgat_train_ref as TR
from tests.test_graphmixer_oracle import ATOL, RTOL

DTYPES = {"32": torch.float32, "64": torch.float64}


@pytest.mark.parametrize("tag", ["32", "64"])
@pytest.mark.parametrize("case", list(TT.CASES))
def test_formulation_matches_reference_step(case, tag):
    g = TT.golden()
    m = TT.build_model(case)
    loss, pos, neg, grads = TR.loss_and_grads(m.state_dict(), TT.heads(case), TT.batch(), dtype=DTYPES[tag])
    ref_loss, ref_logits, ref_grads, ref_norms = TT.stored(g, case, tag)
    got = torch.cat([pos, neg]).double().reshape(-1).numpy()
    np.testing.assert_allclose(got, ref_logits, atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(float(loss), ref_loss, atol=ATOL, rtol=RTOL)
    names = {k for k, v in m.named_parameters() if v.requires_grad}
    assert set(ref_grads) | set(ref_norms) == names and len(names) == 36
    if case in TT.SMALL:
        assert not ref_norms, "the small models store every gradient in full"
    for k, ref in ref_grads.items():
        err, nref = float(torch.linalg.norm(grads[k].double() - ref)), float(torch.linalg.norm(ref))
        assert err <= 1e-5 * nref, (k, err, nref)
    for k, ref in ref_norms.items():
        n = float(torch.linalg.norm(grads[k].double()))
        assert abs(n - ref) <= 1e-5 * ref, (k, n, ref)


def test_reference_fp32_envelope_of_the_gradients():
    """||g_32 - g_64|| / ||g_64|| of the reference's own step on the two small models: the envelope the GPU bound
    10 ||g_32 - g_64|| is taken from stays far below the 1e-4 floor's scale (measured 2.4e-7 .. 2.0e-6)."""
    g = TT.golden()
    for case in TT.SMALL:
        g32, g64 = TT.stored(g, case, "32")[2], TT.stored(g, case, "64")[2]
        for k, ref in g64.items():
            nref = float(torch.linalg.norm(ref))
            if nref > 0:
                assert float(torch.linalg.norm(g32[k] - ref)) < 1e-5 * nref, (case, k)


def test_keep_masks_layout_and_scale():
    """All-ones masks with keep_scale 1 are the no-dropout step; zeroing the bytes of one (row, head) pair of pass 3
    on the src side moves the logits of that row alone; a zeroed fc mask of pass 3 leaves fc without a gradient."""
    case = "small24"
    m = TT.build_model(case)
    sd, batch, H = m.state_dict(), TT.batch(), TT.heads(case)
    B, N = len(batch[0]), 20
    Rr, dm = 3 * B, m.model_dim
    shapes = [(Rr * H * N,), (Rr * N * H * N,), (Rr * H * N,), (Rr, dm), (Rr * N, dm), (Rr, dm)]
    assert hasattr(m, "keep_mask_shapes") and [tuple(s) for s in m.keep_mask_shapes(Rr, N)] == shapes
    ones = [torch.ones(s, dtype=torch.uint8) for s in shapes]
    _, p0, n0, _ = TR.loss_and_grads(sd, H, batch)
    _, p1, n1, _ = TR.loss_and_grads(sd, H, batch, keep=ones, keep_scale=1.0)
    assert torch.equal(p0, p1) and torch.equal(n0, n1)
    k = [x.clone() for x in ones]
    row, head = 5, 1
    k[2].view(Rr, H, N)[row, head] = 0
    _, p2, n2, _ = TR.loss_and_grads(sd, H, batch, keep=k, keep_scale=1.0)
    moved = ((p2 - p0).abs().reshape(-1) > 0) | ((n2 - n0).abs().reshape(-1) > 0)
    assert moved[row] and int(moved.sum()) == 1
    k = [x.clone() for x in ones]
    k[5][:] = 0
    _, _, _, g = TR.loss_and_grads(sd, H, batch, keep=k, keep_scale=1.0)
    assert float(g["attn_model_list.1.multi_head_target.fc.weight"].abs().max()) == 0.0
    assert float(g["attn_model_list.0.multi_head_target.fc.weight"].abs().max()) > 0.0


def test_closed_form_backward_equals_autograd():
    """The fp64 restatement the kernel tests hold tm_tgat_attn_train_bwd to (test_gpu_tgat_train.train_attn_ref)
    against autograd through the forward formula, the time parameters included."""
    from tests.test_gpu_tgat_train import KERNEL_CASES, kernel_inputs, pair_rows, train_attn_ref
    for case in (KERNEL_CASES[1], KERNEL_CASES[5]):
        x = kernel_inputs(case, seed=11)
        ref = train_attn_ref(x, x.keep, x.scale)
        Rr, N, H = x.R, x.N, x.H
        node = x.node.double().requires_grad_(True)
        qf = x.qf.double().requires_grad_(True)
        tw, tb = x.tw.double().requires_grad_(True), x.tb.double().requires_grad_(True)
        ew = (torch.ones(Rr, N, dtype=torch.float64) if x.ew is None else x.ew.double()).requires_grad_(True)
        tf = TR.TimeFeature.apply(x.dt, tw, tb)
        key = torch.cat([node, x.edge.double(), tf], dim=-1)
        m = pair_rows(Rr, H, x.seg)
        s = torch.einsum("rhc,rjc->rhj", qf, key) / x.T
        p = torch.softmax(s.masked_fill(x.mask[m] == 0, -1e10), dim=-1)
        z = torch.einsum("rhj,rjc->rhc", p * ew[m] * (x.keep.view(Rr, H, N).double() * x.scale), key)
        (z * x.gz.double()).sum().backward()
        d_ew = torch.zeros(Rr, N, dtype=torch.float64).index_put_((m.reshape(-1),), ref.d_ew.reshape(Rr * H, N),
                                                                  accumulate=True)
        for name, got, want in (("z", ref.z, z.detach()), ("d_qf", ref.d_qf, qf.grad), ("d_node", ref.d_node, node.grad),
                                ("d_ew", d_ew, ew.grad), ("d_freq", ref.d_time[0], tw.grad),
                                ("d_phase", ref.d_time[1], tb.grad)):
            scale = max(1.0, float(want.abs().max()))
            assert float((got - want).abs().max()) <= 1e-11 * scale, (case, name)
        assert bool((ref.mag_time >= ref.d_time.abs() * (1 - 1e-12)).all())


def test_library_exports_the_training_pair():
    from tempme_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tm_tgat_attn_train_fwd", "tm_tgat_attn_train_bwd", "tm_tgat_attn_train_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    wb = lib.tm_tgat_attn_train_workspace_bytes
    wb.restype = ctypes.c_int64
    wb.argtypes = [ctypes.c_int64, ctypes.c_int32]
    # one [2][d_time] partial per workgroup of four rows, at most 1024 workgroups however many rows
    assert wb(15, 8) == 4 * 4 * 2 * 8
    assert wb(4096, 172) == 1024 * 2 * 172 * 4
    assert 0 < wb(3 * 512 * 20, 172) <= 1024 * 2 * 172 * 4
    assert wb(0, 172) == 0 and wb(-1, 172) == -1


def test_model_has_the_training_interface():
    from tempme_amd.tgat import TGAT
    assert callable(getattr(TGAT, "train_on_hip", None)) and callable(getattr(TGAT, "draw_keep_masks", None))
    m = TT.build_model("small24", drop_out=0.1)
    assert m.train_on_hip() is m and m._train_on_hip is True
    assert m.train_on_hip(False)._train_on_hip is False


def test_learn_base_switch():
    from tempme_amd import learn_base
    with pytest.raises(NotImplementedError, match="--n_layer 2"):
        learn_base.main(["--base_type", "tgat", "--n_layer", "3", "-d", "uslegis_sampled"])
    with pytest.raises(NotImplementedError, match="tgn"):
        learn_base.main(["--base_type", "tgn", "-d", "uslegis_sampled"])
