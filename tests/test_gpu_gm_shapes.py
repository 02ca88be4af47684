"""Every GraphMixer kernel instance the channel width selects, on the device (the matrix: tests/gm_shape_inputs.py,
whose CPU half -- support table, instance coverage, the reference's own margin -- is tests/test_gm_shapes_cpu.py):

  tm_gm_embed       gm_fused_kernel<NC, NTT> for NC = 1..16 at N = 16 / 17, the ends N = 2 / 32, L = 0 / 4, edge_attr;
                    gm_embed_kernel<NMT, NTW>, all four, where a width is no multiple of 4
  tm_gm_embed_bwd   gm_bwd_kernel<NMT, NTW, TS8>, all four, up to the largest shape its LDS plan admits; the shapes
                    it refuses take the torch formulation

against the fp64 oracle (oracle/graphmixer_ref.py): logits atol 2e-5 + rtol 1e-5, d ew of a BCE loss within
1e-5 ||g64|| -- the margin the CPU half holds the fp32 torch formulation to -- and, at the narrow shapes where fp32
itself misses that, max(1e-4 ||g64||, 10 ||g32 - g64||) (check_grads' rule).  The tighter of the two matters: scaling
one tile slot of gm_bwd_kernel's second GEMM by 1.001 moves d ew by 2e-5 to 9e-5 ||g64||, which 1e-4 would let
through.  The profile proves which kernel family ran.  The training
pair's shapes (gm_shape_inputs.TRAIN) run in tests/test_gpu_gm_train.py."""
import numpy as np
import pytest
import torch

import gm_shape_inputs as S
from tests.test_gpu_graphmixer import ATOL, RTOL

pytestmark = pytest.mark.gpu
KERNELS = ("gm_fused_kernel", "gm_embed_kernel", "gm_bwd_kernel")
ids = lambda cs: [c.id for c in cs]  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


def model_on(case, dev):
    inp, sd, ea = S.build(case)
    m = S.make_model(inp, case.seed, dev).to(dev).eval()
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items()), "the seeded weights differ"
    return inp, m, None if ea is None else torch.from_numpy(ea).to(dev)


def contrast(m, inp, ew=None, ea=None):
    p, n = m.contrast(inp.src, inp.dst, inp.fake, inp.cut, None, *inp.sgs,
                      explain_weights=None if ew is None else [ew], edge_attr=ea)
    return torch.cat([p, n]).reshape(-1)


def profiled(fn):
    """fn() with the library's launch profile on -> (result, {kernel: launches} for the three GraphMixer kernels)."""
    from tempme_amd import _lib as L
    L.profile_enable(True)
    try:
        out = fn()
        prof = L.profile_read()
    finally:
        L.profile_enable(False)
    return out, {k: int(prof.get(k, (0.0, 0))[1]) for k in KERNELS}


def logit_ratio(got, ref, tag):
    """The worst |got - ref| / (ATOL + RTOL |ref|), asserted to be at most 1."""
    got, ref = got.detach().double().cpu().numpy(), ref.numpy()
    assert np.isfinite(got).all(), tag
    r = float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max())
    np.testing.assert_allclose(got, ref, atol=ATOL, rtol=RTOL, err_msg=tag)
    return r


def grad_ratio(case, ga):
    """||g_hip - g64|| over gm_shape_inputs.ew_grad_bound (1e-5 ||g64||; the narrow shapes check_grads' envelope),
    asserted to be at most 1."""
    g64 = S.oracle_ew_grad(case, torch.float64)[1]
    ga = ga.detach().double().cpu()
    err, nrm = float(torch.linalg.norm(ga - g64)), float(torch.linalg.norm(g64))
    bound = S.ew_grad_bound(case)
    print(f"{case.id}: d ew err {err:.3e} bound {bound:.3e} |g64| {nrm:.3e}")
    assert err <= bound, (case.id, err, bound)
    return err / bound


def forward_case(case, dev, kernel):
    inp, m, ea = model_on(case, dev)
    ew = torch.from_numpy(inp.ew0).to(dev)
    with torch.no_grad():
        (plain, weighted), prof = profiled(lambda: (contrast(m, inp, None, ea), contrast(m, inp, ew, ea)))
    other = "gm_embed_kernel" if kernel == "gm_fused_kernel" else "gm_fused_kernel"
    assert prof[kernel] == 2 and prof[other] == 0 and prof["gm_bwd_kernel"] == 0, prof
    assert getattr(m, "_gm_key", None) is not None, "the HIP embedding did not run"
    worst = 0.0
    for tag, got, w in (("ori", plain, None), ("expl", weighted, torch.from_numpy(inp.ew0).double())):
        # row 1 of every side has no valid neighbour: logits 1 and B + 1
        assert bool(torch.isfinite(got[[1, case.B + 1]]).all()), (case.id, tag)
        worst = max(worst, logit_ratio(got, S.oracle_logits(case, w, torch.float64), f"{case.id} {tag}"))
    print(f"{case.id}: {kernel} worst logit error / bound {worst:.4f}")


@pytest.mark.parametrize("case", S.FUSED, ids=ids(S.FUSED))
def test_fused_embedding_vs_oracle(dev, case):
    forward_case(case, dev, "gm_fused_kernel")


@pytest.mark.parametrize("case", S.FALLBACK, ids=ids(S.FALLBACK))
def test_fallback_embedding_vs_oracle(dev, case):
    forward_case(case, dev, "gm_embed_kernel")


def backward_case(case, dev):
    inp, m, _ = model_on(case, dev)
    ew = torch.from_numpy(inp.ew0).to(dev).requires_grad_(True)

    def step():
        logits = contrast(m, inp, ew)
        torch.nn.functional.binary_cross_entropy_with_logits(logits, S.bce_targets(case.B).to(dev)).backward()
        return logits

    logits, prof = profiled(step)
    r = logit_ratio(logits, S.oracle_ew_grad(case, torch.float64)[0], case.id)
    assert ew.grad is not None and bool(torch.isfinite(ew.grad).all())
    return m, inp, ew.grad, prof, r


@pytest.mark.parametrize("case", S.EW_BWD, ids=ids(S.EW_BWD))
def test_ew_backward_vs_oracle(dev, case):
    m, inp, g, prof, r = backward_case(case, dev)
    assert prof["gm_bwd_kernel"] == 1, prof
    assert getattr(m, "_gmb_key", None) is not None, "the HIP explanation-weight backward did not run"
    assert all(q.grad is None for k, q in m.named_parameters() if not k.startswith("affinity_score"))
    assert float(g.abs().cpu()[torch.from_numpy(inp.pad)].max()) == 0.0
    gr = grad_ratio(case, g)
    print(f"{case.id}: gm_bwd_kernel worst error / bound: logits {r:.4f}, d ew {gr:.4f}")


@pytest.mark.parametrize("case", S.EW_REFUSED, ids=ids(S.EW_REFUSED))
def test_refused_shapes_take_the_torch_formulation(dev, case):
    m, inp, g, prof, r = backward_case(case, dev)
    assert prof == {k: 0 for k in KERNELS}, prof
    assert getattr(m, "_gmb_key", None) is None and getattr(m, "_gm_key", None) is None
    assert float(g.abs().cpu()[torch.from_numpy(inp.pad)].max()) == 0.0
    gr = grad_ratio(case, g)
    print(f"{case.id}: torch formulation worst error / bound: logits {r:.4f}, d ew {gr:.4f}")
