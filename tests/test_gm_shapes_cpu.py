"""The GraphMixer shape matrix (tests/gm_shape_inputs.py) without a GPU: the support predicates of the library place
every case on the kernel family it is listed under, the listed shapes cover every template instance, and the fp32
torch formulation alone stays well inside the tolerances the GPU tests (tests/test_gpu_gm_shapes.py) hold the
kernels to -- so a kernel that misses them is wrong, not unlucky with its inputs."""
import pytest
import torch

import gm_shape_inputs as S
import gm_train_ref as GR

ATOL, RTOL = 2e-5, 1e-5          # the GPU tests' logit tolerance (tests/test_gpu_graphmixer.py)
ALL_EVAL = S.FUSED + S.FALLBACK + S.EW_BWD + S.EW_REFUSED
ids = lambda cs: [c.id for c in cs]  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    import tempme_amd
    return tempme_amd.lib()


def fused_ok(lib, c):
    return bool(lib.tm_gm_fused_ok(c.N, c.C, c.T, S.dims(c.N, c.C)[1]))


def bwd_ok(lib, c):
    return bool(lib.tm_gm_embed_bwd_ok(c.N, c.C, c.T, c.L, S.dims(c.N, c.C)[0] if c.L else 0))


def test_case_ids_are_unique():
    for cs in (S.FUSED, S.FALLBACK, S.EW_BWD, S.EW_REFUSED):
        assert len(set(ids(cs))) == len(cs)
    assert [S.fused_width(nc) for nc in (1, 2, 3, 4, 15, 16)] == [4, 32, 36, 64, 228, 256]
    assert len(set(S.TRAIN)) == len(S.TRAIN)


def test_support_table(lib):
    for c in S.FUSED:
        assert fused_ok(lib, c), c.id
    for c in S.FALLBACK:
        assert not fused_ok(lib, c), c.id
    for c in S.EW_BWD:
        assert bwd_ok(lib, c), c.id
    for c in S.EW_REFUSED:
        assert not bwd_ok(lib, c), c.id
    for N, C, T, L, p, B in S.TRAIN:
        assert lib.tm_gm_train_ok(N, C, T, L, *S.dims(N, C)), (N, C, T, L)
    # every case is within what the model itself sends to the HIP path (GraphMixer._hip_mode)
    for c in ALL_EVAL:
        assert 2 <= c.N <= 32 and S.dims(c.N, c.C)[0] <= 16 and 0 <= c.L <= 4 and c.C <= 256, c.id


def test_backward_lds_boundary(lib):
    """tm_gm_embed_bwd_ok's LDS plan: C > 192 (r16(C) >= 208) only with one layer, C = 240 = T the widest that fits,
    at C = 256 nothing with a mixer layer (L = 0, three images, is the only plan that fits)."""
    ht = 8
    assert lib.tm_gm_embed_bwd_ok(16, 240, 240, 1, ht) and not lib.tm_gm_embed_bwd_ok(16, 240, 240, 2, ht)
    assert not lib.tm_gm_embed_bwd_ok(16, 241, 240, 1, ht)
    assert lib.tm_gm_embed_bwd_ok(16, 193, 4, 1, ht) and not lib.tm_gm_embed_bwd_ok(16, 193, 4, 2, ht)
    assert lib.tm_gm_embed_bwd_ok(16, 192, 192, 2, ht)
    for T in (0, 4, 20, 256):
        for L in range(1, 5):
            assert not lib.tm_gm_embed_bwd_ok(16, 256, T, L, ht), (T, L)
    assert lib.tm_gm_embed_bwd_ok(16, 256, 20, 0, 0)


def test_every_instance_is_covered(lib):
    fused = {(S.instance(c.N, c.C).NC, S.instance(c.N, c.C).NTT) for c in S.FUSED}
    assert fused == {(nc, ntt) for nc in range(1, 17) for ntt in (1, 2)}
    # both register budgets of gm_fused_kernel (amdgpu_waves_per_eu(NC <= 13 ? 3 : 2))
    assert {nc for nc, _ in fused if nc > 13} == {14, 15, 16}
    four = {(m, w) for m in (1, 2) for w in (3, 4)}
    assert {(S.instance(c.N, c.C).NMT, S.instance(c.N, c.C).NTW) for c in S.FALLBACK} == four
    assert {(S.instance(c.N, c.C).NMT, S.instance(c.N, c.C).NTW) for c in S.EW_BWD} == four
    # the training kernels' fourth tile slot (i = 3 of wave + 4 i < NT) holds a value only above 12 tiles
    assert sum((C + 15) // 16 > 12 for _, C, *_ in S.TRAIN) >= 3
    assert any(T < C for _, C, T, *_ in S.TRAIN)
    assert {2, 32} <= {N for N, *_ in S.TRAIN} and 4 in {L for _, _, _, L, *_ in S.TRAIN}
    # the first named training shape: 13 tiles, a ragged last hidden chunk
    N, C, T, L, p, B = S.TRAIN[0]
    assert (C + 15) // 16 == 13 and S.dims(N, C)[1] == 6 * 128 + 16


@pytest.mark.parametrize("case", ALL_EVAL, ids=ids(ALL_EVAL))
def test_reference_margin(case):
    """fp32 against fp64 through oracle.graphmixer_ref.contrast, without and with explanation weights: logits within
    a tenth of the GPU tolerance; d ew of the BCE loss within 1e-5 ||g64||, or -- where fp32 cannot reach that
    (gm_shape_inputs.narrow: C = 2 and N = 2 give 1.3e-5 to 3.3e-5 with seed 0) -- the x10 envelope of check_grads,
    itself capped at 3e-4 ||g64||.  Each case's seed (gm_shape_inputs._SEEDS) was picked so that this holds with room
    to spare on any thread count."""
    inp = S.build(case)[0]
    worst = 0.0
    for with_ew in (False, True):
        l32, l64 = (S.oracle_logits(case, torch.from_numpy(inp.ew0).to(dt) if with_ew else None, dt)
                    for dt in (torch.float32, torch.float64))
        assert bool(torch.isfinite(l64).all())
        r = float(((l32.double() - l64).abs() / (0.1 * (ATOL + RTOL * l64.abs()))).max())
        worst = max(worst, r)
        assert r <= 1.0, (case.id, with_ew, r)
    (_, g32), (_, g64) = S.oracle_ew_grad(case, torch.float32), S.oracle_ew_grad(case, torch.float64)
    err, nrm = float(torch.linalg.norm(g32.double() - g64)), float(torch.linalg.norm(g64))
    print(f"{case.id}: logits {worst:.3f} of a tenth of the tolerance, d ew fp32 - fp64 {err / nrm:.3e} relative")
    assert nrm > 0 and float(g64.abs()[torch.from_numpy(inp.pad)].max()) == 0.0
    # no unit of the score's ReLU within the logit tolerance of its kink: an embedding that is right to that
    # tolerance cannot take the other side of it, where d ew jumps
    assert S.relu_margin(case) >= ATOL, (case.id, S.relu_margin(case))
    if S.narrow(case):
        assert 10 * err <= 3e-4 * nrm, (case.id, err / nrm)
        assert S.ew_grad_bound(case) == max(1e-4 * nrm, 10 * err)
    else:
        assert err <= 1e-5 * nrm, (case.id, err / nrm)
        assert S.ew_grad_bound(case) == 1e-5 * nrm


@pytest.mark.parametrize("N,C,T,L,p,B", S.TRAIN)
def test_training_reference_margin(N, C, T, L, p, B):
    """gm_train_ref.loss_and_grads in fp32 against fp64 on make_case's inputs and weights (tests/test_gpu_gm_train.py;
    the keep masks here are a CPU draw of the same rate): logits within a tenth of the GPU tolerance, and for every
    parameter the x10 envelope of check_grads at most 3e-4 ||g64||, so that it cannot hide a wrong kernel."""
    inp = S.make_inputs(N, C, T, L, B, seed=N + C + L, V=S.TRAIN_V, E=S.TRAIN_E)
    sd = S.make_model(inp, N + L, "cpu", dropout=p).state_dict()
    HT, HC = S.dims(N, C)
    keep = None
    if p > 0:
        keep = torch.empty(L * 3 * B * (C * HT + C * N + N * HC + N * C), dtype=torch.uint8).bernoulli_(
            1.0 - p, generator=torch.Generator().manual_seed(N + C))
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    batch = (inp.src, inp.dst, inp.fake, inp.cut, *inp.sgs)
    _, p64, n64, g64 = GR.loss_and_grads(sd, L, batch, keep, scale, torch.float64)
    _, p32, n32, g32 = GR.loss_and_grads(sd, L, batch, keep, scale, torch.float32)
    l64, l32 = torch.cat([p64, n64]), torch.cat([p32, n32]).double()
    r = float(((l32 - l64).abs() / (0.1 * (ATOL + RTOL * l64.abs()))).max())
    assert r <= 1.0, r
    worst = 0.0
    for k, ref in g64.items():
        nrm = float(torch.linalg.norm(ref))
        err = float(torch.linalg.norm(g32[k].double() - ref))
        worst = max(worst, err / nrm if nrm > 0 else 0.0)
        assert 10 * err <= 3e-4 * nrm, (k, err, nrm)
    print(f"logits {r:.3f} of a tenth of the tolerance, worst parameter gradient fp32 - fp64 {worst:.3e} relative")
