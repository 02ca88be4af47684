"""CPU conditions of the nonzero-phase GPU tests, on the references alone: on the very inputs those tests use,
(1) the fp32 oracle is far inside the tolerance of its fp64 self, so the GPU tests' bounds are about the
kernels, and (2) a kernel that forms the time argument t * w + phase with ONE rounding (a fused multiply-add,
modelled by phase_inputs.single_rounding) would miss those bounds widely.  Together: the GPU cases fail on a
contracted time argument and pass only on the reference's two roundings.

The floors are half of what the oracle measures (figures in each test's docstring)."""
import numpy as np
import pytest
import torch

import enron_inputs as EI
import phase_inputs as PI
from oracle import encoder_ref as er


@pytest.fixture(scope="module")
def z():
    return EI.golden()


@pytest.fixture(scope="module")
def g(z):
    return EI.graph(z)


@pytest.fixture(scope="module")
def d(z):
    return PI.enron_walks(z)


def test_set_phase_bumps_the_version_and_data_copy_does_not():
    """packed_weights() keys on (data_ptr, _version): set_phase must change the key, and the hazard it avoids
    (a write through .data) is real."""
    p = torch.nn.Parameter(torch.zeros(8))

    class Ex:
        class time_encoder:
            phase = p
    v0 = p._version
    PI.set_phase(Ex, PI.perturbed_phase(8))
    assert p._version > v0 and np.array_equal(p.detach().numpy(), PI.perturbed_phase(8))
    v1 = p._version
    p.data.copy_(torch.ones(8))
    assert p._version == v1


def test_single_rounding_is_the_two_rounding_argument_at_zero_phase():
    """Why the zero-phase suite cannot see the defect: with phase == 0 both forms give the rounded product."""
    rng = np.random.RandomState(0)
    t = torch.from_numpy(rng.uniform(0, 1e8, 4096).astype(np.float32))
    sd = {"time_encoder.basis_freq": torch.from_numpy((1 / 10 ** np.linspace(0, 9, 172)).astype(np.float32)),
          "time_encoder.phase": torch.zeros(172)}
    assert torch.equal(PI.single_rounding(sd, t), er.time_encode(sd, t))
    sd = PI.with_phase(sd, PI.perturbed_phase(172))
    diff = (PI.single_rounding(sd, t) - er.time_encode(sd, t)).abs()
    assert float(diff.max()) > 1e-2


# measured (max over the three sides of the fp32-vs-fp64 distance / tol; min over the sides of the shares):
#   tag        fp64   imp share > 10 tol   hop-1 share > 10 tol
#   N20_base   0.015  0.097                0.828
#   N20_h32    0.015  0.026                0.883
#   N20_notg   0.016  0.163                0.827
#   N20_nodep  0.014  0.179                0.172   (no gate: hop-1 moves only through imp)
FLOORS = {"N20_base": (0.05, 0.50), "N20_h32": (0.013, 0.44), "N20_notg": (0.08, 0.41), "N20_nodep": (0.085, 0.085)}


@pytest.mark.parametrize("tag", sorted(FLOORS))
def test_enron_inputs_discriminate_a_single_rounding(z, g, d, tag):
    """Per side, at phase ~ N(0, 0.5) on the first 32 Enron events: the fp32 oracle within 0.1 tol of the fp64
    oracle for imp and both explanation outputs; the single-rounding oracle beyond 10 tol on >= 5 % of the walks
    (imp) and >= 50 % of the nonzero hop-1 slots for the default constructor (measured 9.7-11 % and 83-86 %),
    and beyond half the measured share for the variants (table above)."""
    var = tag[4:]
    sd = PI.with_phase(EI.weights(z, tag), PI.perturbed_phase(EI.weights(z, tag)["time_encoder.phase"].numel()))
    r32 = PI.enron_reference(sd, g, d, var)
    r64 = PI.enron_reference(sd, g, d, var, torch.float64)
    with PI.oracle_time_encode(PI.single_rounding):
        r1 = PI.enron_reference(sd, g, d, var)
    imp_floor, hop1_floor = FLOORS[tag]
    for s in EI.SIDES:
        for k, name in enumerate(("imp", "expl0", "expl1")):
            own = np.abs(r64[s][k] - r32[s][k]) / PI.tol(r32[s][k])
            print(tag, s, name, "fp32 vs fp64 oracle, max / tol: %.4f" % own.max())
            assert own.max() <= 0.1, (s, name)
        far = [np.abs(r1[s][k] - r32[s][k]) > 10 * PI.tol(r32[s][k]) for k in range(2)]
        nz = r32[s][1] != 0
        print(tag, s, "single rounding beyond 10 tol: imp %.3f, hop-1 %.3f" % (far[0].mean(), far[1][nz].mean()))
        assert far[0].mean() >= imp_floor, s
        assert far[1][nz].mean() >= hop1_floor, s


def _grads(fn, sd0, names, dtype, loss_of):
    sd = {k: v.detach().to(dtype).requires_grad_(k in names) for k, v in sd0.items()}
    with PI.oracle_time_encode(fn):
        loss_of(sd).backward()
    return {k: sd[k].grad.double() for k in names}


def _moves(one, two):
    return {k: float((one[k] - two[k]).norm() / two[k].norm()) for k in two}


@pytest.mark.parametrize("de,G,B,N,zn", [(32, 3, 20, 20, False), (1, 2, 7, 5, False), (32, 1, 9, 20, False),
                                         (32, 3, 20, 20, True), (172, 2, 11, 20, False)])
def test_encoder_training_inputs_discriminate_a_single_rounding(de, G, B, N, zn):
    """test_gpu_encoder_train's synthetic inputs (dt up to 1e6) and seeded explainer, phase ~ N(0, 0.5), fp64
    autograd without dropout: a single-rounding argument moves at least three of the 22 gradients by >= 1e-2 of
    their norm, 50 times that test's 2e-4 bound.  Measured: 19 / 15 / 18 / 20 / 8 tensors beyond 1e-2 for the
    five shapes, the largest by 2.4e-2 .. 6.7e-2."""
    from tempme_amd import TempME
    from tests.test_gpu_encoder_train import PARAMS, _Base, _inputs
    n_feat, e_feat, node6, eid3, ts3, cat, cut, cnt = _inputs(de, G, B, N, seed=de + G + B, zero_nodes=zn)
    torch.manual_seed(7)
    ex = TempME(_Base(n_feat, e_feat), "tgn", "synth", 40, 64, null_model={k: 1 / 12 for k in range(1, 13)})
    PI.set_phase(ex, PI.perturbed_phase(ex.time_encoder.phase.numel()))
    wts = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, G * B * 3 * N)).double()
    nf, ef = torch.from_numpy(n_feat), torch.from_numpy(e_feat)

    def loss_of(sd):
        out = torch.cat([er.forward(sd, nf, ef, node6[k], eid3[k], ts3[k], cat[k], cut[k], cnt[k]).reshape(-1)
                         for k in range(G)])
        return (out * wts).sum()
    sd0 = ex.state_dict()
    mv = _moves(_grads(PI.single_rounding, sd0, PARAMS, torch.float64, loss_of),
                _grads(er.time_encode, sd0, PARAMS, torch.float64, loss_of))
    print(sorted(((round(v, 4), k) for k, v in mv.items()), reverse=True))
    assert sum(v >= 1e-2 for v in mv.values()) >= 3, mv


GATE_MOVED = ("edge_dependency_gcn.0.weight", "edge_dependency_gcn.0.bias", "edge_dependency_gcn.3.weight",
              "edge_dependency_gcn.3.bias", "time_encoder.basis_freq", "time_encoder.phase")


@pytest.mark.parametrize("de,G,B,N", [(32, 3, 12, 20), (1, 2, 5, 5), (32, 1, 7, 10)])
def test_gate_training_inputs_discriminate_a_single_rounding(de, G, B, N):
    """The gate path (edge_importance_train, absolute timestamps up to 1e6) on test_gpu_explain_train's inputs
    and seeded explainer, phase ~ N(0, 0.5), fp32 autograd without dropout: a single-rounding argument moves
    each of the six tensors of GATE_MOVED by >= 1e-2 of its norm, 500 times that test's 2e-5 bound, so its
    timestamps need no rescaling.  Measured, smallest over the three shapes: gcn.0.weight 3.9e-2, gcn.0.bias
    3.4e-2, gcn.3.weight 2.1e-2, gcn.3.bias 2.1e-2, basis_freq 5.5e-2, phase 4.5e-2 (floor: half the smallest);
    gcn.6.weight moves 3e-3 and gcn.6.bias 1e-5, and the outputs by at most 15-19 tol on 1-9 % of the slots.
    With the timestamps at 1e8 every figure grows tenfold (2e-1 .. 4.5e-1)."""
    from tempme_amd import TempME
    from tests.test_gpu_explain_train import GATE, _Base, _explain_inputs
    n_feat, e_feat, eid3, ts3, s1e, s2e, imp_np, w1, w2 = _explain_inputs(de, G, B, N)
    torch.manual_seed(9)
    ex = TempME(_Base(n_feat, e_feat), "tgn", "synth", 40, 64, null_model={k: 1 / 12 for k in range(1, 13)})
    PI.set_phase(ex, PI.perturbed_phase(ex.time_encoder.phase.numel()))
    ef, imp = torch.from_numpy(e_feat), torch.from_numpy(imp_np)

    def loss_of(sd):
        loss = 0
        for k in range(G):
            r1, r2 = er.edge_importance_train(sd, ef, imp[k].unsqueeze(-1), eid3[k], ts3[k], [s1e[k], s2e[k]])
            loss = loss + (r1.reshape(-1) * w1.reshape(G, -1)[k]).sum() + (r2.reshape(-1) * w2.reshape(G, -1)[k]).sum()
        return loss
    sd0 = ex.state_dict()
    mv = _moves(_grads(PI.single_rounding, sd0, GATE, torch.float32, loss_of),
                _grads(er.time_encode, sd0, GATE, torch.float32, loss_of))
    print({k: "%.2e" % v for k, v in mv.items()})
    for k in GATE_MOVED:
        assert mv[k] >= 1e-2, (k, mv[k])


def test_enhance_inputs_discriminate_a_single_rounding():
    """The pooled encoder's perturbed-phase cases (Enron-range timestamps): a single-rounding argument moves
    enhance_predict_agg's logits by >= 100 times their tolerance (measured 790) and the training embeddings and
    every gradient but attention.MLP.3.bias (the output bias: d emb alone) by >= 1000 times theirs (measured
    2900 for the embeddings, 3400 .. 94000 for the gradients).  At the original timestamps (below 60) the
    logits move by 0.06 of their tolerance: those shapes had to be rescaled."""
    import enhance_ref as XR
    import enhance_train_ref as TR
    dd = PI.enhance_inputs(3, 4, 12)
    sides, gats = PI.enhance_sides(dd)
    sd = {k: v.detach() for k, v in PI.enhance_explainer(dd).state_dict().items()}
    ref = lambda s: torch.cat(XR.predict_agg(s, dd["n_feat"], dd["e_feat"], dd["deg"], dd["cut"], sides, gats)[:2]).double()  # noqa: E731
    r32, r64 = ref(sd), ref({k: v.double() for k, v in sd.items()})
    with PI.oracle_time_encode(PI.single_rounding, XR):
        r1 = ref(sd)
    tol = 10 * float((r32 - r64).abs().max())
    print("agg: tolerance", tol, "single rounding moves", float((r1 - r32).abs().max()))
    assert float((r1 - r32).abs().max()) >= 100 * tol

    dd = PI.enhance_inputs(2, 3, 7)
    sd = {k: v.detach() for k, v in PI.enhance_explainer(dd).state_dict().items()}
    d_emb = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (dd["G"], dd["B"], 76)).astype(np.float32))
    e32, g32 = TR.forward_and_grads(sd, dd, d_emb, True, True, None, 1.0, torch.float32)
    e64, g64 = TR.forward_and_grads(sd, dd, d_emb, True, True, None, 1.0, torch.float64)
    with PI.oracle_time_encode(PI.single_rounding, XR):
        e1, g1 = TR.forward_and_grads(sd, dd, d_emb, True, True, None, 1.0, torch.float64)
    tol = 10 * float((e32.double() - e64).abs().max())
    assert float((e1 - e64).abs().max()) >= 1000 * tol
    for k in TR.POOL_PARAMS:
        if k == "attention.MLP.3.bias":
            continue
        gt = 10 * float((g32[k].double() - g64[k]).abs().max())
        ratio = float((g1[k] - g64[k]).abs().max()) / gt
        print(k, "single rounding moves the gradient by %.0f tolerances" % ratio)
        assert ratio >= 1000, k
