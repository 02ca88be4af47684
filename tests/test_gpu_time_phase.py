"""GPU: every eval and training surface of the explainer with a NONZERO TimeEncode phase.

The constructor initialises phase to zero and every golden was made from it, so the rest of the suite runs
the time features at phase == 0, where cos(fma(t, w, 0)) is cos of the rounded product and a contracted time
argument, a wrong phase index, the slot-pass fold over cos(phase) and a stale pack or gate table after a
phase update are all invisible.  Here phase ~ N(0, 0.5) (phase_inputs.py) on the committed Enron walks (first
32 events, N = 20, timestamps up to 9.7e7), against oracle/encoder_ref.py carrying the same phase: the time
argument in fp32 with two roundings as the reference forms it, outputs in fp32 at rtol 1e-5 / atol 1e-6.
test_time_phase_cpu.py proves on the oracle alone that a single-rounding kernel misses these bounds by more
than 10x on >= 5 % of the walks and >= 50 % of the hop-1 slots.  The training kernels' perturbed legs live in
test_gpu_encoder_train.py / test_gpu_explain_train.py; the pooled encoder's are at the end of this file."""
import numpy as np
import pytest
import torch

import enron_inputs as EI
import phase_inputs as PI
from oracle import encoder_ref as er
from oracle import philox as px
from tests.test_gpu_parity import _Base

pytestmark = pytest.mark.gpu

RTOL, ATOL = PI.RTOL, PI.ATOL
N, E = PI.N_DEG, PI.N_EVENTS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z():
    return EI.golden()


@pytest.fixture(scope="module")
def g(z):
    return EI.graph(z)


@pytest.fixture(scope="module")
def d(z):
    return PI.enron_walks(z)


@pytest.fixture(scope="module")
def finder(dev, g):
    import tempme_amd as tm
    return tm.NeighborFinder.from_edges(g["src"], g["dst"], g["eidx"], g["ts"], g["n_nodes"], device=dev, seed=0,
                                        split=px.SPLIT_TEST)


_REF = {}


def _reference(z, g, d, tag, phase):
    """The fp32 oracle at ``phase`` on the golden walks, computed once per (weights, phase) and left unchanged."""
    key = (tag, phase.tobytes())
    if key not in _REF:
        _REF[key] = PI.enron_reference(PI.with_phase(EI.weights(z, tag), phase), g, d, tag[4:])
    return _REF[key]


def _explainer(dev, g, z, tag, phase):
    import tempme_amd as tm
    ctor = dict(out_dim=40, hid_dim=64)
    ctor.update(EI.VARIANTS[tag[4:]])
    ex = tm.TempME(_Base(g["n_feat"], g["e_feat"], dev), "tgn", "enron", device=dev, null_model=EI.null(z), **ctor)
    missing, unexpected = ex.load_state_dict(EI.weights(z, tag), strict=False)
    assert not unexpected
    ex = ex.to(dev).eval()
    PI.set_phase(ex, phase)
    return ex


def _phase(z, tag, seed=5):
    return PI.perturbed_phase(EI.weights(z, tag)["time_encoder.phase"].numel(), PI.SIGMA, seed)


def _dropin(ex, d):
    """TempME.forward x3 and retrieve_explanation(training=False) as eval_one_epoch calls them -> per side
    (imp [B, W, 1], hop-1 [B, N], hop-2 [B, N^2])."""
    imps, subs, walks = [], [], []
    for s in EI.SIDES:
        x = d[s]
        w = (x["node"], x["eid"], x["ts"], x["cat"], x["marg"])
        with torch.no_grad():
            imps.append(ex(w, d["ts_cut"], x["cnt"]))
        subs.append((x["sub_node"], x["sub_eid"], x["sub_ts"]))
        walks.append(w)
    with torch.no_grad():
        expl = ex.retrieve_explanation(subs[0], imps[0], walks[0], subs[1], imps[1], walks[1], subs[2], imps[2],
                                       walks[2], training=False)
    B = d["B"]
    e0 = expl[0].detach().cpu().numpy().reshape(3, B, -1)
    e1 = expl[1].detach().cpu().numpy().reshape(3, B, -1)
    return {s: (imps[k].detach().cpu().numpy(), e0[k], e1[k]) for k, s in enumerate(EI.SIDES)}


def _pipeline(dev, finder, z, ex, edge_table):
    from tempme_amd.pipeline import ExplainPipeline
    return ExplainPipeline(ex, finder.graph, torch.from_numpy(z["test_sampler_dst"]), N, 3, E, seed=0,
                           split=px.SPLIT_TEST, edge_table=edge_table)


def _run_pipeline(dev, pipe, z, d):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:E], dtype=dt)).to(dev)  # noqa: E731
    imp, h1, h2 = pipe.run(t(z["test_src"], np.int32), t(z["test_dst"], np.int32), t(z["test_ts"], np.float64),
                           t(z["test_eidx"], np.int32), torch.arange(E, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    pipe.check_errors()
    eid3 = pipe.buf.eid3.cpu().numpy()
    for k, s in enumerate(EI.SIDES):       # the pipeline sampled the golden walks (pinned in test_gpu_enron.py)
        assert np.array_equal(eid3[k], d[s]["eid"]), s
    imp, h1, h2 = imp.cpu().numpy(), h1.cpu().numpy(), h2.cpu().numpy()
    return {s: (imp[k][..., None], h1[k], h2[k]) for k, s in enumerate(EI.SIDES)}


def _check(got, ref, what):
    for s in EI.SIDES:
        for name, a, b in zip(("imp", "expl0", "expl1"), got[s], ref[s]):
            err = np.abs(a - b) / PI.tol(b)
            print(what, s, name, "max |got - oracle| / tol = %.3f" % err.max())
    for s in EI.SIDES:
        for name, a, b in zip(("imp", "expl0", "expl1"), got[s], ref[s]):
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, err_msg=f"{what} {s} {name}")


def _moved(a, b):
    """Shares of walks / nonzero hop-1 slots that differ beyond the tolerance between two results."""
    imp = np.concatenate([(np.abs(a[s][0] - b[s][0]) > PI.tol(b[s][0])).reshape(-1) for s in EI.SIDES])
    nz = np.concatenate([(b[s][1] != 0).reshape(-1) for s in EI.SIDES])
    h1 = np.concatenate([(np.abs(a[s][1] - b[s][1]) > PI.tol(b[s][1])).reshape(-1) for s in EI.SIDES])
    return float(imp.mean()), float(h1[nz].mean())


# ------------------------------------------------------------------ a. the drop-in eval surface
# N20_base: register-resident walk_kernel, gate_pos_kernel; N20_h32: LDS-tiled gcn_kernel / head_kernel;
# notg: the plain Attention; nodep: no dependency gate
@pytest.mark.parametrize("tag", ["N20_base", "N20_h32", "N20_notg", "N20_nodep"])
def test_dropin_eval_perturbed_phase(dev, g, z, d, tag):
    ph = _phase(z, tag)
    ex = _explainer(dev, g, z, tag, ph)
    got = _dropin(ex, d)
    assert ex._packed is not None, "the HIP encoder did not run"
    _check(got, _reference(z, g, d, tag, ph), tag)


# ------------------------------------------------------------------ b. the fused pipeline
# edge_table=True: table-mode walk_kernel with the evc / devc fold over cos(phase), gate_table_kernel,
# explain_tab_kernel; False: lin_event's edge product inside the walk kernel, gate_reg_kernel
@pytest.mark.parametrize("edge_table", [True, False])
def test_pipeline_perturbed_phase(dev, finder, g, z, d, edge_table):
    tag = "N20_base"
    ph = _phase(z, tag)
    ex = _explainer(dev, g, z, tag, ph)
    got = _run_pipeline(dev, _pipeline(dev, finder, z, ex, edge_table), z, d)
    _check(got, _reference(z, g, d, tag, ph), f"pipeline edge_table={edge_table}")


# ------------------------------------------------------------------ c. phase changes between calls
@pytest.mark.parametrize("surface", ["dropin", "pipeline_table", "pipeline_no_table"])
def test_phase_update_between_calls_is_followed(dev, finder, g, z, d, surface):
    """An in-place update of phase as an optimizer makes it (no_grad add_): the next call must repack the
    weights and rebuild the per-edge-id gate / lin_event tables.  The second result is checked against the
    oracle at the new phase, and it differs from the first beyond the tolerance on most walks and hop-1
    slots, so a stale pack or table cannot pass."""
    tag = "N20_base"
    ph = _phase(z, tag)
    ex = _explainer(dev, g, z, tag, ph)
    if surface == "dropin":
        run = lambda: _dropin(ex, d)  # noqa: E731
    else:
        pipe = _pipeline(dev, finder, z, ex, surface == "pipeline_table")
        run = lambda: _run_pipeline(dev, pipe, z, d)  # noqa: E731
    first = run()
    _check(first, _reference(z, g, d, tag, ph), surface + " before")
    delta = PI.perturbed_phase(ph.size, PI.SIGMA, seed=6)
    with torch.no_grad():
        ex.time_encoder.phase.add_(torch.from_numpy(delta).to(dev))
    ph2 = ex.time_encoder.phase.detach().cpu().numpy()
    assert np.array_equal(ph2, ph + delta)
    second = run()
    _check(second, _reference(z, g, d, tag, ph2), surface + " after")
    imp_moved, h1_moved = _moved(second, first)
    print(surface, "moved beyond tol: walks %.3f, nonzero hop-1 slots %.3f" % (imp_moved, h1_moved))
    assert imp_moved > 0.5 and h1_moved > 0.5


# ------------------------------------------------------------------ d. after a real training step
def test_eval_after_train_step_matches_oracle(dev, g, z):
    """The golden training iteration (test_train_step_matches_reference_enron's step, goldens unchanged) leaves
    phase at about +-1e-3, the regime of every user after step one; then eval forward and explanation on the
    same walks against the oracle fed the explainer's own state dict."""
    from tests.test_gpu_enron import _golden_train_step
    ex, out, p0, dd = _golden_train_step(dev, g, z)
    ph = ex.time_encoder.phase.detach().cpu().numpy()
    moved = np.abs(ph - p0["time_encoder.phase"].cpu().numpy())
    print("phase after one Adam step: max |phase| %.2e, entries moved %d / %d" % (np.abs(ph).max(), (moved > 0).sum(),
                                                                                  ph.size))
    assert np.abs(ph).max() > 1e-4 and (moved > 1e-4).mean() > 0.5
    ex.eval()
    got = _dropin(ex, dd)
    sd = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    _check(got, PI.enron_reference(sd, g, dd), "after train step")


# ------------------------------------------------------------------ f. the pooled encoder (enhance_predict_*)
def test_enhance_predict_agg_eval_perturbed_phase(dev):
    """enhance_predict_agg (eval, no gradients: walk_pool_kernel / pool_tail_kernel) against tests/enhance_ref.py
    at the smallest seeded shape with Enron-range timestamps; tolerance 10x the restatement's own
    fp32-vs-fp64 distance, the convention of test_gpu_enhance.py."""
    import enhance_ref as XR
    dd = PI.enhance_inputs(3, 4, 12)
    sides, gats = PI.enhance_sides(dd)
    ex = PI.enhance_explainer(dd, dev).eval()
    sd = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    ref = lambda s: torch.cat(XR.predict_agg(s, dd["n_feat"], dd["e_feat"], dd["deg"], dd["cut"], sides, gats)[:2])  # noqa: E731
    r32, r64 = ref(sd).double(), ref({k: v.double() for k, v in sd.items()})
    tol = 10 * float((r32 - r64).abs().max())
    with torch.no_grad():
        pos, neg = ex.enhance_predict_agg(dd["cut"], sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides],
                                          *[x.to(dev) for x in gats])
    dist = float((torch.cat([pos, neg]).cpu().double() - r64).abs().max())
    print("enhance_predict_agg logits", dist, "tolerance", tol)
    assert dist <= tol


def test_enhance_train_groups_perturbed_phase(dev):
    """enhance_train_groups forward + backward (gcn_kernel / head_pool_train_kernel / head_pool_bwd_kernel /
    gcn_bwd_kernel) against fp64 autograd through tests/enhance_train_ref.py with the same keep-masks; shapes,
    masks, upstream gradient and tolerances as test_gpu_enhance_train.test_backward_matches_fp64_autograd."""
    import enhance_train_ref as TR
    dd = PI.enhance_inputs(2, 3, 7)
    ex = PI.enhance_explainer(dd, dev).train()
    sd = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    G, B, W = dd["G"], dd["B"], dd["W"]
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    cut = to(dd["cut"], torch.float64).reshape(1, -1).expand(G, -1).contiguous()
    args = (to(dd["node"], torch.int32), to(dd["eid"], torch.int32), to(dd["ts"], torch.float32),
            to(dd["cat"], torch.int32), cut, to(dd["cnt"], torch.float32), G, B, W)
    rng = np.random.default_rng(11)
    drop = torch.from_numpy((rng.uniform(0, 1, (G * B * W, ex.dropout_cols())) >= 0.5).astype(np.uint8))
    d_emb = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (G, B, ex.mlp_dim)).astype(np.float32))
    e32, g32 = TR.forward_and_grads(sd, dd, d_emb, True, True, drop, 2.0, torch.float32)
    e64, g64 = TR.forward_and_grads(sd, dd, d_emb, True, True, drop, 2.0, torch.float64)
    ex.zero_grad()
    emb = ex.enhance_train_groups(*args, drop=drop.to(dev), drop_scale=2.0, use_module_dropout=False)
    (emb * d_emb.to(dev)).sum().backward()
    grads = {k: p.grad.detach().cpu() for k, p in ex.named_parameters() if p.grad is not None}
    tol = 10 * float((e32.double() - e64).abs().max())
    dist = float((emb.detach().cpu().double() - e64).abs().max())
    print("emb", dist, "tolerance", tol)
    missed = [("emb", dist, tol)] if not dist <= tol else []
    for k in TR.POOL_PARAMS:
        gt = 10 * float((g32[k].double() - g64[k]).abs().max())
        dg = float((grads[k].double() - g64[k]).abs().max())
        print("grad", k, dg, "tolerance", gt)
        if not dg <= gt:
            missed.append((k, dg, gt))
    assert not missed, missed
