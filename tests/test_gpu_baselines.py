"""The baseline explainers on the device (tempme_amd/baselines.py) and ``attention_weights`` of the two attention-based
base models, on the uslegis batch of tgn_inputs at B = 8 (the golden's batch) and B = 32, N = 20.

``attention_weights`` is held to the probabilities hooks on the reference's attention modules recorded
(tests/golden/attn_probs_uslegis.npz): tolerance 10 x max |p32 - p64| of the golden itself, at least 1e-6
(attn_probs_ref.golden_tol: TGN hop-1 1.1e-5, hop-2 1.7e-5; TGAT hop-1 2.0e-5, hop-2 1.8e-5).  Measured on an MI355X:
TGN hop-1 5.4e-7, hop-2 3.9e-7; TGAT hop-1 1.07e-6, hop-2 3.0e-7 from the reference's fp64 run.
Everything else here is exact: bit-equal logits, bit-equal gradients, equal figures.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_probs_ref as AP
import tgat_inputs as TA
import tgn_inputs as TI
from tests.test_graphmixer_oracle import build as build_graphmixer

pytestmark = pytest.mark.gpu

CASE = "uslegis"
RATIOS = [0.05, 0.2, 0.6]
BASES = ("tgn", "tgat", "graphmixer")
_models = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


def model(base, dev):
    if base not in _models:
        m = {"tgn": lambda: TI.build_model(CASE), "tgat": lambda: TA.build_model(CASE),
             "graphmixer": lambda: build_graphmixer(CASE)}[base]()
        _models[base] = m.to(dev).eval()
    return _models[base]


def make_batch(B):
    from tempme_amd.train import Batch
    d = TI.load_batch(bsz=B)
    return Batch(d["src"], d["dst"], d["ts_cut"], d["e_idx"], d["fake"], [d["sg_src"], d["sg_tgt"], d["sg_bgd"]],
                 None, None), d


def sides(b):
    return (b.src, b.dst, b.fake, b.ts) + tuple(b.subgraphs)


def args_for(base, N=TI.N_DEG, B=8):
    return SimpleNamespace(base_type=base, n_degree=N, bs=B, ratios=RATIOS, seed=5)


def contrast(base, m, b, w=None):
    a = (b.src, b.dst, b.fake, b.ts, b.e_idx) + tuple(b.subgraphs)
    if base == "tgat":
        if w is None:
            return m.contrast(*a, test=True, if_explain=False)
        return m.contrast(*a, test=True, if_explain=True, stacked_weights=tuple(w))
    return m.contrast(*a, explain_weights=w)


def records(b, dev, hops):
    from tempme_amd import baselines
    return baselines.node_records(b, dev, hops)


# ------------------------------------------------------------------ 1. attention_weights
@pytest.mark.parametrize("base", ["tgn", "tgat"])
def test_attention_weights_match_the_reference(dev, base):
    from tempme_amd import _lib as L
    g = AP.golden()
    m = model(base, dev)
    b, d = make_batch(AP.GOLDEN_B)
    B, N = d["B"], d["N"]
    with torch.no_grad():
        before = torch.cat(contrast(base, m, b))
    L.profile_enable(True)
    h1, h2 = m.attention_weights(*sides(b))
    prof = L.profile_read()
    L.profile_enable(False)
    with torch.no_grad():
        after = torch.cat(contrast(base, m, b))
    m.check_errors()
    H = g[f"{base}_hop1_64"].shape[1]
    assert tuple(h1.shape) == (3 * B, H, N) and tuple(h2.shape) == (3 * B * N, H, N)
    assert h1.dtype == h2.dtype == torch.float32 and h1.device == dev and not h1.requires_grad
    for tag, got in (("hop1", h1), ("hop2", h2)):
        name = f"{base}_{tag}"
        tol = AP.golden_tol(g, name)
        err = float(np.abs(got.cpu().double().numpy() - g[name + "_64"]).max())
        print(name, "max |p - reference fp64|", err, "tol", tol)
        assert err <= tol
        assert float(np.abs(got.cpu().numpy() - g[name + "_32"]).max()) <= tol
    # the default path is untouched: bit-equal logits around the call, and exactly two launches of the new kernel
    assert torch.equal(before, after)
    label = f"{base}_attn_probs_kernel"
    assert prof[label][1] == 2 and sum(v[1] for k, v in prof.items() if k.endswith("_attn_probs_kernel")) == 2
    assert prof[f"{base}_attn_fwd_kernel"][1] == (2 if base == "tgn" else 3)
    # a contrast launches none
    L.profile_enable(True)
    with torch.no_grad():
        contrast(base, m, b)
    prof = L.profile_read()
    L.profile_enable(False)
    assert not any(k.endswith("_attn_probs_kernel") for k in prof)
    # the head means are the kernel's second output, and prepared inputs give the same bits
    m1, m2 = m.attention_weights(*sides(b), head_mean=True)
    assert np.array_equal(m1.cpu().numpy(), AP.head_mean32(h1.cpu().numpy()))
    assert np.array_equal(m2.cpu().numpy(), AP.head_mean32(h2.cpu().numpy()))
    prep = m.prepare_contrast(*sides(b))
    p1, p2 = m.attention_weights(*sides(b), prepared=prep)
    assert torch.equal(p1, h1) and torch.equal(p2, h2)


def test_attention_weights_of_a_stateful_tgn_raise(dev):
    m = TI.build_model(CASE).to(dev)
    m.forbidden_memory_update = False
    b, _ = make_batch(8)
    with pytest.raises(NotImplementedError, match="forbidden_memory_update=False"):
        m.attention_weights(*sides(b))


def test_attention_weights_of_a_training_tgat_raise(dev):
    m = TA.build_model(CASE).to(dev)
    m.train()
    b, _ = make_batch(8)
    with pytest.raises(NotImplementedError, match="training mode"):
        m.attention_weights(*sides(b))


# ------------------------------------------------------------------ 2. the explanations
@pytest.mark.parametrize("B", [8, 32])
@pytest.mark.parametrize("base", ["tgn", "tgat"])
def test_attention_explanation(dev, base, B):
    from tempme_amd import baselines
    m = model(base, dev)
    b, d = make_batch(B)
    N = d["N"]
    e = baselines.attention_explanation(m, b)
    nodes = records(b, dev, 2)
    assert [tuple(x.shape) for x in e] == [(3 * B, N), (3 * B, N * N)]
    m1, m2 = m.attention_weights(*sides(b), head_mean=True)
    for x, n, raw in zip(e, nodes, (m1, m2.reshape(3 * B, N * N))):
        assert x.dtype == torch.float32 and x.device == dev
        assert bool((x >= 0).all()) and bool((x[n == 0] == 0).all()) and bool((n == 0).any())
        # a live slot may still carry 0: the head-major pairing masks it with another row's record
        assert torch.equal(x[n != 0], raw[n != 0]) and bool((x[n != 0] > 0).any())
    same = baselines.baseline_explanation("attention", args_for(base, N, B), m, b)
    assert all(torch.equal(x, y) for x, y in zip(e, same))


def test_attention_explanation_of_graphmixer_points_to_saliency(dev):
    from tempme_amd import baselines
    m = model("graphmixer", dev)
    b, _ = make_batch(8)
    with pytest.raises(NotImplementedError, match="saliency"):
        baselines.attention_explanation(m, b)
    with pytest.raises(NotImplementedError, match="saliency"):
        baselines.baseline_explanation("attention", args_for("graphmixer"), m, b)


@pytest.mark.parametrize("B", [8, 32])
@pytest.mark.parametrize("base", BASES)
def test_saliency_is_the_gradient_through_contrast(dev, base, B):
    from tempme_amd import baselines
    m = model(base, dev)
    b, d = make_batch(B)
    N = d["N"]
    hops = 1 if base == "graphmixer" else 2
    nodes = records(b, dev, hops)
    assert all(p.grad is None for p in m.parameters()) and not m.training
    e = baselines.saliency_explanation(args_for(base, N, B), m, b)
    assert all(p.grad is None for p in m.parameters()) and not m.training
    # by hand
    w = [torch.ones(n.shape, dtype=torch.float32, device=dev, requires_grad=True) for n in nodes]
    pos, neg = contrast(base, m, b, w)
    (pos.sum() + neg.sum()).backward()
    for p in m.parameters():
        p.grad = None
    assert len(e) == hops
    for x, wi, n in zip(e, w, nodes):
        assert tuple(x.shape) == tuple(n.shape) and x.dtype == torch.float32 and not x.requires_grad
        assert torch.equal(x, wi.grad.abs() * (n != 0))
        assert bool((x >= 0).all()) and bool((x[n == 0] == 0).all()) and float(x.max()) > 0
    # the mode is put back as it was
    m.train()
    try:
        e2 = baselines.saliency_explanation(args_for(base, N, B), m, b)
        assert m.training and all(p.grad is None for p in m.parameters())
    finally:
        m.eval()
    assert all(torch.equal(x, y) for x, y in zip(e, e2))


def test_random_explanation_on_the_device(dev):
    from tempme_amd import baselines
    b, d = make_batch(8)
    m = model("tgn", dev)
    e = baselines.baseline_explanation("random", args_for("tgn"), m, b)
    again = baselines.random_explanation(b, 5, 2, dev)
    nodes = records(b, dev, 2)
    for x, y, n in zip(e, again, nodes):
        assert x.device == dev and torch.equal(x, y) and bool((x[n == 0] == 0).all()) and bool((x >= 0).all())
    assert len(baselines.baseline_explanation("random", args_for("graphmixer"), model("graphmixer", dev), b)) == 1
    with pytest.raises(ValueError, match="lime"):
        baselines.baseline_explanation("lime", args_for("tgn"), m, b)


# ------------------------------------------------------------------ 3. into the fidelity harness
def _methods(base):
    return ("saliency", "random") if base == "graphmixer" else ("attention", "saliency", "random")


@pytest.mark.parametrize("device_metrics", [False, True])
@pytest.mark.parametrize("base", BASES)
def test_threshold_rows_equal_threshold_test_by_hand(dev, base, device_metrics):
    from tempme_amd import baselines, fidelity
    from tempme_amd.train import split_stacked_weights
    m = model(base, dev)
    B = 32
    b, d = make_batch(B)
    args = args_for(base, d["N"], B)
    rows = baselines.threshold_rows(args, m, b, _methods(base), device_metrics=device_metrics)
    assert tuple(rows) == _methods(base)
    with torch.no_grad():
        p, n = contrast(base, m, b)
    y_ori = torch.where(torch.cat([p, n]).sigmoid() > 0.5, 1., 0.).view(-1, 1)
    assert 0 < float(y_ori.sum()) < 2 * B                       # both classes: the ranking figures exist
    for method in _methods(base):
        expl = baselines.baseline_explanation(method, args, m, b)
        if base == "tgat":
            expl = split_stacked_weights(*expl, flat=True)
        want = fidelity.threshold_test(args, expl, m, b.src, b.dst, b.fake, b.ts, b.e_idx, p, n, y_ori, *b.subgraphs,
                                       device_metrics=device_metrics)
        got = rows[method]
        if device_metrics:
            assert torch.is_tensor(got) and got.device == dev and got.dtype == torch.float64
            assert tuple(got.shape) == (5,) and torch.equal(got, want)
        else:
            assert len(got) == 5 and tuple(got) == tuple(want)
        print(base, method, "ratio figures", [float(v) for v in got])
        assert np.isfinite(np.asarray([float(v) for v in got])).all()
    with pytest.raises(ValueError, match="lime"):
        baselines.threshold_rows(args, m, b, ("lime",))


@pytest.mark.parametrize("base", BASES)
def test_kept_and_ranked_edges_take_a_baseline(dev, base):
    from tempme_amd import baselines, fidelity
    from tempme_amd.ranked_edges import ranked_edges
    from tempme_amd.train import split_stacked_weights
    m = model(base, dev)
    B = 8
    b, d = make_batch(B)
    args = args_for(base, d["N"], B)
    roots = (b.src, b.dst, b.fake)
    for method in _methods(base):
        expl = baselines.baseline_explanation(method, args, m, b)
        r = ranked_edges(expl, b.subgraphs, roots, 5, check=True)
        assert tuple(r.eid.shape) == (2, B, 5) and bool((r.count >= 0).all())
        assert bool((r.score[:, :, :-1] >= r.score[:, :, 1:]).all()) and bool((r.score >= 0).all())
        six = split_stacked_weights(*expl, flat=True) if base == "tgat" else expl
        k = fidelity.kept_edges(args, six, *b.subgraphs, roots, 0.2, 5)
        assert tuple(k.eid.shape) == (2, B, 5) and bool((k.count <= r.count).all())
