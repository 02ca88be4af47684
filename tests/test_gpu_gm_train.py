"""Base-GraphMixer training on the HIP path (GraphMixer.train_on_hip: tm_gm_train_fwd / tm_gm_train_bwd,
csrc/graphmixer_train.hip) against the torch formulation with the same dropout masks (tests/gm_train_ref.py),
the reference's own training step (tests/golden/graphmixer_train.npz) and, end to end, learn_base.train_epoch."""
import os

import numpy as np
import pytest
import torch

import gm_train_ref as GR
import tgn_inputs as TI
from gm_shape_inputs import TRAIN
from oracle import graphmixer_ref as O
from tests.test_gpu_graphmixer import ATOL, CASES, RTOL
from tests.test_graphmixer_oracle import SEEDS

pytestmark = pytest.mark.gpu

# N, C, L, p, B: one / two token tiles, channel counts with and without padding to 16, a ragged last hidden chunk
# (HC = 688 = 5 * 128 + 48), R N no multiple of any reduction chunk (B = 7), NULL masks (p = 0)
SHAPES = [(30, 172, 3, 0.5, 20), (12, 172, 2, 0.5, 20), (20, 32, 1, 0.0, 20), (16, 100, 3, 0.5, 7), (20, 1, 3, 0.5, 20)]
# every test below runs SHAPES (T = C, ids as before) and gm_shape_inputs.TRAIN (its own T: the fourth tile slot of
# a wave at C > 192, T < C, 4 layers, N = 2 and 32)
ALL_SHAPES = [(*s, None) for s in SHAPES] + [(N, C, L, p, B, T) for N, C, T, L, p, B in TRAIN]
ALL_IDS = ["-".join(str(x) for x in s) for s in SHAPES] + [f"{N}-{C}-{L}-{p}-{B}-T{T}" for N, C, T, L, p, B in TRAIN]
EMBED = ("projection_layer", "mlp_mixers")
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


def bce_step(model, batch):
    p, n = model.contrast(batch[0], batch[1], batch[2], batch[3], None, *batch[4:], explain_weights=None, edge_attr=None)
    crit = torch.nn.functional.binary_cross_entropy_with_logits
    loss = crit(p, torch.ones_like(p)) + crit(n, torch.zeros_like(n))
    loss.backward()
    return loss.detach(), p.detach(), n.detach()


def grads_of(model):
    return {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in model.named_parameters()
            if v.requires_grad}


def make_case(dev, N, C, L, p, B, T=None):
    """Inputs as test_hip_ew_gradient_vs_oracle builds them (V = 300, E = 2000, padding neighbours at rate 0.25, one
    row with no valid neighbour); one HIP training step, a second identical one, the same call with the flag off,
    and the fp64 / fp32 torch formulation with the same masks on the CPU.  T (default C) is the node-feature and
    time-encoding width.  Computed once per shape."""
    T = C if T is None else T
    key = (N, C, L, p, B, T)
    if key in _cache:
        return _cache[key]
    from tempme_amd.graphmixer import GraphMixer
    rng = np.random.default_rng(N + C + L)
    V, E = 300, 2000
    nf = rng.uniform(0, 1, (V, T)).astype(np.float32)
    ef = rng.uniform(0, 1, (E + 1, C)).astype(np.float32)
    nf[0] = ef[0] = 0
    torch.manual_seed(N + L)
    m = GraphMixer(nf, ef, n_neighbors=N, device=dev, num_tokens=N, num_layers=L, dropout=p).to(dev)
    cut = np.floor(rng.uniform(5e7, 1e8, B))
    sgs = []
    for _ in range(3):
        node = rng.integers(1, V, (B, N))
        node[rng.uniform(size=node.shape) < 0.25] = 0
        node[1] = 0
        eid = np.where(node > 0, rng.integers(1, E + 1, node.shape), 0)
        ts = np.where(node > 0, np.floor(cut[:, None] - rng.uniform(0, 5e7, node.shape)), 0.0)
        sgs.append(([node.astype(np.float64), None], [eid.astype(np.float64), None], [ts, None]))
    src, dst, fake = (rng.integers(1, V, B) for _ in range(3))
    batch = (src, dst, fake, cut, *sgs)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    keep = None
    if p > 0:
        keep = m.draw_keep_masks(3 * B, N, generator=torch.Generator(device=dev).manual_seed(N + C))
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    c = type("Case", (), {})()
    c.model, c.batch, c.sd, c.keep, c.scale, c.L = m, batch, sd, keep, scale, L
    # the flag off first: the torch formulation (its own dropout draws), no marker
    m.train()
    m.gm_keep_masks = keep
    bce_step(m, batch)
    c.off_marker = getattr(m, "_gm_train_key", None)
    c.off_grads = grads_of(m)
    m.zero_grad(set_to_none=True)
    m.train_on_hip()
    c.loss, c.pos, c.neg = bce_step(m, batch)
    c.marker = getattr(m, "_gm_train_key", None)
    c.grads = grads_of(m)
    m.zero_grad(set_to_none=True)
    c.loss2, c.pos2, c.neg2 = bce_step(m, batch)
    c.grads2 = grads_of(m)
    m.zero_grad(set_to_none=True)
    kc = None if keep is None else keep.cpu()
    c.ref64 = GR.loss_and_grads(sd, L, batch, kc, scale, torch.float64)
    c.ref32 = GR.loss_and_grads(sd, L, batch, kc, scale, torch.float32)
    _cache[key] = c
    return c


def check_grads(grads, g64, g32, tag=""):
    """For every parameter tensor ||g_hip - g_64|| <= max(1e-4 ||g_64||, 10 ||g_32 - g_64||): 1e-4 is the bound
    tm_gm_embed_bwd is held to through the same chain, the x10 envelope DESIGN.md section 6i's rule for a
    different summation order.  Returns the worst ratio to that bound per tensor kind."""
    worst = {}
    for k, ref in g64.items():
        assert grads.get(k) is not None, f"{tag}{k}: no gradient"
        got = grads[k].double().cpu()
        err = float(torch.linalg.norm(got - ref))
        bound = max(1e-4 * float(torch.linalg.norm(ref)), 10 * float(torch.linalg.norm(g32[k].double() - ref)))
        kind = ".".join(x for x in k.split(".") if not x.isdigit())
        worst[kind] = max(worst.get(kind, 0.0), err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
        print(f"{tag}{k}: err {err:.3e} bound {bound:.3e} |g64| {float(torch.linalg.norm(ref)):.3e}")
        assert err <= bound, (tag, k, err, bound)
    return worst


@pytest.mark.parametrize("N,C,L,p,B,T", ALL_SHAPES, ids=ALL_IDS)
def test_logits_match_fp64_formulation(dev, N, C, L, p, B, T):
    c = make_case(dev, N, C, L, p, B, T)
    _, p64, n64, _ = c.ref64
    got = torch.cat([c.pos, c.neg]).double().cpu().numpy()
    print("max |logit - fp64|", float(np.abs(got - torch.cat([p64, n64]).numpy()).max()))
    np.testing.assert_allclose(got, torch.cat([p64, n64]).numpy(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("N,C,L,p,B,T", ALL_SHAPES, ids=ALL_IDS)
def test_parameter_gradients_match_fp64_formulation(dev, N, C, L, p, B, T):
    c = make_case(dev, N, C, L, p, B, T)
    worst = check_grads(c.grads, c.ref64[3], c.ref32[3])
    print("worst err / bound per tensor kind:", {k: round(v, 4) for k, v in sorted(worst.items())})


@pytest.mark.parametrize("N,C,L,p,B,T", ALL_SHAPES, ids=ALL_IDS)
def test_every_embedding_parameter_has_a_gradient(dev, N, C, L, p, B, T):
    c = make_case(dev, N, C, L, p, B, T)
    names = [k for k in c.grads if k.startswith(EMBED)]
    assert len(names) == 2 + 12 * L
    for k, g in c.grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        assert g.shape == c.sd[k].shape


@pytest.mark.parametrize("N,C,L,p,B,T", ALL_SHAPES, ids=ALL_IDS)
def test_second_call_is_bitwise_equal(dev, N, C, L, p, B, T):
    c = make_case(dev, N, C, L, p, B, T)
    assert torch.equal(c.pos, c.pos2) and torch.equal(c.neg, c.neg2)
    for k, g in c.grads.items():
        assert torch.equal(g, c.grads2[k]), k


@pytest.mark.parametrize("N,C,L,p,B,T", ALL_SHAPES, ids=ALL_IDS)
def test_path_markers(dev, N, C, L, p, B, T):
    c = make_case(dev, N, C, L, p, B, T)
    assert c.off_marker is None, "train_on_hip is off by default: the torch formulation must run"
    assert all(g is not None for g in c.off_grads.values())
    assert c.marker == (3 * B, N, p > 0), "the HIP training path did not run"
    m = c.model
    # eval, explanation weights and edge_attr keep their paths
    before = m._gm_train_key
    m._gm_train_key = None
    ew = torch.rand(3 * B, N, device=dev)
    m.contrast(c.batch[0], c.batch[1], c.batch[2], c.batch[3], None, *c.batch[4:], explain_weights=[ew])
    m.eval()
    with torch.no_grad():
        m.contrast(c.batch[0], c.batch[1], c.batch[2], c.batch[3], None, *c.batch[4:])
    m.train()
    with torch.no_grad():
        m.contrast(c.batch[0], c.batch[1], c.batch[2], c.batch[3], None, *c.batch[4:])
    assert m._gm_train_key is None
    m._gm_train_key = before


@pytest.mark.parametrize("N,C,L,p,B,T", ALL_SHAPES, ids=ALL_IDS)
def test_eval_after_an_adam_step_follows_the_weights(dev, N, C, L, p, B, T):
    """One Adam step through the HIP path, then model.eval() under no_grad (the packed eval kernels) against the
    fp64 oracle on the updated state_dict: the packs follow the weights."""
    c = make_case(dev, N, C, L, p, B, T)
    m = c.model
    try:
        opt = torch.optim.Adam(m.parameters(), lr=0.01)
        m.train()
        opt.zero_grad()
        bce_step(m, c.batch)
        opt.step()
        moved = max(float((v.detach().cpu() - c.sd[k]).abs().max()) for k, v in m.named_parameters()
                    if k.startswith(EMBED))
        assert moved > 1e-3, "the embedding's parameters did not move"
        m.eval()
        with torch.no_grad():
            pos, neg = m.contrast(c.batch[0], c.batch[1], c.batch[2], c.batch[3], None, *c.batch[4:])
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        p64, n64 = O.contrast(sd, L, c.batch[0], c.batch[1], c.batch[2], c.batch[3], *c.batch[4:], dtype=torch.float64)
        np.testing.assert_allclose(torch.cat([pos, neg]).double().cpu().numpy(), torch.cat([p64, n64]).numpy(),
                                   atol=ATOL, rtol=RTOL)
    finally:
        m.load_state_dict(c.sd)
        m.zero_grad(set_to_none=True)
        m.train()


@pytest.mark.parametrize("case", CASES)
def test_reference_training_step_on_the_device(dev, case):
    """The reference's own step (tests/golden/graphmixer_train.npz: .train(), dropout 0, 3 layers, the golden batch):
    HIP loss and logits within ATOL / RTOL, gradients within max(1e-4 ||g_ref||, 10 ||g_32 - g_64||)."""
    from tempme_amd.graphmixer import GraphMixer
    g = np.load(os.path.join(TI.G, "graphmixer_train.npz"))
    d = TI.load_batch()
    nf, ef = TI.feats(case)
    torch.manual_seed(SEEDS[case])
    m = GraphMixer(nf, ef, n_neighbors=TI.N_DEG, device=dev, num_tokens=TI.N_DEG, num_layers=3, dropout=0.0).to(dev)
    m.train().train_on_hip()
    batch = (d["src"], d["dst"], d["fake"], d["ts_cut"], d["sg_src"], d["sg_tgt"], d["sg_bgd"])
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    loss, pos, neg = bce_step(m, batch)
    assert m._gm_train_key == (3 * d["B"], d["N"], False)
    np.testing.assert_allclose(pos.cpu().numpy(), g[f"{case}_pos"], atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(neg.cpu().numpy(), g[f"{case}_neg"], atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(float(loss), float(g[f"{case}_loss"]), atol=ATOL, rtol=RTOL)
    g64 = GR.loss_and_grads(sd, 3, batch, dtype=torch.float64)[3]
    g32 = GR.loss_and_grads(sd, 3, batch, dtype=torch.float32)[3]
    ref = {str(k): torch.from_numpy(g[f"{case}_grad_{k}"]).double() for k in g[f"{case}_grad_names"]}
    assert set(ref) == set(g64)
    # the reference's stored fp32 gradients stand where g_64 stands above; the envelope stays the fp32
    # formulation's distance to fp64
    shifted = {k: ref[k] + (g32[k].double() - g64[k]) for k in ref}
    got = grads_of(m)
    # a gradient that is identically zero (channel_norm.weight with one channel: the LayerNorm's output is its bias)
    # has no norm to be relative to, and the reference's fp32 step leaves rounding residue there: held to 1e-5 of
    # the norm of the same LayerNorm's bias gradient, as in tests/test_gm_train_cpu.py
    for k in [k for k in ref if k.endswith("norm.weight")]:
        nb = float(torch.linalg.norm(ref[k[:-len("weight")] + "bias"]))
        if float(torch.linalg.norm(g64[k])) <= 1e-12 * nb:
            err = float(torch.linalg.norm(got[k].double().cpu() - ref.pop(k)))
            print(f"{case} {k}: identically zero, err {err:.3e} against 1e-5 * {nb:.3e}")
            assert err <= 1e-5 * nb, (k, err, nb)
    check_grads(got, ref, shifted, tag=f"{case} ")


def test_train_epoch_lowers_the_loss(dev):
    """learn_base.train_epoch on the uslegis fixture (bs = 64, N = 30, p = 0.1, 3 layers, Adam lr 0.01, seeded
    model, order and draws) for 60 steps: the mean loss of the last ten steps is below the mean of the first ten.

    The step count comes from the CPU torch formulation (tests/gm_train_ref.py in fp32 with autograd and
    torch.optim.Adam, on the same batches: the oracle's khop / neg_sample with train_epoch's keys; its own mask
    draws): first ten 1.3995, last ten 1.2226 after 60 steps (a drop of 0.177; after 40 steps 1.3083, a drop of
    0.091), so the condition holds there with a wide margin."""
    import pandas as pd

    from tempme_amd import learn_base
    from tempme_amd.graphmixer import GraphMixer
    G = os.path.join(TI.G, "data")
    g_df = pd.read_csv(os.path.join(G, "ml_uslegis_sampled.csv"))
    ef = np.load(os.path.join(G, "ml_uslegis_sampled.npy"))
    nf = np.load(os.path.join(G, "ml_uslegis_sampled_node.npy"))
    sp = learn_base.split_data(g_df, device=dev)
    N, bs, steps = 30, 64, 60
    torch.manual_seed(3)
    m = GraphMixer(nf, ef, n_neighbors=N, device=dev, num_tokens=N, num_layers=3, dropout=0.1).to(dev)
    m.train_on_hip()
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    idx = np.random.default_rng(0).permutation(len(sp.train_src_l))
    out = learn_base.train_epoch(m, opt, sp.train_ngh_finder, sp.train_rand_sampler, sp.train_src_l, sp.train_dst_l,
                                 sp.train_ts_l, sp.train_e_idx_l, bs, idx_list=idx, max_steps=steps, metrics=False)
    loss = out["loss"]
    assert len(loss) == steps and np.isfinite(loss).all()
    assert m._gm_train_key == (3 * bs, N, True)
    first, last = float(np.mean(loss[:10])), float(np.mean(loss[-10:]))
    print("first ten", first, "last ten", last)
    assert last < first, (first, last)
