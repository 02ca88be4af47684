"""Training the motif-enhanced predictor on the GPU: tm_encoder_pool_train_fwd / tm_encoder_pool_bwd /
tm_encoder_pool_wgrad through TempME.enhance_train_groups and enhance_predict_*, against the fp64 restatement with
the same keep-masks (tests/enhance_train_ref.py) and the reference's own gradients (tests/golden/enhance_uslegis.npz).

Tolerances: 10x the restatement's own fp32-vs-fp64 distance for that quantity at that shape, computed here and
printed (the convention of tests/test_gpu_enhance.py); the golden cases take the golden file's envelopes."""
import numpy as np
import pytest
import torch

import enhance_inputs as XI
import enhance_train_ref as TR
from enhance_inputs import Base, agg_with_grads, check_agg_against_golden, make_explainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = {"2x3x7": (2, 3, 7), "1x1x12": (1, 1, 12)}      # 42 walks: a 16-walk tile straddles the groups, the last is partial


def build(seed=3, shape=(2, 3, 7), de=32, zero_nodes=False, hid_dim=64, **kw):
    import tempme_amd as tm
    d = TR.seeded_inputs(seed, *shape, de=de, zero_nodes=zero_nodes)
    torch.manual_seed(7)
    ex = tm.TempME(Base(d["n_feat"], d["e_feat"]), "tgn", "uslegis_sampled", 40, hid_dim, device=DEV,
                   null_model={k: 1.0 / 12 for k in range(1, 13)}, **kw).to(DEV).train()
    ex.set_node_degree(d["deg"])
    d["sd"] = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    G = d["G"]
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)  # noqa: E731
    cut = to(d["cut"], torch.float64).reshape(1, -1).expand(G, -1).contiguous()
    d["args"] = (to(d["node"], torch.int32), to(d["eid"], torch.int32), to(d["ts"], torch.float32),
                 to(d["cat"], torch.int32), cut, to(d["cnt"], torch.float32), G, d["B"], d["W"])
    return ex, d


def masks(ex, d, seed=11, p=0.5):
    rng = np.random.default_rng(seed)
    n = d["G"] * d["B"] * d["W"]
    return torch.from_numpy((rng.uniform(0, 1, (n, ex.dropout_cols())) >= p).astype(np.uint8)), 1.0 / (1.0 - p)


def run(ex, d, drop=None, scale=1.0, d_emb=None):
    """enhance_train_groups with injected masks -> (emb, {parameter name: gradient or None})."""
    ex.zero_grad()
    emb = ex.enhance_train_groups(*d["args"], drop=None if drop is None else drop.to(DEV), drop_scale=scale,
                                  use_module_dropout=False)
    if d_emb is None:
        return emb.detach(), None
    (emb * d_emb.to(DEV)).sum().backward()
    return emb.detach(), {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in ex.named_parameters()}


def d_emb_for(ex, d, seed=5):
    """A random upstream gradient; its histogram columns are non-zero and must have no effect."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.normal(0, 1, (d["G"], d["B"], ex.mlp_dim)).astype(np.float32))


# ------------------------------------------------------------------ 1. forward without masks = the eval pooled path
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_without_masks_is_the_eval_pooled_path(shape):
    ex, d = build(shape=SHAPES[shape])
    sd, tg, ic = d["sd"], ex.use_temporal_guidance, ex.if_cat
    r32 = TR.groups(sd, d, tg, ic)
    r64 = TR.groups({k: v.double() for k, v in sd.items()}, d, tg, ic)
    tol = 10 * float((r32.double() - r64).abs().max())
    got, _ = run(ex, d)
    assert tuple(got.shape) == (d["G"], d["B"], ex.mlp_dim)
    dist = float((got.cpu().double() - r64).abs().max())
    with torch.no_grad():
        ev = ex.eval().enhance_groups(*d["args"])
    de = float((got - ev).abs().max())
    print(shape, "train fwd vs fp64", dist, "tolerance", tol, "| vs enhance_groups", de, "tolerance", 2 * tol)
    assert dist <= tol
    assert float((ev.cpu().double() - r64).abs().max()) <= tol
    assert de <= 2 * tol
    assert torch.equal(got[:, :, ex.hid_dim:], ev[:, :, ex.hid_dim:])          # the histogram: exact counts


# ------------------------------------------------------------------ 2. backward vs fp64 autograd, same masks
VARIANTS = {
    "default": dict(),
    "default_1x1x12": dict(shape=SHAPES["1x1x12"]),
    "zero_nodes": dict(zero_nodes=True),
    "nocat": dict(if_cat_feature=False),
    "plain_attention": dict(use_temporal_guidance=False),            # no dropout: the masks are not passed on
    "hid32": dict(hid_dim=32),
    "hid128": dict(hid_dim=128),
    "hid48_padded": dict(hid_dim=48),
    "de1": dict(de=1),                                               # the LDS-tiled event_gcn kernels
    "de4": dict(de=4),                                               # register-resident event_gcn, Q = 12
    "de36": dict(de=36),                                             # register-resident event_gcn, Q = 14
    "de36_zero_nodes": dict(de=36, zero_nodes=True),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_backward_matches_fp64_autograd(variant):
    ex, d = build(**VARIANTS[variant])
    tg, ic = ex.use_temporal_guidance, ex.if_cat
    drop, scale = masks(ex, d) if tg else (None, 1.0)
    d_emb = d_emb_for(ex, d)
    assert not ic or bool((d_emb[:, :, ex.hid_dim:] != 0).all())
    e32, g32 = TR.forward_and_grads(d["sd"], d, d_emb, tg, ic, drop, scale, torch.float32)
    e64, g64 = TR.forward_and_grads(d["sd"], d, d_emb, tg, ic, drop, scale, torch.float64)
    emb, grads = run(ex, d, drop, scale, d_emb)
    tol = 10 * float((e32.double() - e64).abs().max())
    dist = float((emb.cpu().double() - e64).abs().max())
    print(variant, "emb", dist, "tolerance", tol)
    missed = [("emb", dist, tol)] if not dist <= tol else []
    names = TR.pool_params(tg)
    assert len(names) == 16
    for k in names:
        assert grads[k] is not None, k
        assert tuple(grads[k].shape) == tuple(d["sd"][k].shape), k
        gt = 10 * float((g32[k].double() - g64[k]).abs().max())
        dg = float((grads[k].double() - g64[k]).abs().max())
        print(variant, "grad", k, dg, "tolerance", gt)
        if not dg <= gt:
            missed.append((k, dg, gt))
    for k in TR.SCORING_PARAMS:
        assert grads[k] is None and g64[k] is None, k                 # the reference's autograd leaves them unused too
    assert not missed, missed                                         # every gradient is measured before the first miss


# ------------------------------------------------------------------ 3. the masks act, and only the documented columns
def test_masks_are_applied_and_only_documented_columns_matter():
    ex, d = build()
    drop, scale = masks(ex, d)
    d_emb = d_emb_for(ex, d)
    plain, _ = run(ex, d)
    emb, grads = run(ex, d, drop, scale, d_emb)
    assert not torch.equal(emb, plain)
    sd64 = {k: v.double() for k, v in d["sd"].items()}
    r64 = TR.groups(sd64, d, True, True, drop, scale)
    tol = 10 * float((TR.groups(d["sd"], d, True, True, drop, scale).double() - r64).abs().max())
    dist = float((emb.cpu().double() - r64).abs().max())
    print("masked emb", dist, "tolerance", tol)
    assert dist <= tol
    flipped = drop.clone()
    flipped[:, 2 + ex.hid_dim:] ^= 1                                  # the scoring MLP's hidden columns and the padding
    emb2, grads2 = run(ex, d, flipped, scale, d_emb)
    assert torch.equal(emb, emb2)
    for k in TR.POOL_PARAMS:
        assert torch.equal(grads[k], grads2[k]), k
    d_emb2 = d_emb.clone()
    d_emb2[:, :, ex.hid_dim:] = 0                                     # the histogram's upstream gradient: no effect
    _, grads3 = run(ex, d, drop, scale, d_emb2)
    for k in TR.POOL_PARAMS:
        assert torch.equal(grads[k], grads3[k]), k


# ------------------------------------------------------------------ 4. reproducible
def test_forward_and_backward_are_bitwise_reproducible():
    ex, d = build()
    drop, scale = masks(ex, d)
    d_emb = d_emb_for(ex, d)
    emb, grads = run(ex, d, drop, scale, d_emb)
    emb2, grads2 = run(ex, d, drop, scale, d_emb)
    assert torch.equal(emb, emb2)
    for k in TR.POOL_PARAMS:
        assert torch.equal(grads[k], grads2[k]), k


# ------------------------------------------------------------------ 5. enhance_predict_agg end to end
@pytest.fixture(scope="module")
def gold():
    return XI.golden()


@pytest.fixture(scope="module", params=XI.CASES)
def case(request):
    d = XI.load(request.param)
    d["case"] = request.param
    d["sd_all"] = dict(d["sd"], **d["aff"])
    return d


def agg(ex, case, gats):
    B = case["B"]
    sides = [XI.side_walks(case, s, B) for s in XI.SIDES]
    return ex.enhance_predict_agg(case["ts_cut"][:B], sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides], *gats)


def profiled(fn):
    from tempme_amd import _lib as L
    L.profile_enable(True)
    try:
        out = fn()
        prof = L.profile_read()
    finally:
        L.profile_enable(False)
    return out, (lambda k: prof.get(k, (0.0, 0))[1])


def test_agg_eval_mode_with_gradients_matches_golden(case, gold):
    """Eval mode, parameters requiring gradients: no dropout, three groups, the golden's dropout-free function."""
    ex = make_explainer(case, DEV).eval()
    ex.set_node_degree(case["deg"])
    (pos, neg, grads), count = profiled(lambda: agg_with_grads(ex, case))
    assert count("head_pool_train_kernel") == 1 and count("head_pool_bwd_kernel") == 1
    check_agg_against_golden(pos, neg, grads, gold, case["case"])


def test_agg_train_mode_is_seeded_by_torch_rng(case):
    ex = make_explainer(case, DEV, dropout_p=0.1).train()
    ex.set_node_degree(case["deg"])
    assert ex.attention.dropout.p == 0.1 and ex.attention.MLP[2].p == 0.1
    gats = [g.clone().to(DEV).requires_grad_(True) for g in case["gats"]]
    torch.manual_seed(123)
    p1, n1 = agg(ex, case, gats)
    torch.manual_seed(123)
    p2, n2 = agg(ex, case, gats)
    torch.manual_seed(124)
    p3, n3 = agg(ex, case, gats)
    assert torch.equal(p1, p2) and torch.equal(n1, n2)
    assert not torch.equal(p1, p3) and not torch.equal(n1, n3)
    assert bool(torch.isfinite(p1).all()) and tuple(p1.shape) == (case["B"], 1) and tuple(n1.shape) == (case["B"], 1)
    ex.zero_grad()
    (p1.sum() + n1.sum()).backward()
    for g in gats:
        assert g.grad is not None and bool(torch.isfinite(g.grad).all()) and float(g.grad.abs().max()) > 0
    params = dict(ex.named_parameters())
    for k in TR.POOL_PARAMS:
        assert params[k].grad is not None and bool(torch.isfinite(params[k].grad).all()), k


# ------------------------------------------------------------------ 6. routing
def test_new_entry_points_are_exported():
    import tempme_amd
    from tempme_amd import _lib
    lib = tempme_amd.lib()
    for name in ("tm_encoder_pool_train_workspace_bytes", "tm_encoder_pool_train_fwd", "tm_encoder_pool_bwd",
                 "tm_encoder_pool_wgrad"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_train_mode_agg_runs_the_pooled_training_kernels(case):
    ex = make_explainer(case, DEV, dropout_p=0.1).train()
    ex.set_node_degree(case["deg"])
    gats = [g.clone().to(DEV).requires_grad_(True) for g in case["gats"]]

    def step():
        pos, neg = agg(ex, case, gats)
        (pos.sum() + neg.sum()).backward()
    step()                                                            # weight packs, tables
    _, count = profiled(step)
    for k in ("head_pool_train_kernel", "pool_tail_kernel", "head_pool_bwd_kernel", "gcn_bwd_kernel",
              "walk_importance_kernel", "gcn_kernel"):
        assert count(k) == 1, (k, count(k))
    assert count("head_kernel") == 0 and count("head_bwd_kernel") == 0 and count("walk_pool_kernel") == 0


def test_frozen_explainer_under_no_grad_keeps_the_eval_path(case):
    ex = make_explainer(case, DEV).eval().requires_grad_(False)
    ex.set_node_degree(case["deg"])
    gats = [g.to(DEV) for g in case["gats"]]
    with torch.no_grad():
        agg(ex, case, gats)
        _, count = profiled(lambda: agg(ex, case, gats))
    assert count("walk_pool_kernel") == 1 and count("pool_tail_kernel") == 1
    assert count("head_pool_train_kernel") == 0 and count("head_pool_bwd_kernel") == 0


def test_pairs_and_walks_take_the_training_path(case):
    """Eval mode with trainable parameters (no dropout draws): enhance_predict_pairs stacks its sides as two groups,
    each equal bit for bit to its own enhance_predict_walks call; sides of different shapes run one call per side."""
    ex = make_explainer(case, DEV).eval()
    ex.set_node_degree(case["deg"])
    B = 5
    (ws, cs), (wt, ct) = XI.side_walks(case, "src", B), XI.side_walks(case, "tgt", B)
    cut = case["ts_cut"][:B]
    (s, t), count = profiled(lambda: ex.enhance_predict_pairs(ws, wt, cut, cs, ct))
    assert count("head_pool_train_kernel") == 1 and count("walk_pool_kernel") == 0
    assert s.requires_grad and tuple(s.shape) == (B, 76)
    assert torch.equal(s, ex.enhance_predict_walks(ws, cut, cs)) and torch.equal(t, ex.enhance_predict_walks(wt, cut, ct))
    half = tuple(a[:, :30] for a in wt[:4]) + (None,)                  # 30 walks per event on the tgt side
    (s2, t2), count = profiled(lambda: ex.enhance_predict_pairs(ws, half, cut, cs, ct[:, :30]))
    assert count("head_pool_train_kernel") == 2
    assert torch.equal(s2, s) and tuple(t2.shape) == (B, 76)


# ------------------------------------------------------------------ 7. error paths (host arrays: checked before any launch)
def test_out_of_range_ids_raise_index_error(case):
    ex = make_explainer(case, DEV).train()
    ex.set_node_degree(case["deg"])
    B = 5
    walks, cnt = XI.side_walks(case, "src", B)
    cut = case["ts_cut"][:B]
    assert tuple(ex.enhance_predict_walks(walks, cut, cnt).shape) == (B, 76)
    node = walks[0].copy()
    node[2, 5, 1] = case["n_feat"].shape[0]                           # outside the node table and node_degree
    with pytest.raises(IndexError):
        ex.enhance_predict_walks((node,) + tuple(walks[1:]), cut, cnt)
    eid = walks[1].copy()
    eid[1, 3, 0] = case["e_feat"].shape[0]
    with pytest.raises(IndexError):
        ex.enhance_predict_walks((walks[0], eid) + tuple(walks[2:]), cut, cnt)
    assert tuple(ex.enhance_predict_walks(walks, cut, cnt).shape) == (B, 76)
