"""Motif-enhanced link prediction on the GPU: tm_walk_importance and tm_encoder_pool_fwd (through
TempME.walk_importance_groups / enhance_groups) and TempME.enhance_predict_* against the reference's own outputs
(tests/golden/enhance_uslegis.npz) and the fp64 restatement (tests/enhance_ref.py).

Tolerances: 10x the fp32 envelope max |reference fp32 - restatement fp64| the golden generator stored for each
quantity (read from the file), or, for the seeded cases without a golden, 10x the restatement's own
fp32-vs-fp64 distance at that shape, computed in the test."""
import numpy as np
import pytest
import torch

import enhance_inputs as XI
import enhance_ref as XR
from enhance_inputs import Base, agg_with_grads, check_agg_against_golden, make_explainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
W = 60


@pytest.fixture(scope="module")
def gold():
    return XI.golden()


@pytest.fixture(scope="module", params=XI.CASES)
def case(request):
    d = XI.load(request.param)
    d["case"] = request.param
    d["sd_all"] = dict(d["sd"], **d["aff"])
    ex = make_explainer(d, DEV).eval()
    ex.set_node_degree(d["deg"])
    d["ex"] = ex
    return d


def dev_sides(d, bsz, sides=XI.SIDES):
    """The first bsz events of the given sides as enhance_groups' device tensors [G, bsz, W, ...]."""
    t = lambda k, dt: torch.from_numpy(np.stack([np.asarray(d[s][k][:bsz]) for s in sides])).to(DEV, dt).contiguous()  # noqa: E731
    cut = torch.from_numpy(np.asarray(d["ts_cut"][:bsz], dtype=np.float64)).to(DEV)
    return dict(node6=t("node", torch.int32), eid3=t("eid", torch.int32), ts3=t("ts", torch.float32),
                cat=t("cat", torch.int32).reshape(len(sides), bsz, W), cnt=t("cnt", torch.float32),
                cut=cut.reshape(1, bsz).expand(len(sides), bsz).contiguous())


# ------------------------------------------------------------------ 1. tm_walk_importance
@pytest.mark.parametrize("bsz", [32, 5, 1])
def test_walk_importance_matches_reference(case, gold, bsz):
    ex, c = case["ex"], case["case"]
    a = dev_sides(case, bsz)
    got = ex.walk_importance_groups(a["node6"], a["ts3"], a["cut"], 3, bsz, W).cpu().numpy()
    tol = 10 * float(gold[f"{c}_env_wgt"])
    for g, side in enumerate(XI.SIDES):
        d = float(np.abs(got[g] - gold[f"{c}_wgt_{side}_{bsz}"]).max())
        print(c, bsz, side, "wgt", d, "tolerance", tol)
        assert d <= tol
    one = ex.walk_importance_groups(a["node6"][1:2].contiguous(), a["ts3"][1:2].contiguous(), a["cut"][1:2].contiguous(),
                                    1, bsz, W)
    assert np.array_equal(one.cpu().numpy()[0], got[1])             # a group's weights do not depend on its neighbours
    w = ex.compute_walk_importance(case["tgt"]["ts"][:bsz], case["tgt"]["node"][:bsz], case["ts_cut"][:bsz])
    assert tuple(w.shape) == (bsz, W) and np.array_equal(w.cpu().numpy(), got[1])


def test_walk_importance_padding_walk_and_zero_recency(case, gold):
    """A walk whose six node ids are 0 (count 0, mean degree 0) and a walk whose timestamps all equal the cut
    (time difference 0), against the restatement in fp64."""
    ex, c = case["ex"], case["case"]
    bsz = 5
    node = case["src"]["node"][:bsz].copy()
    ts = case["src"]["ts"][:bsz].copy()
    cut = np.asarray(case["ts_cut"][:bsz], dtype=np.float64)
    node[0, 0, :] = 0
    ts[1, 3, :] = cut[1]
    want = XR.walk_importance(case["deg"], ts, node, cut, dtype=torch.float64).numpy()
    to = lambda a, dt: torch.from_numpy(a).to(DEV, dt).reshape(1, *a.shape).contiguous()  # noqa: E731
    got = ex.walk_importance_groups(to(node, torch.int32), to(ts, torch.float32), to(cut, torch.float64), 1, bsz, W)
    d = float(np.abs(got.cpu().numpy()[0] - want).max())
    tol = 10 * float(gold[f"{c}_env_wgt"])
    print(c, "edited walks", d, "tolerance", tol)
    assert d <= tol
    bad = node.copy()
    bad[2, 5, 1] = case["deg"].shape[0]                         # one id past the degree table
    with pytest.raises(IndexError):
        ex.walk_importance_groups(to(bad, torch.int32), to(ts, torch.float32), to(cut, torch.float64), 1, bsz, W)
    ex.walk_importance_groups(to(node, torch.int32), to(ts, torch.float32), to(cut, torch.float64), 1, bsz, W)  # flag reset


def test_walk_importance_all_ones_default(case):
    """node_degree = ones (the constructor's default): the group std of count / (count + 1e-6) is ~2e-7, far below
    the 1e-6 added to it, so the degree weights are a function of fp32 rounding and no parity with the reference is
    claimed.  Checked: finite, every event's weights sum to W within 1e-4 W, and equal to the formula
    with fp64 reductions.  The last bound: given the same fp32 elements and the fp64 statistics rounded to fp32,
    the weights differ only by the device's exp (<= 2 ulp) in rec and in the sigmoid and by the final divisions,
    < 10 ulp = 1.2e-6 relative of weights below 4; 1e-5 absolute."""
    ex = make_explainer(case, DEV).eval()
    assert bool((ex.node_degree == 1).all())
    a = dev_sides(case, 32)
    got = ex.walk_importance_groups(a["node6"], a["ts3"], a["cut"], 3, 32, W).cpu().numpy()
    assert np.isfinite(got).all()
    assert float(np.abs(got.sum(-1) - W).max()) <= 1e-4 * W
    ones = np.ones(case["deg"].shape[0], dtype=np.float32)
    for g, side in enumerate(XI.SIDES):
        want = XR.walk_importance(ones, case[side]["ts"], case[side]["node"], case["ts_cut"], reduce64=True).numpy()
        d = float(np.abs(got[g] - want).max())
        print(case["case"], side, "all-ones vs fp64-reduction formula", d)
        assert d <= 1e-5


# ------------------------------------------------------------------ 2. pooled encoder vs the golden embeddings
def pooled(ex, a, G, bsz, M, etab):
    return ex.enhance_groups(a["node6"], a["eid3"], a["ts3"], a["cat"], a["cut"], a["cnt"], G, bsz, W, M=M, etab=etab)


@pytest.mark.parametrize("bsz", [32, 1, 2])
def test_pooled_encoder_matches_reference(case, gold, bsz):
    """B = 32 as three groups; B = 1: 20 slots at M = 3 (one full 16-slot unit and a partial one); B = 2: a unit
    straddles the two events.  With the per-edge-id table where the dims have one (synth: de = 32) at M = 3, and
    without it at M = 1; every launch twice, compared bitwise."""
    ex, c = case["ex"], case["case"]
    sides = XI.SIDES if bsz == 32 else ("src",)
    a = dev_sides(case, bsz, sides)
    etab = ex.dropin_edge_table()
    assert (etab is not None) == (c == "synth")
    tol = 10 * float(gold[f"{c}_env_emb"])
    for M, tab in ((XI.M_SLOT, etab), (1, None), (XI.M_SLOT, None)):
        out = pooled(ex, a, len(sides), bsz, M, tab)
        again = pooled(ex, a, len(sides), bsz, M, tab)
        assert tuple(out.shape) == (len(sides), bsz, 76)
        assert torch.equal(out, again), "the pooled encoder is not bitwise reproducible"
        for g, side in enumerate(sides):
            d = float(np.abs(out[g].cpu().numpy() - gold[f"{c}_emb_{side}_{bsz}"]).max())
            print(c, bsz, side, "M", M, "table" if tab is not None else "no table", "emb", d, "tolerance", tol)
            assert d <= tol
    # into the leading columns of a wider row (ld_out), the rest untouched
    wide = torch.full((len(sides), bsz, 76 + 172), 7.0, device=DEV)
    ex.enhance_groups(a["node6"], a["eid3"], a["ts3"], a["cat"], a["cut"], a["cnt"], len(sides), bsz, W, M=1, out=wide)
    assert torch.equal(wide[:, :, :76], pooled(ex, a, len(sides), bsz, 1, None)) and bool((wide[:, :, 76:] == 7.0).all())


def test_pooled_encoder_persistent_grid(case, gold):
    """Grids of 512 units or more run the fused kernel's persistent form (one partial per slot, summed over its M
    walks in registers) instead of the split form the small cases above take: the three sides five times over as
    15 groups (600 units at M = 3, 1800 at M = 1), each group against its side's golden."""
    ex, c = case["ex"], case["case"]
    a = {k: v.repeat(5, *([1] * (v.dim() - 1))).contiguous() for k, v in dev_sides(case, 32).items()}
    tol = 10 * float(gold[f"{c}_env_emb"])
    for M, tab in ((XI.M_SLOT, ex.dropin_edge_table()), (1, None)):
        out = pooled(ex, a, 15, 32, M, tab)
        assert torch.equal(out, pooled(ex, a, 15, 32, M, tab)), "the pooled encoder is not bitwise reproducible"
        assert torch.equal(out[:3], out[12:])
        for g, side in enumerate(XI.SIDES):
            d = float(np.abs(out[g].cpu().numpy() - gold[f"{c}_emb_{side}_32"]).max())
            print(c, side, "M", M, "persistent grid emb", d, "tolerance", tol)
            assert d <= tol


# ------------------------------------------------------------------ 3. the other kernel families, seeded weights
FAMILIES = {
    "hid32_nocat": dict(hid_dim=32, if_cat_feature=False),          # LDS-tiled kernels, no histogram
    "hid48_padded": dict(hid_dim=48),                                # weights zero-padded to 64: the fused kernel
    "hid40_padded_nocat": dict(hid_dim=40, if_cat_feature=False),    # zero-padded to 48: the LDS-tiled kernels
    "plain_attention": dict(use_temporal_guidance=False),            # fused kernel, scores not time-weighted
    "hid128": dict(hid_dim=128),
    "zero_node_table": dict(zero_nodes=True),                        # fused kernel, one event_gcn branch, edge table
}


def seeded_walks(rng, B, Wk, M, n_nodes, n_edges):
    """Random walks [B, Wk, ...] in find_k_walks' layout: the M walks of a hop-1 slot share position 2."""
    slot = lambda a: np.repeat(a, M, axis=1)  # noqa: E731
    S = Wk // M
    node = rng.integers(0, n_nodes, (B, Wk, 6))
    node[:, :, 4:6] = slot(rng.integers(1, n_nodes, (B, S, 2)))
    node[0, 1, 0:2] = 0                                              # padding entries
    eid = rng.integers(1, n_edges, (B, Wk, 3))
    eid[:, :, 2] = slot(rng.integers(1, n_edges, (B, S)))
    cut = np.floor(rng.uniform(50, 60, B))
    ts = np.sort(np.floor(rng.uniform(0, 50, (B, Wk, 3))), axis=-1)
    ts[:, :, 2] = slot(np.floor(rng.uniform(40, 50, (B, S))))
    cnt = rng.integers(0, 4, (B, Wk, 3, 3)).astype(np.float64)
    cnt[:, :, 2, :] = slot(rng.integers(0, 4, (B, S, 3)).astype(np.float64))
    cat = rng.integers(0, 12, (B, Wk, 1))
    return node, eid, ts, cat, cnt, cut


@pytest.mark.parametrize("family", list(FAMILIES))
def test_pooled_encoder_other_kernel_families(family):
    import tempme_amd as tm
    kw = dict(FAMILIES[family])
    zero_nodes = kw.pop("zero_nodes", False)
    rng = np.random.default_rng(sorted(FAMILIES).index(family))
    n_nodes, n_edges, B, Wk, M = 40, 90, 4, 12, 3
    n_feat = torch.zeros(n_nodes, 172) if zero_nodes else torch.from_numpy(rng.uniform(0, 1, (n_nodes, 172)).astype(np.float32))
    e_feat = torch.from_numpy(rng.uniform(0, 1, (n_edges, 32)).astype(np.float32))
    torch.manual_seed(7)
    ex = tm.TempME(Base(n_feat, e_feat), "tgn", "uslegis_sampled", 40, kw.pop("hid_dim", 64), device=DEV,
                   null_model={k: 1.0 / 12 for k in range(1, 13)}, **kw).to(DEV).eval()
    deg = rng.integers(1, 30, n_nodes).astype(np.float32)
    ex.set_node_degree(deg)
    node, eid, ts, cat, cnt, cut = seeded_walks(rng, B, Wk, M, n_nodes, n_edges)
    sd = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    temporal, if_cat = ex.use_temporal_guidance, ex.if_cat
    walks = (node, eid, ts, cat)
    r32 = XR.predict_walks(sd, n_feat, e_feat, deg, walks, cut, cnt, temporal, if_cat)
    r64 = XR.predict_walks({k: v.double() for k, v in sd.items()}, n_feat, e_feat, deg, walks, cut, cnt, temporal, if_cat)
    tol = 10 * float((r32.double() - r64).abs().max())
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt).reshape(1, *a.shape).contiguous()  # noqa: E731
    args = (to(node, torch.int32), to(eid, torch.int32), to(ts, torch.float32), to(cat[..., 0], torch.int32),
            to(cut, torch.float64), to(cnt, torch.float32), 1, B, Wk)
    etab = ex.dropin_edge_table()
    assert (etab is not None) == (ex._hid_packed() == 64 and if_cat)
    for Mk, tab in ((M, etab), (1, None)):
        out = ex.enhance_groups(*args, M=Mk, etab=tab)
        assert tuple(out.shape) == (1, B, ex.mlp_dim)
        assert torch.equal(out, ex.enhance_groups(*args, M=Mk, etab=tab))
        d = float((out[0].cpu().double() - r64).abs().max())
        print(family, "M", Mk, "emb", d, "tolerance", tol)
        assert d <= tol


# ------------------------------------------------------------------ 4.-6. enhance_predict_agg
def test_enhance_predict_agg_eval_matches_reference(case, gold):
    ex, c = case["ex"], case["case"]
    B = case["B"]
    sides = [XI.side_walks(case, s, B) for s in XI.SIDES]
    with torch.no_grad():
        pos, neg = ex.enhance_predict_agg(case["ts_cut"][:B], sides[0][0], sides[1][0], sides[2][0],
                                          [s[1] for s in sides], *[g.to(DEV) for g in case["gats"]])
        emb = ex.enhance_predict_walks(sides[1][0], case["ts_cut"][:B], sides[1][1])
    assert tuple(pos.shape) == (B, 1) and tuple(neg.shape) == (B, 1) and pos.device.type == "cuda"
    tol = 10 * float(gold[f"{c}_env_logit"])
    dl = max(float(np.abs(pos.cpu().numpy() - gold[f"{c}_pos"]).max()), float(np.abs(neg.cpu().numpy() - gold[f"{c}_neg"]).max()))
    print(c, "logits", dl, "tolerance", tol)
    assert dl <= tol
    assert float(np.abs(emb.cpu().numpy() - gold[f"{c}_emb_tgt_{B}"]).max()) <= 10 * float(gold[f"{c}_env_emb"])


def test_enhance_predict_agg_train_mode_gradients(case, gold):
    """Train mode with dropout_p = 0: the torch-op formulation on the device, logits and gradients of the golden.
    TemporalAwareAttention builds its two Dropouts with its own default p = 0.1 whatever TempME's dropout_p is
    (explainer_new.py:121, :769-780), so they are set to 0 here as well: the golden is the dropout-free function."""
    ex = make_explainer(case, DEV, dropout_p=0.0).train()
    for m in ex.attention.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    ex.set_node_degree(case["deg"])
    pos, neg, grads = agg_with_grads(ex, case)
    check_agg_against_golden(pos, neg, grads, gold, case["case"])


def test_eval_without_gradients_runs_the_hip_path(case):
    from tempme_amd import _lib as L
    ex = make_explainer(case, DEV).eval().requires_grad_(False)
    ex.set_node_degree(case["deg"])
    B = case["B"]
    sides = [XI.side_walks(case, s, B) for s in XI.SIDES]
    gats = [g.to(DEV) for g in case["gats"]]
    with torch.no_grad():
        ex.enhance_predict_agg(case["ts_cut"][:B], sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides], *gats)
        L.profile_enable(True)
        try:
            ex.enhance_predict_agg(case["ts_cut"][:B], sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides], *gats)
            prof = L.profile_read()
        finally:
            L.profile_enable(False)
    count = lambda k: prof.get(k, (0.0, 0))[1]  # noqa: E731
    assert count("walk_pool_kernel") == 1 and count("pool_tail_kernel") == 1 and count("walk_importance_kernel") == 1
    assert count("head_kernel") == 0 and count("walk_kernel") == 0 and count("gcn_kernel") == 0
