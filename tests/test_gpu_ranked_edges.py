"""Ranked explanation edges on the device: tm_ranked_edges (csrc/ranked_edges.hip) through the C ABI,
ranked_edges.ranked_edges, fidelity.kept_edges and ExplainPipeline.ranked_edges against the numpy restatement
(tests/ranked_edges_ref.py).

The kernel only compares, so every output is checked with np.array_equal, scores as uint32 bit patterns: there is no
tolerance.  Shapes are the smallest at which each mechanism can fail: one entry, a handful, a count that is no power
of two, fewer edges than k, the workload's N = 20, entry counts just over a padded-size boundary (1,122; 4,160) and
the LDS bound (8,064 entries), dead and missing rows, NaN and signed zeros.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import ranked_edges_ref as ER

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 3
SENT = -77


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ the kernel through the C ABI
def launch(dev, imp, node, eid, n, hops, group_rows, k, err=None):
    """tm_ranked_edges on [rows, ne] host records -> (rc, eid, score bits, slot, mult, count, err flag), numpy; the
    outputs sit in windows of guarded buffers."""
    from tempme_amd import _lib as L
    rows, (n_groups, R) = imp.shape[0], group_rows.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    parts = [[d(x[:, :n]), d(x[:, n:]) if hops == 2 else None] for x in (imp, node, eid)]
    grp = d(group_rows)
    kk = max(k, 0)
    bufs = [torch.full((n_groups * kk + 2 * GUARD,), SENT, dtype=dt, device=dev)
            for dt in (torch.int32, torch.float32, torch.int32, torch.int32)]
    cnt = torch.full((n_groups + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    win = lambda b: C.c_void_p(b.data_ptr() + 4 * GUARD)                # noqa: E731
    rc = L.lib().tm_ranked_edges(L.ptr(parts[0][0]), L.ptr(parts[0][1]), L.ptr(parts[1][0]), L.ptr(parts[1][1]),
                                 L.ptr(parts[2][0]), L.ptr(parts[2][1]), rows, n, hops, L.ptr(grp), n_groups, R, k,
                                 win(bufs[0]), win(bufs[1]), win(bufs[2]), win(bufs[3]), win(cnt), L.ptr(flag),
                                 L.stream_ptr(dev))
    outs = []
    for b, m in zip(bufs + [cnt], [n_groups * kk] * 4 + [n_groups]):
        h = b.cpu().numpy()
        assert (h[:GUARD] == SENT).all() and (h[GUARD + m:] == SENT).all(), "a guard word around an output was written"
        outs.append(h[GUARD:GUARD + m])
    o_eid, o_score, o_slot, o_mult, o_cnt = outs
    sh = (n_groups, kk)
    return (rc, o_eid.reshape(sh), o_score.view(np.uint32).reshape(sh), o_slot.reshape(sh), o_mult.reshape(sh), o_cnt,
            int(flag.item()))


def check_case(dev, imp, node, eid, n, hops, group_rows, k, err=0):
    want = ER.ranked_edges_ref(imp, node, eid, group_rows, k)
    rc, *got = launch(dev, imp, node, eid, n, hops, group_rows, k)
    assert rc == 0
    for name, g, w in zip(("eid", "score bits", "slot", "mult", "count"), got, want):
        assert np.array_equal(g, w), (name, g, w)
    assert got[5] == want[5] == err
    return got


def rows_each(rows):
    return np.arange(rows, dtype=np.int32).reshape(rows, 1)


# (n, hops, R, B, eid_hi, k): rows = 3 B
SHAPES = {
    "one_entry": (1, 1, 1, 1, 3, 1),
    "four_entries": (1, 2, 2, 1, 2, 4),
    "24_entries": (3, 2, 2, 2, 5, 24),
    "count_below_k": (5, 2, 1, 3, 4, 8),
    "n20_pairs": (20, 2, 2, 4, 60, 20),
    "n20_rows": (20, 2, 1, 4, 60, 20),
    "one_hop_n20": (20, 1, 2, 4, 9, 20),
    "1122_entries": (33, 2, 1, 1, 200, 40),
    "4160_entries": (64, 2, 1, 1, 500, 64),
    "lds_bound_k64": (63, 2, 2, 1, 900, 64),
    "lds_bound_k8064": (63, 2, 2, 1, 900, 8064),
}


@pytest.mark.parametrize("mode", ER.MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_equals_restatement(dev, name, mode):
    n, hops, R, B, eid_hi, k = SHAPES[name]
    rng = np.random.default_rng(1000 * list(SHAPES).index(name) + ER.MODES.index(mode))
    imp, node, eid = ER.make_records(rng, 3 * B, n, hops, eid_hi, mode)
    groups = ER.pair_groups(B) if R == 2 else rows_each(3 * B)
    if name == "24_entries":
        # every pair holds one edge id as a hop-1 slot of its first row and a hop-2 slot of its second
        for a, b in groups:
            eid[a, 1], eid[b, n + 4], node[a, 1], node[b, n + 4] = 2, 2, 9, 9
    got = check_case(dev, imp, node, eid, n, hops, groups, k)
    if name == "count_below_k":
        assert (got[4] < k).all() and (got[0][:, -1] == 0).all() and (got[2][:, -1] == -1).all()
    if name == "24_entries":
        assert all(2 in e.tolist() for e in got[0])


def test_limits(dev):
    from tempme_amd import _lib as L
    n = 64
    imp, node, eid = ER.make_records(np.random.default_rng(5), 2, n, 2, 50)
    two = np.array([[0, 1]], np.int32)
    rc, *got = launch(dev, imp, node, eid, n, 2, two, 8)                # 2 x 4,160 entries
    assert rc == L.TM_E_UNSUPPORTED and "8192" in L.lib().tm_last_error().decode()
    assert (got[0] == SENT).all() and (got[4] == SENT).all()
    assert launch(dev, imp, node, eid, n, 2, rows_each(2), 0)[0] == L.TM_E_ARG          # k < 1
    assert launch(dev, imp, node, eid, n, 2, rows_each(2), 4161)[0] == L.TM_E_ARG       # k > R ne
    assert launch(dev, imp, node, eid, n, 3, rows_each(2), 8)[0] == L.TM_E_ARG          # hops
    rc, *got = launch(dev, imp, node, eid, n, 2, np.zeros((0, 1), np.int32), 8)         # no group: no launch
    assert rc == 0 and got[0].size == 0
    # the largest n with one row: 90 + 90^2 = 8,190 entries
    imp, node, eid = ER.make_records(np.random.default_rng(6), 3, 90, 2, 300)
    check_case(dev, imp, node, eid, 90, 2, rows_each(3), 90)


def test_dead_missing_and_out_of_range_rows(dev):
    n, B = 4, 2
    imp, node, eid = ER.make_records(np.random.default_rng(9), 3 * B, n, 2, 6, "slot")
    node[1] = 0                                                          # row 1 dead by its nodes
    eid[4] = np.where(np.arange(n + n * n) % 2, 0, -3)                   # row 4 dead by its edge ids
    groups = np.array([[1, 4], [1, -1], [0, -1], [-1, 2], [-1, -1], [3, 3]], np.int32)
    got = check_case(dev, imp, node, eid, n, 2, groups, 5)
    assert got[4][0] == got[4][1] == got[4][4] == 0 and got[4][2] > 0 and got[4][3] > 0
    assert (got[2][3][: min(got[4][3], 5)] >= n + n * n).all()           # slots of the second position
    # a row outside [-1, rows) sets the flag and counts as no row; the other groups are untouched
    bad = np.array([[0, 6], [2, 5], [-2, 3]], np.int32)
    got = check_case(dev, imp, node, eid, n, 2, bad, 5, err=ER.TM_E_ARG)
    assert got[4][1] > 0


def test_nan_and_signed_zeros(dev):
    nan = float("nan")
    n = 4
    # row 0: edge 1 (NaN, 2.0), edge 2 (-0.0, +0.0), edge 3 NaN only;  row 1: -0.0 alone on edge 7, +0.0 on edge 5,
    # -inf on edge 6: the zeros tie and order by edge id, ahead of -inf
    imp = np.array([[nan, -0.0, 2.0, nan, 0.0, -1.0] + [0.5] * 14,
                    [-0.0, 0.0, -math.inf, nan] + [nan] * 16], np.float32)
    eid = np.array([[1, 2, 1, 3, 2, 4] + [9] * 14, [7, 5, 6, 8] + [8] * 16], np.int32)
    node = np.ones((2, 20), np.int32)
    got = check_case(dev, imp, node, eid, n, 2, rows_each(2), 6)
    assert got[0][0].tolist() == [1, 9, 2, 4, 3, 0] and got[0][1].tolist() == [5, 7, 6, 8, 0, 0]
    assert got[1][0].tolist()[2] == 0 and got[1][1].tolist()[:2] == [0, 0]               # +0.0 bits
    assert got[1][0][4] == ER.QNAN_BITS and got[1][1][3] == ER.QNAN_BITS
    assert got[3][1].tolist() == [1, 1, 1, 17, 0, 0]


# ------------------------------------------------------------------ ranked_edges.ranked_edges
def side_lists(dev, node, eid, ts, B, n, hops):
    """per side (node, eid, time) records, each a list over hops, device tensors of rows [s B, (s + 1) B)"""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    cut = [slice(0, n), slice(n, None)][:hops]
    return [tuple([d(x[s * B:(s + 1) * B, c]) for c in cut] for x in (node, eid, ts)) for s in range(3)]


def expected_fields(imp, node, eid, ts, roots, n, hops, groups, k):
    """RankedEdges fields from the restatement's slots, numpy"""
    ne = imp.shape[1]
    w_eid, w_bits, w_slot, w_mult, w_count, _ = ER.ranked_edges_ref(imp, node, eid, groups, k)
    w_node, w_center = np.zeros_like(w_eid), np.zeros(w_eid.shape, np.int64)
    w_ts, w_hop = np.zeros(w_eid.shape, np.float64), np.zeros_like(w_eid)
    for g in range(w_eid.shape[0]):
        for j in range(k):
            if w_slot[g, j] < 0:
                continue
            p, s = divmod(int(w_slot[g, j]), ne)
            row = groups[g, p]
            w_node[g, j], w_ts[g, j], w_hop[g, j] = node[row, s], ts[row, s], 1 if s < n else 2
            w_center[g, j] = roots[row] if s < n else node[row, (s - n) // n]
    return dict(eid=w_eid, score=w_bits, node=w_node, center=w_center, ts=w_ts, hop=w_hop, mult=w_mult, count=w_count)


def assert_fields(got, want, shape):
    for name, w in want.items():
        g = getattr(got, name).cpu().numpy()
        g = g.view(np.uint32) if name == "score" else g
        assert g.shape == (shape if name == "count" else shape + (w.shape[-1],)), (name, g.shape)
        assert np.array_equal(g.reshape(w.shape), w), name


@pytest.fixture(scope="module")
def n20(dev):
    """the workload's N at a tiny B: records, times, roots and the explanation on the device"""
    B, n = 4, 20
    rng = np.random.default_rng(20)
    imp, node, eid = ER.make_records(rng, 3 * B, n, 2, 60, "slot")
    ts = rng.uniform(0, 1e6, imp.shape)
    roots = rng.integers(1, 50, 3 * B)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    expl = [d(imp[:, :n]), d(imp[:, n:])]
    root_l = [d(roots[s * B:(s + 1) * B]) for s in range(3)]
    return dict(B=B, n=n, imp=imp, node=node, eid=eid, ts=ts, roots=roots, expl=expl, root_l=root_l,
                subs=side_lists(dev, node, eid, ts, B, n, 2))


def test_wrapper_pairs_and_rows(dev, n20):
    import tempme_amd as tm
    c, B, n, k = n20, n20["B"], n20["n"], 20
    args = (c["imp"], c["node"], c["eid"], c["ts"], c["roots"], n, 2)
    got = tm.ranked_edges(c["expl"], c["subs"], c["root_l"], k)
    assert isinstance(got, tm.RankedEdges) and all(x.is_cuda for x in got)
    assert got.score.dtype == torch.float32 and got.ts.dtype == torch.float64 and got.center.dtype == torch.int64
    assert_fields(got, expected_fields(*args, ER.pair_groups(B), k), (2, B))
    # two launches agree bit for bit
    again = tm.ranked_edges(c["expl"], c["subs"], c["root_l"], k)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, again))
    rows = tm.ranked_edges(c["expl"], c["subs"], c["root_l"], k, pairs=False)
    assert_fields(rows, expected_fields(*args, rows_each(3 * B), k), (3 * B,))
    # the TGAT per-side six-list is the same explanation
    six = [c["expl"][h][s * B:(s + 1) * B] for s in range(3) for h in (0, 1)]
    tg = tm.ranked_edges(six, c["subs"], c["root_l"], k)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, tg))
    # a gathered pack's three sides ([3, B, ...] tensors indexed by side) give the same
    pack = [tuple([torch.stack([sg[i][h] for sg in c["subs"]]) for h in (0, 1)] for i in range(3))]
    packed = [tuple([x[h][s] for h in (0, 1)] for x in pack[0]) for s in range(3)]
    pk = tm.ranked_edges(c["expl"], packed, c["root_l"], k)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, pk))
    # explicit groups: a missing row, and an out-of-range row that only check=True reports
    grp = torch.tensor([[0, -1], [B, 2 * B]], dtype=torch.int32, device=dev)
    ex = tm.ranked_edges(c["expl"], c["subs"], c["root_l"], k, groups=grp)
    assert_fields(ex, expected_fields(*args, grp.cpu().numpy(), k), (2,))
    bad = torch.tensor([[0, 3 * B]], dtype=torch.int32, device=dev)
    tm.ranked_edges(c["expl"], c["subs"], c["root_l"], k, groups=bad)
    with pytest.raises(IndexError):
        tm.ranked_edges(c["expl"], c["subs"], c["root_l"], k, groups=bad, check=True)


def test_wrapper_one_hop(dev):
    import tempme_amd as tm
    B, n, k = 2, 6, 5
    rng = np.random.default_rng(3)
    imp, node, eid = ER.make_records(rng, 3 * B, n, 1, 5, "beta")
    ts, roots = rng.uniform(0, 100, imp.shape), rng.integers(1, 9, 3 * B)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    got = tm.ranked_edges([d(imp)], side_lists(dev, node, eid, ts, B, n, 1),
                          [d(roots[s * B:(s + 1) * B]) for s in range(3)], k)
    assert_fields(got, expected_fields(imp, node, eid, ts, roots, n, 1, ER.pair_groups(B), k), (2, B))
    assert (got.hop.cpu().numpy() <= 1).all()


def test_wrapper_argument_checks(dev, n20):
    import tempme_amd as tm
    c = n20
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm.ranked_edges([x.cpu() for x in c["expl"]], c["subs"], c["root_l"], 5)
    with pytest.raises(TypeError, match="float32"):
        tm.ranked_edges([x.double() for x in c["expl"]], c["subs"], c["root_l"], 5)
    with pytest.raises(ValueError, match="hop-2"):
        tm.ranked_edges([c["expl"][0], c["expl"][1][:, :-1]], c["subs"], c["root_l"], 5)
    with pytest.raises(ValueError, match="records"):
        tm.ranked_edges([x[:-3] for x in c["expl"]], c["subs"], c["root_l"], 5)
    with pytest.raises(ValueError, match="k = 0"):
        tm.ranked_edges(c["expl"], c["subs"], c["root_l"], 0)
    with pytest.raises(ValueError, match="k = 841"):
        tm.ranked_edges(c["expl"], c["subs"], c["root_l"], 841)
    # n = 64 with two rows is 8,320 entries: refused naming the bound; one row (4,160) runs
    n = 64
    imp, node, eid = ER.make_records(np.random.default_rng(1), 3, n, 2, 400)
    ts, roots = np.zeros(imp.shape), np.arange(1, 4)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    a = ([d(imp[:, :n]), d(imp[:, n:])], side_lists(dev, node, eid, ts, 1, n, 2), [d(roots[s:s + 1]) for s in range(3)])
    with pytest.raises(NotImplementedError, match="8192"):
        tm.ranked_edges(*a, 8)
    got = tm.ranked_edges(*a, 8, pairs=False)
    assert_fields(got, expected_fields(imp, node, eid, ts, roots, n, 2, rows_each(3), 8), (3,))


def test_one_kernel_per_call(dev, n20):
    import tempme_amd as tm
    from tempme_amd import _lib as L
    c = n20
    tm.ranked_edges(c["expl"], c["subs"], c["root_l"], 20)
    L.profile_enable(True)
    try:
        for pairs in (True, False, True):
            tm.ranked_edges(c["expl"], c["subs"], c["root_l"], 20, pairs=pairs)
        prof = L.profile_read()
    finally:
        L.profile_enable(False)
    assert set(prof) == {"ranked_edges_kernel"} and prof["ranked_edges_kernel"][1] == 3, prof


# ------------------------------------------------------------------ fidelity.kept_edges
@pytest.mark.parametrize("ratio", (0.05, 0.3))
def test_kept_edges_are_the_masked_subgraph(dev, n20, ratio):
    from types import SimpleNamespace

    from tempme_amd import _lib as L
    from tempme_amd import fidelity
    c, B, n = n20, n20["B"], n20["n"]
    ne = n + n * n
    args = SimpleNamespace(base_type="tgn", n_degree=n)
    # the masked node records straight from tm_mask_least_important
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    imp_d, node_d = d(c["imp"]), d(c["node"])
    top = min(max(math.ceil(ratio * ne), 1), ne)
    kd = torch.tensor([ne - top], dtype=torch.int32, device=dev)
    masked = torch.empty((1, 3 * B, ne), dtype=torch.int32, device=dev)
    L.check(L.lib().tm_mask_least_important(L.ptr(imp_d), 3 * B, ne, L.ptr(kd), 1, L.ptr(node_d), L.ptr(masked),
                                            L.stream_ptr(dev)), "mask")
    masked = masked[0].cpu().numpy()
    for pairs, groups, R in ((True, ER.pair_groups(B), 2), (False, rows_each(3 * B), 1)):
        got = fidelity.kept_edges(args, c["expl"], *c["subs"], c["root_l"], ratio, R * ne, pairs=pairs)
        g_eid, g_cnt = got.eid.cpu().numpy().reshape(len(groups), -1), got.count.cpu().numpy().reshape(-1)
        for g, rws in enumerate(groups):
            keep = np.concatenate([c["eid"][r][(masked[r] != 0) & (c["eid"][r] > 0)] for r in rws])
            want = np.unique(keep)
            assert g_cnt[g] == len(want) and g_cnt[g] <= top * R
            assert np.array_equal(np.sort(g_eid[g][:g_cnt[g]]), want) and (g_eid[g][g_cnt[g]:] == 0).all()
        # and it is ranked_edges of the restatement on those records
        want = ER.ranked_edges_ref(c["imp"], masked, c["eid"], groups, R * ne)
        assert np.array_equal(g_eid, want[0])
        assert np.array_equal(got.score.cpu().numpy().view(np.uint32).reshape(len(groups), -1), want[1])


# ------------------------------------------------------------------ ExplainPipeline.ranked_edges
def test_pipeline_ranked_edges(dev):
    import tempme_amd as tm
    from tempme_amd.pipeline import ExplainPipeline
    z = np.load(os.path.join(G, "synth_small.npz"))
    n_nodes, n_edges = int(max(z["src"].max(), z["dst"].max())) + 1, int(z["eidx"].max()) + 1
    f = tm.NeighborFinder.from_edges(z["src"], z["dst"], z["eidx"], z["ts"], n_nodes, device=dev, seed=1)
    rng = np.random.default_rng(0)

    class Base:
        n_feat_th = torch.from_numpy(rng.uniform(0, 1, (n_nodes, 172)).astype(np.float32))
        e_feat_th = torch.from_numpy(rng.uniform(0, 1, (n_edges, 32)).astype(np.float32))
        node_raw_features = torch.nn.Embedding.from_pretrained(n_feat_th, padding_idx=0, freeze=True)
        edge_raw_features = torch.nn.Embedding.from_pretrained(e_feat_th, padding_idx=0, freeze=True)

    torch.manual_seed(0)
    ex = tm.TempME(Base(), "tgn", "synth", 40, 64, device=dev,
                   null_model={k: 1 / 12 for k in range(1, 13)}).to(dev).eval()
    B, N, k = 4, 7, 10
    pipe = ExplainPipeline(ex, f.graph, torch.from_numpy(np.unique(z["dst"])), N, 3, B, seed=1)
    with pytest.raises(RuntimeError, match="nothing has run"):
        pipe.ranked_edges(k)
    s = slice(100, 100 + B)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[s], dtype=dt)).to(dev)  # noqa: E731
    src, dst = t(z["src"], np.int32), t(z["dst"], np.int32)
    _, h1, h2 = pipe.run(src, dst, t(z["ts"], np.float64), t(z["eidx"], np.int32),
                         torch.arange(B, dtype=torch.int32, device=dev))
    b = pipe.buf
    subs = [([b.sub1_node[i], b.sub2_node[i]], [b.sub1_eid[i], b.sub2_eid[i]], [b.sub1_ts[i], b.sub2_ts[i]])
            for i in range(3)]
    for pairs, shape in ((True, (2, B, k)), (False, (3 * B, k))):
        got = pipe.ranked_edges(k, pairs=pairs)
        want = tm.ranked_edges([h1.reshape(3 * B, N), h2.reshape(3 * B, N * N)], subs, (src, dst, b.dst_fake[:B]), k,
                               pairs=pairs)
        assert tuple(got.eid.shape) == shape and int(got.count.max()) > 0
        assert all(a.cpu().numpy().tobytes() == w.cpu().numpy().tobytes() for a, w in zip(got, want))
    pipe.check_errors()
    # against the restatement, from the buffers on the host
    h = lambda x, w: x.cpu().numpy().reshape(3 * B, w)                  # noqa: E731
    imp = np.concatenate([h(h1, N), h(h2, N * N)], 1)
    node = np.concatenate([h(b.sub1_node, N), h(b.sub2_node, N * N)], 1)
    eid = np.concatenate([h(b.sub1_eid, N), h(b.sub2_eid, N * N)], 1)
    want = ER.ranked_edges_ref(imp, node, eid, ER.pair_groups(B), k)
    got = pipe.ranked_edges(k)
    assert np.array_equal(got.eid.cpu().numpy().reshape(2 * B, k), want[0])
    assert np.array_equal(got.score.cpu().numpy().view(np.uint32).reshape(2 * B, k), want[1])
    assert np.array_equal(got.count.cpu().numpy().reshape(-1), want[4])
