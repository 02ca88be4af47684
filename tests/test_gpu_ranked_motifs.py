"""Ranked motif instances on the device: tm_ranked_motifs and tm_motif_mask (csrc/ranked_motifs.hip) through the C
ABI, ranked_motifs.ranked_motifs, ExplainPipeline.ranked_motifs, fidelity.motif_masked_nodes and
fidelity.motif_threshold_test against the numpy restatement (tests/ranked_motifs_ref.py).

The kernels only compare (the category sums are fp64 additions in a fixed order), so every output is checked with
np.array_equal, scores and cat_max as uint32 bit patterns, cat_sum as uint64: there is no tolerance.  Every output
sits between guard words.  Shapes are the smallest at which each mechanism can fail: one entry, a handful, a count that
is no power of two, fewer instances than k, the workload's W = 60 (N = 20, M = 3) as rows and as pairs, several waves
(W = 192 pairs) and the bound of 1,024 entries with k = 8 and k = 1,024.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ranked_motifs_ref as MR

pytestmark = pytest.mark.gpu

GUARD = 3
SENT = -77
OUTS = ("eid", "score", "walk", "mult", "cat", "count", "cat_n", "cat_max", "cat_sum")
ATOL, RTOL = 2e-5, 1e-5          # batched against single contrast, as tests/test_gpu_tgn.py holds it


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


def to_dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ tm_ranked_motifs through the C ABI
def launch(dev, eid3, cat, imp, group_rows, k, W=None, rows=None):
    """tm_ranked_motifs on host walks -> (rc, dict of numpy outputs in the restatement's layout, err flag); the outputs
    sit in windows of guarded buffers."""
    from tempme_amd import _lib as L
    rows = imp.shape[0] if rows is None else rows
    W = imp.shape[1] if W is None else W
    n_groups, R = group_rows.shape
    kk = max(k, 0)
    sizes = dict(eid=n_groups * kk * 3, score=n_groups * kk, walk=n_groups * kk, mult=n_groups * kk,
                 cat=n_groups * kk, count=n_groups, cat_n=n_groups * 12, cat_max=n_groups * 12, cat_sum=n_groups * 12)
    dts = dict(score=torch.float32, cat_max=torch.float32, cat_sum=torch.float64)
    bufs = {n: torch.full((sizes[n] + 2 * GUARD,), SENT, dtype=dts.get(n, torch.int32), device=dev) for n in OUTS}
    win = lambda b: C.c_void_p(b.data_ptr() + b.element_size() * GUARD)      # noqa: E731
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d_eid, d_cat, d_imp, d_grp = (to_dev(dev, x) for x in (eid3, cat, imp, group_rows))
    rc = L.lib().tm_ranked_motifs(L.ptr(d_eid), L.ptr(d_cat), L.ptr(d_imp), rows, W, L.ptr(d_grp), n_groups, R, k,
                                  *[win(bufs[n]) for n in OUTS], L.ptr(flag), L.stream_ptr(dev))
    out = {}
    for n in OUTS:
        h = bufs[n].cpu().numpy()
        m = sizes[n]
        assert (h[:GUARD] == SENT).all() and (h[GUARD + m:] == SENT).all(), f"a guard word around {n} was written"
        out[n] = h[GUARD:GUARD + m]
    shapes = dict(eid=(n_groups, kk, 3), count=(n_groups,), cat_n=(n_groups, 12), cat_max=(n_groups, 12),
                  cat_sum=(n_groups, 12))
    views = dict(score=np.uint32, cat_max=np.uint32, cat_sum=np.uint64)
    for n in OUTS:
        out[n] = out[n].view(views.get(n, out[n].dtype)).reshape(shapes.get(n, (n_groups, kk)))
    return rc, out, int(flag.item())


def check_case(dev, eid3, cat, imp, group_rows, k, err=0):
    want = MR.ranked_motifs_ref(eid3, cat, imp, group_rows, k)
    rc, got, flag = launch(dev, eid3, cat, imp, group_rows, k)
    assert rc == 0
    for n in OUTS:
        assert np.array_equal(got[n], want[n]), (n, got[n], want[n])
    assert flag == want["err"] == err
    return got


# (W, R, B, eid_hi, k): rows = 3 B
SHAPES = {
    "one_entry": (1, 1, 1, 2, 1),
    "eight_entries": (4, 2, 1, 2, 8),
    "24_entries": (12, 2, 2, 2, 24),
    "count_below_k": (10, 1, 3, 1, 10),
    "w60_pairs": (60, 2, 4, 4, 20),
    "w60_rows": (60, 1, 4, 4, 20),
    "w192_pairs": (192, 2, 1, 6, 64),
    "bound_k8": (512, 2, 1, 8, 8),
    "bound_k1024": (512, 2, 1, 8, 1024),
}


@pytest.mark.parametrize("mode", MR.MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_equals_restatement(dev, name, mode):
    W, R, B, eid_hi, k = SHAPES[name]
    rng = np.random.default_rng(1000 * list(SHAPES).index(name) + MR.MODES.index(mode))
    eid3, cat, imp = MR.make_walks(rng, 3 * B, W, eid_hi, mode)
    groups = MR.pair_groups(B) if R == 2 else MR.rows_each(3 * B)
    if name == "eight_entries":
        # both pairs hold one instance in each of their rows
        for a, b in groups:
            eid3[a, 1], eid3[b, 2], cat[a, 1], cat[b, 2] = (2, 2, 1), (2, 2, 1), 5, 5
    got = check_case(dev, eid3, cat, imp, groups, k)
    if name == "count_below_k":
        assert (got["count"] < k).all() and (got["walk"][:, -1] == -1).all() and (got["cat"][:, -1] == -1).all()
    if name == "eight_entries":
        for g in range(len(groups)):
            j = got["eid"][g].tolist().index([2, 2, 1])
            assert got["mult"][g, j] >= 2 and got["walk"][g, j] < W
    if name == "24_entries":
        assert any(c & (c - 1) for c in got["count"].tolist())           # a count that is no power of two
    if name in ("w60_pairs", "bound_k8"):
        # two launches agree bit for bit
        again = launch(dev, eid3, cat, imp, groups, k)[1]
        assert all(got[n].tobytes() == again[n].tobytes() for n in OUTS)


def test_limits(dev):
    from tempme_amd import _lib as L
    eid3, cat, imp = MR.make_walks(np.random.default_rng(5), 2, 513, 4)
    rc, got, _ = launch(dev, eid3, cat, imp, np.array([[0, 1]], np.int32), 8)            # 1,026 entries
    assert rc == L.TM_E_UNSUPPORTED and "1024" in L.lib().tm_last_error().decode()
    assert (got["eid"] == SENT).all() and (got["count"] == SENT).all() and (got["cat_n"] == SENT).all()
    eid3, cat, imp = MR.make_walks(np.random.default_rng(6), 2, 1025, 4)
    rc, got, _ = launch(dev, eid3, cat, imp, MR.rows_each(2), 8)                          # 1,025 entries
    assert rc == L.TM_E_UNSUPPORTED and "1024" in L.lib().tm_last_error().decode()
    assert (got["eid"] == SENT).all() and (got["walk"] == SENT).all() and (got["count"] == SENT).all()
    eid3, cat, imp = MR.make_walks(np.random.default_rng(7), 2, 6, 4)
    for k, grp in ((0, MR.rows_each(2)), (7, MR.rows_each(2)), (13, np.array([[0, 1]], np.int32))):
        rc, got, _ = launch(dev, eid3, cat, imp, grp, k)                                  # k < 1, k > R W
        assert rc == L.TM_E_ARG
        assert (got["eid"] == SENT).all() and (got["count"] == SENT).all() and (got["cat_sum"].view(np.float64)
                                                                                 == SENT).all()
    assert launch(dev, eid3, cat, imp, np.zeros((1, 3), np.int32), 2)[0] == L.TM_E_ARG    # R = 3
    assert launch(dev, eid3, cat, imp, MR.rows_each(2), 1, W=0)[0] == L.TM_E_ARG          # W < 1
    rc, got, _ = launch(dev, eid3, cat, imp, np.zeros((0, 1), np.int32), 2)               # no group: no launch
    assert rc == 0 and got["eid"].size == 0
    check_case(dev, eid3, cat, imp, np.array([[0, 1]], np.int32), 12)                     # k = R W runs


def test_missing_and_out_of_range_rows(dev):
    W, B = 5, 2
    eid3, cat, imp = MR.make_walks(np.random.default_rng(9), 3 * B, W, 2, "walk")
    eid3[1] = 0                                                          # row 1: padding walks only
    groups = np.array([[1, 4], [1, -1], [0, -1], [-1, 2], [-1, -1], [3, 3]], np.int32)
    got = check_case(dev, eid3, cat, imp, groups, 5)
    assert got["count"][1] == got["count"][4] == 0 and got["count"][2] > 0 and got["count"][3] > 0
    assert (got["walk"][3][:got["count"][3]] >= W).all()                 # entries of the second position
    assert (got["mult"][5][:got["count"][5]] % 2 == 0).all()             # the same row twice: every walk twice
    # a row outside [-1, rows) sets the flag and counts as no row; the other groups are right
    bad = np.array([[0, 6], [2, 5], [-2, 3]], np.int32)
    got = check_case(dev, eid3, cat, imp, bad, 5, err=MR.TM_E_ARG)
    assert got["count"][1] > 0


def test_categories_out_of_range(dev):
    W = 6
    eid3, cat, imp = MR.make_walks(np.random.default_rng(11), 3, W, 2, "walk", dead=0.0)
    good = check_case(dev, eid3, cat, imp, MR.rows_each(3), W)
    cat[0, 2], cat[2, 0] = 12, -1
    got = check_case(dev, eid3, cat, imp, MR.rows_each(3), W, err=MR.TM_E_ARG)
    # the walk is excluded everywhere: one entry fewer in the profile, the untouched row as before
    assert got["cat_n"][0].sum() == W - 1 and got["cat_n"][2].sum() == W - 1 and got["mult"][0].sum() == W - 1
    assert all(np.array_equal(got[n][1], good[n][1]) for n in OUTS)


def test_large_ids_and_the_third_position(dev):
    big = 2 ** 31 - 1
    # equal in the first two ids, different in the third; ids near 2^31 - 1; one score everywhere: the order is the
    # triples' own, all 96 bits
    triples = [(big, big, big), (big, big, big - 1), (big, big - 1, big), (big - 1, big, big), (big, big, 0),
               (big, big, big - 1), (7, big, 1), (big, big, big)]
    eid3 = np.array([triples], np.int32)
    cat = np.array([[i % 12 for i in range(8)]], np.int32)
    imp = np.full((1, 8), 0.5, np.float32)
    got = check_case(dev, eid3, cat, imp, MR.rows_each(1), 8)
    assert got["count"][0] == 6
    assert got["eid"][0].tolist()[:6] == [list(t) for t in sorted(set(triples))]
    assert got["mult"][0].tolist() == [1, 1, 1, 1, 2, 2, 0, 0] and got["walk"][0].tolist()[4:6] == [1, 0]
    # a negative later id compares as unsigned
    eid3 = np.array([[(7, -1, 0), (7, big, 0), (7, big, -2 ** 31)]], np.int32)
    got = check_case(dev, eid3, np.zeros((1, 3), np.int32), np.ones((1, 3), np.float32), MR.rows_each(1), 3)
    assert got["walk"][0].tolist() == [1, 2, 0]


def test_nan_and_signed_zeros(dev):
    nan = float("nan")
    eid3 = np.array([[(1, 1, 1), (2, 2, 2), (1, 1, 1), (3, 3, 3), (2, 2, 2), (4, 4, 4), (5, 5, 5)],
                     [(7, 0, 0), (5, 0, 0), (6, 0, 0), (8, 1, 1), (8, 1, 1), (8, 1, 1), (0, 0, 0)]], np.int32)
    cat = np.array([[0, 1, 0, 2, 1, 1, 2], [3, 3, 3, 4, 4, 4, 0]], np.int32)
    imp = np.array([[nan, -0.0, 2.0, nan, 0.0, -0.0, -math.inf], [-0.0, 0.0, -math.inf, nan, nan, nan, 1.0]],
                   np.float32)
    got = check_case(dev, eid3, cat, imp, MR.rows_each(2), 7)
    assert [t[0] for t in got["eid"][0].tolist()] == [1, 2, 4, 5, 3, 0, 0]
    assert [t[0] for t in got["eid"][1].tolist()] == [5, 7, 6, 8, 0, 0, 0]
    assert got["score"][0].tolist()[1:3] == [0, 0] and got["score"][1].tolist()[:2] == [0, 0]     # +0.0 bits
    assert got["score"][0][4] == MR.QNAN_BITS and got["score"][1][3] == MR.QNAN_BITS
    assert got["cat_max"][1][4] == MR.QNAN_BITS and got["cat_n"][1][4] == 3 and got["cat_sum"][1][4] == 0
    assert got["cat_max"][0][1] == 0 and got["cat_sum"][0][1] == 0                                # zeros: +0.0
    # both rows as one pair
    check_case(dev, eid3, cat, imp, np.array([[0, 1], [1, 0]], np.int32), 14)


# ------------------------------------------------------------------ tm_motif_mask through the C ABI
def mask_launch(dev, ranked, count, node, eid, m_list):
    from tempme_amd import _lib as L
    rows, k, _ = ranked.shape
    ne = node.shape[1]
    n = len(m_list) * rows * ne
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
    d = [to_dev(dev, x) for x in (ranked, count, node, eid)]
    ms = np.asarray(m_list, np.int32)
    rc = L.lib().tm_motif_mask(L.ptr(d[0]), L.ptr(d[1]), rows, k, L.ptr(d[2]), L.ptr(d[3]), ne, ms.ctypes.data,
                               len(m_list), C.c_void_p(buf.data_ptr() + 4 * GUARD), L.stream_ptr(dev))
    h = buf.cpu().numpy()
    assert (h[:GUARD] == SENT).all() and (h[GUARD + n:] == SENT).all(), "a guard word around the mask was written"
    return rc, h[GUARD:GUARD + n].reshape(len(m_list), rows, ne)


def subgraph_records(rng, rows, n, hops, eid_hi):
    ne = n + n * n if hops == 2 else n
    node = rng.integers(1, 50, (rows, ne)).astype(np.int32)
    node[rng.uniform(size=node.shape) < 0.2] = 0
    eid = rng.integers(-1, eid_hi + 1, (rows, ne)).astype(np.int32)
    return node, eid


@pytest.mark.parametrize("hops", (1, 2))
@pytest.mark.parametrize("n", (3, 20))
def test_mask_equals_restatement(dev, n, hops):
    from tempme_amd import _lib as L
    rng = np.random.default_rng(100 * n + hops)
    rows, W, k = 6, 30, 8
    eid3, cat, imp = MR.make_walks(rng, rows, W, 5, "walk")
    eid3[2] = 0                                                          # a row with no live walk
    eid3[4, 2:] = eid3[4, 0]                                             # a row with two instances at the most
    node, eid = subgraph_records(rng, rows, n, hops, 5)
    r = MR.ranked_motifs_ref(eid3, cat, imp, MR.rows_each(rows), k)
    assert r["count"][2] == 0 and r["count"][4] <= 2 and r["count"].max() > k
    m_list = [1, 2, 3, k - 1, k]                                         # below, at and above the rows' counts
    rc, got = mask_launch(dev, r["eid"], r["count"], node, eid, m_list)
    assert rc == 0
    want = MR.motif_mask_ref(r["eid"], r["count"], node, eid, m_list)
    assert np.array_equal(got, want)
    assert (got[:, 2] == 0).all() and np.array_equal(got[2, 4], got[4, 4]) and (got[0] != got[4]).any()
    # the kernel's own ranking gives the same mask
    mine = launch(dev, eid3, cat, imp, MR.rows_each(rows), k)[1]
    assert np.array_equal(mask_launch(dev, mine["eid"], mine["count"], node, eid, m_list)[1], want)
    # refusals leave the output untouched
    for bad in ([0], [k + 1], [1] * 65):
        rc, got = mask_launch(dev, r["eid"], r["count"], node, eid, bad)
        assert rc == L.TM_E_ARG and (got == SENT).all()


# ------------------------------------------------------------------ ranked_motifs.ranked_motifs
def expected_fields(node6, eid3, ts3, cat, imp, groups, k):
    """RankedMotifs fields from the restatement's walks, numpy"""
    W = imp.shape[1]
    w = MR.ranked_motifs_ref(eid3, cat, imp, groups, k)
    G = groups.shape[0]
    w["node"], w["ts"] = np.zeros((G, k, 6), np.int32), np.zeros((G, k, 3), np.float64)
    for g in range(G):
        for j in range(k):
            if w["walk"][g, j] >= 0:
                p, i = divmod(int(w["walk"][g, j]), W)
                w["node"][g, j], w["ts"][g, j] = node6[groups[g, p], i], ts3[groups[g, p], i]
    del w["err"]
    return w


def assert_fields(got, want, shape):
    bits = dict(score=np.uint32, cat_max=np.uint32, cat_sum=np.uint64)
    for name, w in want.items():
        g = getattr(got, name).cpu().numpy()
        g = g.view(bits[name]) if name in bits else g
        assert g.shape == shape + w.shape[1:], (name, g.shape)
        assert np.array_equal(g.reshape(w.shape), w), name


@pytest.fixture(scope="module")
def enron_walks(dev):
    """the reference's walks of four Enron events at N = 20 (W = 60), as host arrays, and seeded scores"""
    import enron_inputs as EN
    B = 4
    d = EN.walks(EN.golden(), 20, bsz=B)
    sides = [(d[s]["node"], d[s]["eid"], d[s]["ts"], d[s]["cat"], d[s]["marg"]) for s in EN.SIDES]
    st = lambda i, dt: np.concatenate([np.asarray(s[i]) for s in sides]).astype(dt)      # noqa: E731
    node6, eid3, ts3 = st(0, np.int32), st(1, np.int32), st(2, np.float32)
    cat = st(3, np.int32).reshape(3 * B, -1)
    imp = (np.round(np.random.default_rng(4).uniform(size=cat.shape) * 16) / 16).astype(np.float32)
    return dict(B=B, W=cat.shape[1], sides=sides, node6=node6, eid3=eid3, ts3=ts3, cat=cat, imp=imp,
                imp_d=to_dev(dev, imp))


def test_wrapper_pairs_rows_and_groups(dev, enron_walks):
    import tempme_amd as tm
    c, B, W, k = enron_walks, enron_walks["B"], enron_walks["W"], 12
    rec = (c["node6"], c["eid3"], c["ts3"], c["cat"], c["imp"])
    assert (c["eid3"][:, :, 0] > 0).any() and W == 60
    got = tm.ranked_motifs(c["imp_d"].view(3, B, W), c["sides"], k)
    assert isinstance(got, tm.RankedMotifs) and all(x.is_cuda for x in got)
    assert got.score.dtype == torch.float32 and got.ts.dtype == torch.float64 and got.cat_sum.dtype == torch.float64
    assert_fields(got, expected_fields(*rec, MR.pair_groups(B), k), (2, B))
    # device tensors per side, [3B, W] scores, and one side-major tuple give the same bits
    dsides = [tuple(to_dev(dev, np.asarray(x)) for x in s[:4]) for s in c["sides"]]
    stacked = tuple(to_dev(dev, x).view(3, B, *x.shape[1:]) for x in (c["node6"], c["eid3"], c["ts3"], c["cat"]))
    for walks in (dsides, stacked):
        again = tm.ranked_motifs(c["imp_d"], walks, k)
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, again))
    rows = tm.ranked_motifs(c["imp_d"], c["sides"], k, pairs=False)
    assert_fields(rows, expected_fields(*rec, MR.rows_each(3 * B), k), (3 * B,))
    # explicit groups: a missing row, and an out-of-range row that only check=True reports
    grp = torch.tensor([[0, -1], [B, 2 * B], [5, 5]], dtype=torch.int32, device=dev)
    ex = tm.ranked_motifs(c["imp_d"], c["sides"], k, groups=grp)
    assert_fields(ex, expected_fields(*rec, grp.cpu().numpy(), k), (3,))
    bad = torch.tensor([[0, 3 * B]], dtype=torch.int32, device=dev)
    tm.ranked_motifs(c["imp_d"], c["sides"], k, groups=bad)
    with pytest.raises(IndexError):
        tm.ranked_motifs(c["imp_d"], c["sides"], k, groups=bad, check=True)


def test_wrapper_argument_checks(dev, enron_walks):
    import tempme_amd as tm
    c, B, W = enron_walks, enron_walks["B"], enron_walks["W"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm.ranked_motifs(c["imp_d"].cpu(), c["sides"], 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm.ranked_motifs(c["imp_d"], [tuple(torch.from_numpy(np.asarray(x)) for x in s[:4]) for s in c["sides"]], 5)
    with pytest.raises(TypeError, match="float32"):
        tm.ranked_motifs(c["imp_d"].double(), c["sides"], 5)
    with pytest.raises(ValueError, match="imp has shape"):
        tm.ranked_motifs(c["imp_d"].view(2, -1, W), c["sides"], 5)
    with pytest.raises(ValueError, match="rows and walks"):
        tm.ranked_motifs(c["imp_d"][:-3], c["sides"], 5, pairs=False)
    with pytest.raises(TypeError, match="three sides"):
        tm.ranked_motifs(c["imp_d"], c["sides"][:2], 5)
    with pytest.raises(ValueError, match="k = 0"):
        tm.ranked_motifs(c["imp_d"], c["sides"], 0)
    with pytest.raises(ValueError, match="k = 121"):
        tm.ranked_motifs(c["imp_d"], c["sides"], 121)
    with pytest.raises(ValueError, match="k = 61"):
        tm.ranked_motifs(c["imp_d"], c["sides"], 61, pairs=False)
    with pytest.raises(ValueError, match="groups has shape"):
        tm.ranked_motifs(c["imp_d"], c["sides"], 5, groups=torch.zeros((2, 3), dtype=torch.int32, device=dev))
    # W = 513 with two rows is 1,026 entries: refused naming the bound; one row runs
    eid3, cat, imp = MR.make_walks(np.random.default_rng(1), 3, 513, 6)
    walks = (torch.zeros((3, 1, 513, 6), dtype=torch.int32, device=dev), to_dev(dev, eid3).view(3, 1, 513, 3),
             torch.zeros((3, 1, 513, 3), dtype=torch.float32, device=dev), to_dev(dev, cat).view(3, 1, 513))
    with pytest.raises(NotImplementedError, match="1024"):
        tm.ranked_motifs(to_dev(dev, imp), walks, 8)
    got = tm.ranked_motifs(to_dev(dev, imp), walks, 8, pairs=False)
    want = MR.ranked_motifs_ref(eid3, cat, imp, MR.rows_each(3), 8)
    assert np.array_equal(got.eid.cpu().numpy(), want["eid"]) and np.array_equal(got.count.cpu().numpy(), want["count"])


def test_one_kernel_per_call(dev, enron_walks):
    import tempme_amd as tm
    from tempme_amd import _lib as L
    c = enron_walks
    tm.ranked_motifs(c["imp_d"], c["sides"], 12)
    L.profile_enable(True)
    try:
        for pairs in (True, False, True):
            tm.ranked_motifs(c["imp_d"], c["sides"], 12, pairs=pairs)
        prof = L.profile_read()
    finally:
        L.profile_enable(False)
    assert set(prof) == {"ranked_motifs_kernel"} and prof["ranked_motifs_kernel"][1] == 3, prof


# ------------------------------------------------------------------ ExplainPipeline.ranked_motifs
def test_pipeline_ranked_motifs(dev):
    import tempme_amd as tm
    from tempme_amd.pipeline import ExplainPipeline
    from tempme_amd.workload import enron_like, split
    g = enron_like(n_nodes=60, n_edges=3000, node_feat="uniform", seed=3)
    (src, dst, ts, eidx), rows, pool = split(g)
    f = tm.NeighborFinder.from_edges(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"],
                                     device=dev, seed=1)

    class Base:
        n_feat_th = torch.from_numpy(g["n_feat"])
        e_feat_th = torch.from_numpy(g["e_feat"])
        node_raw_features = torch.nn.Embedding.from_pretrained(n_feat_th, padding_idx=0, freeze=True)
        edge_raw_features = torch.nn.Embedding.from_pretrained(e_feat_th, padding_idx=0, freeze=True)

    torch.manual_seed(0)
    ex = tm.TempME(Base(), "tgn", "synth", 40, 64, device=dev,
                   null_model={k: 1 / 12 for k in range(1, 13)}).to(dev).eval()
    B, N, M, k = 4, 7, 3, 10
    W = N * M
    pipe = ExplainPipeline(ex, f.graph, to_dev(dev, pool.astype(np.int32)), N, M, B, seed=1)
    with pytest.raises(RuntimeError, match="nothing has run"):
        pipe.ranked_motifs(k)
    t = lambda a, dt: to_dev(dev, np.ascontiguousarray(a[:B], dtype=dt))                  # noqa: E731
    with torch.no_grad():
        imp, _, _ = pipe.run(t(src, np.int32), t(dst, np.int32), t(ts, np.float64), t(eidx, np.int32),
                             torch.arange(B, dtype=torch.int32, device=dev))
    b = pipe.buf
    sides = [(b.node6[s], b.eid3[s], b.ts3[s], b.cat[s]) for s in range(3)]
    for pairs, shape in ((True, (2, B, k)), (False, (3 * B, k))):
        got = pipe.ranked_motifs(k, pairs=pairs)
        want = tm.ranked_motifs(imp, sides, k, pairs=pairs)
        assert tuple(got.score.shape) == shape and int(got.count.max()) > 0
        assert all(a.cpu().numpy().tobytes() == w.cpu().numpy().tobytes() for a, w in zip(got, want))
    pipe.check_errors()
    # against the restatement, from the buffers on the host
    h = lambda x, *s: x.cpu().numpy().reshape(3 * B, W, *s)             # noqa: E731
    want = expected_fields(h(b.node6, 6), h(b.eid3, 3), h(b.ts3, 3), h(b.cat), h(imp), MR.pair_groups(B), k)
    assert_fields(pipe.ranked_motifs(k), want, (2, B))


# ------------------------------------------------------------------ fidelity.motif_threshold_test
def _tgn_case(dev):
    import tgn_inputs as TI
    d = TI.load_batch(bsz=8)
    m = TI.build_model("synth").to(dev)
    run = lambda sgs: m.contrast(d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], *sgs)   # noqa: E731
    expl = [x[:3 * 32].view(3, 32, -1)[:, :8].reshape(24, -1).to(dev) for x in TI.explanation("synth")]
    return SimpleNamespace(base="tgn", m=m, run=run, N=d["N"], B=8, hops=2, expl=expl, ratios=[0.1, 0.4],
                           batch=(d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"]),
                           sgs=(d["sg_src"], d["sg_tgt"], d["sg_bgd"]))


def _tgat_case(dev):
    import tgat_inputs as TA
    import tgn_inputs as TI
    d = TI.load_batch(bsz=8)
    m = TA.build_model("synth").to(dev)
    run = lambda sgs: m.contrast(d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], *sgs, test=True,  # noqa: E731
                                 if_explain=False)
    ex = [x[:3 * 32].view(3, 32, -1)[:, :8].to(dev) for x in TI.explanation("synth")]
    six = [ex[h][s].contiguous() for s in range(3) for h in (0, 1)]
    return SimpleNamespace(base="tgat", m=m, run=run, N=d["N"], B=8, hops=2, expl=six, ratios=[0.1, 0.4],
                           batch=(d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"]),
                           sgs=(d["sg_src"], d["sg_tgt"], d["sg_bgd"]))


def _graphmixer_case(dev):
    import gm_shape_inputs as S
    case = S.FUSED[0]
    inp = S.build(case)[0]
    m = S.make_model(inp, case.seed, dev).to(dev).eval()
    run = lambda sgs: m.contrast(inp.src, inp.dst, inp.fake, inp.cut, None, *sgs)         # noqa: E731
    return SimpleNamespace(base="graphmixer", m=m, run=run, N=inp.N, B=inp.B, hops=1, ratios=[0.2, 0.5],
                           expl=[to_dev(dev, inp.ew0)], batch=(inp.src, inp.dst, inp.fake, inp.cut, None),
                           sgs=tuple(inp.sgs))


def host_figures(logits, ori, y):
    """threshold_test's five figures of one masked copy from its logits [2B], the original logits [2B] and labels, on
    the host: sigmoids and means in fp64; AP, AUC and accuracy from the sigmoid rounded to fp32 (what the product
    ranks and thresholds)."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    B = len(logits) // 2
    sig = lambda x: 1.0 / (1.0 + np.exp(-x.astype(np.float64)))         # noqa: E731
    p, po = sig(logits), sig(ori)
    sign = np.concatenate([np.ones(B), -np.ones(B)])                     # pos - pos_ori, neg_ori - neg
    p32 = p.astype(np.float32)
    return np.array([average_precision_score(y, p32), roc_auc_score(y, p32), np.mean((p32 > 0.5) == (y > 0.5)),
                     np.mean(sign * (p - po)), np.mean(sign * (logits.astype(np.float64) - ori))])


@pytest.mark.parametrize("base", ("tgn", "graphmixer", "tgat"))
def test_motif_threshold_test(dev, base):
    """The batched contrast of every m against base_model.contrast run once per m on subgraphs masked by the numpy
    restatement (atol 2e-5 + rtol 1e-5, the project's bound for batched against single contrast), and the [Gm, 5]
    figures against the same figures computed on the host from those logits.  Bounds of the figures: AP and AUC are
    rank statistics of the same fp32 probabilities, summed in fp64 (1e-12); accuracy is a mean of 2B zeros and ones,
    exact in fp32 up to one rounding (1e-7); the fidelity figures are fp32 means of 2B fp32 differences against
    fp64 ones: (2B + 3) roundings of 6e-8 relative to the largest term, 2e-6 for probabilities (terms <= 1) and
    2e-6 max(1, |logit|) for logits at 2B <= 16."""
    from tempme_amd import fidelity
    c = {"tgn": _tgn_case, "graphmixer": _graphmixer_case, "tgat": _tgat_case}[base](dev)
    B, N, W = c.B, c.N, 8
    ne = N + N * N if c.hops == 2 else N
    rec = lambda i, dt: np.concatenate([np.concatenate([np.asarray(sg[i][h]) for h in range(c.hops)], 1)  # noqa: E731
                                        for sg in c.sgs]).astype(dt)
    node, eid = rec(0, np.int32), rec(1, np.int32)
    node6, eid3, ts3, cat, imp = MR.walks_from_subgraph(np.random.default_rng(77), eid, W)
    walks = [tuple(to_dev(dev, x[s * B:(s + 1) * B]) for x in (node6, eid3, ts3, cat)) for s in range(3)]
    imp_d = to_dev(dev, imp)
    m_list = [1, 2, W - 2, W - 1]
    args = SimpleNamespace(base_type=c.base, n_degree=N, bs=B, ratios=c.ratios)

    # the restatement's masks, the kernel's masks through the Python surface
    r = MR.ranked_motifs_ref(eid3, cat, imp, MR.rows_each(3 * B), W - 1)
    assert 2 < r["count"].max() <= W - 2                                 # m = W - 2 and W - 1 both keep every motif
    want_mask = MR.motif_mask_ref(r["eid"], r["count"], node, eid, m_list)
    import tempme_amd as tm
    ranked = tm.ranked_motifs(imp_d, walks, W - 1, pairs=False)
    got_mask = fidelity.motif_masked_nodes(ranked, c.sgs, N, m_list, c.hops)
    assert tuple(got_mask.shape) == (len(m_list), 3 * B, ne) and np.array_equal(got_mask.cpu().numpy(), want_mask)
    assert (want_mask[0] != want_mask[2]).any() and (want_mask[2] != node).any() and want_mask[2].any()

    with torch.no_grad():
        pos, neg = fidelity.motif_masked_contrast(args, imp_d, walks, c.m, *c.batch[:4], *c.sgs, m_list)
        logits = torch.cat([pos, neg], dim=1).cpu().numpy()
        assert logits.shape == (len(m_list), 2 * B)
        for g in range(len(m_list)):
            sgs = []
            for s, sg in enumerate(c.sgs):
                rows = want_mask[g, s * B:(s + 1) * B].astype(np.float64)
                nodes = [rows[:, :N], rows[:, N:]] if c.hops == 2 else [rows, None]
                sgs.append((nodes, sg[1], sg[2]))
            p, n = c.run(sgs)
            single = torch.cat([p.reshape(-1), n.reshape(-1)]).cpu().numpy()
            print(base, "m =", m_list[g], "max |batched - single| =", float(np.abs(logits[g] - single).max()))
            np.testing.assert_allclose(logits[g], single, atol=ATOL, rtol=RTOL)
        ori_t = torch.cat([x.reshape(-1) for x in c.run(c.sgs)])
    ori = ori_t.cpu().numpy()
    y_ori = torch.cat([torch.ones(B), torch.zeros(B)]).to(dev).view(-1, 1)   # both classes: AUC is defined
    y = y_ori.cpu().numpy().reshape(-1)
    a = (args, imp_d, walks, c.m, *c.batch, ori_t[:B], ori_t[B:], y_ori, *c.sgs, m_list)
    host = fidelity.motif_threshold_test(*a)
    devm = fidelity.motif_threshold_test(*a, device_metrics=True)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and host.shape == (len(m_list), 5)
    assert devm.is_cuda and devm.dtype == torch.float64 and tuple(devm.shape) == (len(m_list), 5)
    want = np.stack([host_figures(logits[g], ori, y) for g in range(len(m_list))])
    scale = max(1.0, float(np.abs(logits).max()), float(np.abs(ori).max()))
    tol = np.array([1e-12, 1e-12, 1e-7, 2e-6, 2e-6 * scale])
    for got in (host, devm.cpu().numpy()):
        print(base, "figures off by", np.abs(got - want).max(0))
        assert (np.abs(got - want) <= tol).all(), (got, want)
    # every row's count is at most W - 2: m = W - 2 and m = W - 1 are the same subgraphs, the same bits
    assert logits[2].tobytes() == logits[3].tobytes()
    assert host[2].tobytes() == host[3].tobytes() and devm[2].cpu().numpy().tobytes() == devm[3].cpu().numpy().tobytes()
    # a larger k (the default is max(m_list) = W - 1) changes nothing
    again = fidelity.motif_threshold_test(*a, k=W)
    assert again.tobytes() == host.tobytes()

    # threshold_test on the same case: its figures are the means over ratios of the same per-ratio terms, computed
    # here as the function computed them before its tail moved into a helper
    fns = {"tgn": fidelity.masked_contrast, "graphmixer": fidelity.masked_contrast_graphmixer,
           "tgat": fidelity.masked_contrast_tgat}
    thr = fidelity.threshold_test(args, c.expl, c.m, *c.batch, ori_t[:B], ori_t[B:], y_ori, *c.sgs)
    thr_dev = fidelity.threshold_test(args, c.expl, c.m, *c.batch, ori_t[:B], ori_t[B:], y_ori, *c.sgs,
                                      device_metrics=True)
    with torch.no_grad():
        pos, neg = fns[base](c.m, c.expl, *c.batch[:4], *c.sgs, N, c.ratios)
        po, no = ori_t[:B].reshape(1, -1), ori_t[B:].reshape(1, -1)
        fid_prob = torch.cat([pos.sigmoid() - po.sigmoid(), no.sigmoid() - neg.sigmoid()], dim=1).mean(1)
        fid_logit = torch.cat([pos - po, no - neg], dim=1).mean(1)
        y_pred = torch.cat([pos, neg], dim=1).sigmoid()
        acc = (torch.where(y_pred > 0.5, 1., 0.) == y_ori.reshape(1, -1)).float().mean(1)
        rm = tm.rank_metrics(y_ori.reshape(-1), y_pred).mean(0)
        want_dev = torch.cat([rm, torch.stack([acc.mean(), fid_prob.mean(), fid_logit.mean()]).double()])
    print(base, "threshold_test", [repr(float(x)) for x in thr])
    assert thr_dev.cpu().numpy().tobytes() == want_dev.cpu().numpy().tobytes()
    assert thr[2:] == (float(acc.mean().item()), float(fid_prob.mean().item()), float(fid_logit.mean().item()))
    assert abs(thr[0] - float(rm[0])) <= 1e-12 and abs(thr[1] - float(rm[1])) <= 1e-12
