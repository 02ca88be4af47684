"""Ranked explanation edges, the parts that need no device: the numpy restatement of tm_ranked_edges
(tests/ranked_edges_ref.py) against a brute-force set-and-sort restatement written here, the C-ABI symbol and the
public name, and the CPU-tensor refusal.  Everything is compared exactly."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import ranked_edges_ref as ER

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(imp, node, eid, group_rows, k):
    """The same semantics the long way round: every live entry listed, the edge ids as a set, each edge's entries
    filtered out of the list again, the edges ordered by a pairwise comparison."""
    rows, ne = imp.shape
    out = []
    for rws in group_rows:
        entries = [(int(eid[r, s]), p * ne + s, np.float32(imp[r, s]))
                   for p, r in enumerate(rws) if 0 <= r < rows
                   for s in range(ne) if node[r, s] != 0 and eid[r, s] > 0]
        edges = []
        for e in set(x[0] for x in entries):
            mine = [x for x in entries if x[0] == e]
            nums = [x[2] for x in mine if not np.isnan(x[2])]
            edges.append((e, max(nums) if nums else np.float32("nan"), min(x[1] for x in mine), len(mine)))

        def cmp(a, b):
            an, bn = np.isnan(a[1]), np.isnan(b[1])
            if an != bn:
                return 1 if an else -1
            if not an and a[1] != b[1]:
                return -1 if a[1] > b[1] else 1
            return a[0] - b[0]
        edges.sort(key=functools.cmp_to_key(cmp))
        pad = [(0, np.float32(0.0), -1, 0)] * max(0, k - len(edges))
        out.append((len(edges), (edges + pad)[:k]))
    return out


def bits(f):
    return ER.QNAN_BITS if np.isnan(f) else 0 if f == 0 else int(np.float32(f).view(np.uint32))


@pytest.mark.parametrize("seed", range(10))
def test_restatement_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    n, hops, R = int(rng.integers(1, 5)), int(rng.integers(1, 3)), int(rng.integers(1, 3))
    rows, G = 5, 4
    imp, node, eid = ER.make_records(rng, rows, n, hops, 4, ER.MODES[seed % 3], dead=0.3)
    flat = imp.reshape(-1)
    flat[rng.integers(0, flat.size, 3)] = (np.nan, -0.0, 0.0)          # special scores among the ordinary ones
    if seed % 2:
        node[2] = 0                                                      # a dead row
    group_rows = rng.integers(-1, rows, (G, R)).astype(np.int32)
    ne = imp.shape[1]
    k = int(rng.integers(1, R * ne + 1))
    g_eid, g_bits, g_slot, g_mult, g_count, err = ER.ranked_edges_ref(imp, node, eid, group_rows, k)
    assert err == 0
    want = brute_force(imp, node, eid, group_rows, k)
    for g, (count, edges) in enumerate(want):
        assert g_count[g] == count
        assert g_eid[g].tolist() == [x[0] for x in edges]
        assert g_bits[g].tolist() == [bits(x[1]) for x in edges]
        assert g_slot[g].tolist() == [x[2] for x in edges]
        assert g_mult[g].tolist() == [x[3] for x in edges]


def test_restatement_special_scores():
    nan, inf = float("nan"), float("inf")
    # one row of six slots: edge 1 carries (NaN, 2.0), edge 2 (-0.0, +0.0), edge 3 NaN only, edge 4 -inf, slot 5 dead
    imp = np.array([[nan, -0.0, 2.0, nan, 0.0, -inf, 9.0]], np.float32)
    eid = np.array([[1, 2, 1, 3, 2, 4, 5]], np.int32)
    node = np.array([[7, 7, 7, 7, 7, 7, 0]], np.int32)
    e, b, s, m, c, err = ER.ranked_edges_ref(imp, node, eid, np.array([[0]], np.int32), 6)
    f = b.view(np.float32)
    assert c[0] == 4 and err == 0
    assert e[0].tolist() == [1, 2, 4, 3, 0, 0] and s[0].tolist() == [0, 1, 5, 3, -1, -1]
    assert m[0].tolist() == [2, 2, 1, 1, 0, 0]
    assert f[0, 0] == 2.0 and b[0, 1] == 0 and f[0, 2] == -inf and b[0, 3] == ER.QNAN_BITS and b[0, 4] == 0
    assert not math.copysign(1.0, f[0, 1]) < 0                          # a zero maximum is +0.0
    # an out-of-range row is flagged and skipped, -1 is skipped silently
    assert ER.ranked_edges_ref(imp, node, eid, np.array([[1, 0]], np.int32), 2)[5] == ER.TM_E_ARG
    assert ER.ranked_edges_ref(imp, node, eid, np.array([[-1, 0]], np.int32), 2)[5] == 0


def test_symbol_in_header_and_exports():
    from tempme_amd import _lib
    src = open(os.path.join(REPO, "include", "tempme.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+tm_ranked_edges\s*\(", src)
    assert "tm_ranked_edges" in _lib.EXPORTS
    import tempme_amd
    assert hasattr(tempme_amd.lib(), "tm_ranked_edges")
    assert tempme_amd.lib().tm_version() == 3
    from tempme_amd.ranked_edges import RankedEdges, ranked_edges
    assert tempme_amd.ranked_edges is ranked_edges and tempme_amd.RankedEdges is RankedEdges
    assert RankedEdges._fields == ("eid", "score", "node", "center", "ts", "hop", "mult", "count")
    from tempme_amd import fidelity, pipeline
    assert callable(fidelity.kept_edges) and callable(pipeline.ExplainPipeline.ranked_edges)


def test_ranked_edges_refuses_cpu_tensors():
    import tempme_amd
    n = 2
    sub = ([torch.ones(1, n, dtype=torch.int32)], [torch.ones(1, n, dtype=torch.int32)], [torch.zeros(1, n)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tempme_amd.ranked_edges([torch.rand(1, n)], (sub,), (torch.ones(1),), 1, pairs=False)
