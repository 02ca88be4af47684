"""Ranked motif instances, the parts that need no device: hand-worked cases of the numpy restatement of
tm_ranked_motifs and tm_motif_mask (tests/ranked_motifs_ref.py), the C-ABI symbols and the public names, and the
refusal of CPU tensors.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import ranked_motifs_ref as MR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def bits(f):
    return int(np.float32(f).view(np.uint32))


def one_row(triples, cats, scores):
    eid3 = np.array([triples], np.int32)
    return eid3, np.array([cats], np.int32), np.array([scores], np.float32)


def test_duplicates_share_one_instance():
    # (1,2,3) sits in walks 0, 2 and 4 with scores 0.5, 0.75, 0.25; (4,5,0) once; walk 3 is padding
    eid3, cat, imp = one_row([(1, 2, 3), (4, 5, 0), (1, 2, 3), (0, 0, 0), (1, 2, 3)], [3, 7, 3, 0, 3],
                             [0.5, 0.625, 0.75, 9.0, 0.25])
    o = MR.ranked_motifs_ref(eid3, cat, imp, np.array([[0]], np.int32), 3)
    assert o["count"].tolist() == [2] and o["err"] == 0
    assert o["eid"][0].tolist() == [[1, 2, 3], [4, 5, 0], [0, 0, 0]]
    assert o["score"][0].tolist() == [bits(0.75), bits(0.625), 0]
    assert o["walk"][0].tolist() == [0, 1, -1] and o["mult"][0].tolist() == [3, 1, 0]
    assert o["cat"][0].tolist() == [3, 7, -1]
    # the profile counts entries, not instances; the padding walk (score 9) is in no category
    assert o["cat_n"][0].tolist() == [0, 0, 0, 3, 0, 0, 0, 1, 0, 0, 0, 0]
    assert o["cat_max"][0, 3] == bits(0.75) and o["cat_max"][0, 7] == bits(0.625) and o["cat_max"][0, 0] == 0
    assert o["cat_sum"][0, 3] == np.float64(1.5).view(np.uint64) and o["cat_sum"][0, 0] == 0


def test_ties_are_broken_by_the_triple_and_the_third_id_counts():
    # four instances at one score: ordered by the triple, ids unsigned; (7,8,9) and (7,8,10) differ in the third id only
    big = 2 ** 31 - 1
    eid3, cat, imp = one_row([(7, 8, 10), (big, 1, 1), (7, 8, 9), (7, 0, 0), (7, 8, 9)], [1, 1, 2, 2, 2],
                             [0.5, 0.5, 0.5, 0.5, 0.5])
    o = MR.ranked_motifs_ref(eid3, cat, imp, np.array([[0]], np.int32), 5)
    assert o["count"].tolist() == [4]
    assert o["eid"][0].tolist() == [[7, 0, 0], [7, 8, 9], [7, 8, 10], [big, 1, 1], [0, 0, 0]]
    assert o["walk"][0].tolist() == [3, 2, 0, 1, -1] and o["mult"][0].tolist() == [1, 2, 1, 1, 0]
    # a negative later id compares as unsigned: after every positive one
    eid3, cat, imp = one_row([(7, -1, 0), (7, big, 0)], [0, 0], [1.0, 1.0])
    o = MR.ranked_motifs_ref(eid3, cat, imp, np.array([[0]], np.int32), 2)
    assert o["eid"][0].tolist() == [[7, big, 0], [7, -1, 0]]


def test_nan_and_signed_zeros():
    # (1,1,1): NaN and 2.0 -> 2.0;  (2,2,2): -0.0 and +0.0 -> +0.0;  (3,3,3): NaN only -> the quiet NaN, last;
    # (4,4,4): -0.0 alone -> +0.0, tied with (2,2,2) and after it;  (5,5,5): -inf, after the zeros, before the NaN
    eid3, cat, imp = one_row([(1, 1, 1), (2, 2, 2), (1, 1, 1), (3, 3, 3), (2, 2, 2), (4, 4, 4), (5, 5, 5)],
                             [0, 1, 0, 2, 1, 1, 2], [NAN, -0.0, 2.0, NAN, 0.0, -0.0, -math.inf])
    o = MR.ranked_motifs_ref(eid3, cat, imp, np.array([[0]], np.int32), 7)
    assert o["count"].tolist() == [5]
    assert [t[0] for t in o["eid"][0].tolist()] == [1, 2, 4, 5, 3, 0, 0]
    assert o["score"][0].tolist() == [bits(2.0), 0, 0, bits(-math.inf), MR.QNAN_BITS, 0, 0]
    assert o["cat_n"][0].tolist()[:3] == [2, 3, 2]
    assert o["cat_max"][0].tolist()[:3] == [bits(2.0), 0, bits(-math.inf)]
    # NaN scores stay out of the sums; -0.0 + 0.0 + -0.0 from a +0.0 accumulator is +0.0
    assert o["cat_sum"][0].tolist()[:3] == [int(np.float64(2.0).view(np.uint64)), 0,
                                            int(np.float64(-math.inf).view(np.uint64))]


def test_pairs_missing_rows_and_bad_categories():
    eid3 = np.array([[(1, 2, 3), (4, 4, 4)], [(4, 4, 4), (1, 2, 3)], [(9, 9, 9), (8, 8, 8)]], np.int32)
    cat = np.array([[0, 1], [1, 0], [12, -1]], np.int32)
    imp = np.array([[0.25, 0.5], [0.75, 0.125], [1.0, 1.0]], np.float32)
    o = MR.ranked_motifs_ref(eid3, cat, imp, np.array([[0, 1], [1, -1], [-1, -1]], np.int32), 4)
    # an instance shared by both rows of the pair: entries 1 and 2 carry (4,4,4), entries 0 and 3 carry (1,2,3)
    assert o["count"].tolist() == [2, 2, 0] and o["err"] == 0
    assert o["eid"][0].tolist() == [[4, 4, 4], [1, 2, 3], [0, 0, 0], [0, 0, 0]]
    assert o["walk"][0].tolist() == [1, 0, -1, -1] and o["mult"][0].tolist() == [2, 2, 0, 0]
    assert o["score"][0].tolist()[:2] == [bits(0.75), bits(0.25)]
    assert o["walk"][1].tolist() == [0, 1, -1, -1]
    assert o["cat_sum"][0, 1] == np.float64(1.25).view(np.uint64)
    # categories 12 and -1: the flag, and the walks are in no instance and no category
    o = MR.ranked_motifs_ref(eid3, cat, imp, np.array([[0, 2]], np.int32), 4)
    assert o["err"] == MR.TM_E_ARG and o["count"].tolist() == [2] and o["cat_n"][0].sum() == 2
    # a row outside [-1, rows): the flag, that position skipped
    o = MR.ranked_motifs_ref(eid3, cat, imp, np.array([[3, 1]], np.int32), 4)
    assert o["err"] == MR.TM_E_ARG and o["walk"][0].tolist() == [2, 3, -1, -1]


def test_mask_restatement():
    ranked = np.array([[(5, 6, 0), (7, 5, 8), (9, 9, 9)], [(0, 0, 0)] * 3], np.int32)
    count = np.array([3, 0], np.int32)
    node = np.array([[11, 12, 0, 14, 15, 16], [21, 22, 23, 24, 25, 26]], np.int32)
    eid = np.array([[5, 8, 6, 9, 0, -5], [5, 6, 7, 8, 9, 1]], np.int32)
    out = MR.motif_mask_ref(ranked, count, node, eid, [1, 2, 3])
    assert out[0].tolist() == [[11, 0, 0, 0, 0, 0], [0] * 6]       # edge 6 sits in the top triple, but its node is 0
    assert out[1].tolist() == [[11, 12, 0, 0, 0, 0], [0] * 6]
    assert out[2].tolist() == [[11, 12, 0, 14, 0, 0], [0] * 6]     # a row with no live walk keeps nothing
    # count below m: the padded triples past count add nothing
    out = MR.motif_mask_ref(ranked, np.array([1, 0], np.int32), node, eid, [3])
    assert out[0].tolist() == [[11, 0, 0, 0, 0, 0], [0] * 6]


def test_symbols_and_public_names():
    import tempme_amd
    from tempme_amd import _lib, fidelity, pipeline
    src = open(os.path.join(REPO, "include", "tempme.h")).read()
    for name in ("tm_ranked_motifs", "tm_motif_mask"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src)
        assert name in _lib.EXPORTS
        assert hasattr(tempme_amd.lib(), name)
    from tempme_amd.ranked_motifs import RankedMotifs, ranked_motifs
    assert tempme_amd.ranked_motifs is ranked_motifs and tempme_amd.RankedMotifs is RankedMotifs
    assert RankedMotifs._fields == ("eid", "score", "cat", "node", "ts", "walk", "mult", "count", "cat_n", "cat_max",
                                    "cat_sum")
    assert callable(fidelity.motif_masked_nodes) and callable(fidelity.motif_threshold_test)
    assert callable(pipeline.ExplainPipeline.ranked_motifs)


def test_ranked_motifs_refuses_cpu_tensors():
    import tempme_amd
    side = (torch.zeros(1, 2, 6, dtype=torch.int32), torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(1, 2, 3),
            torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tempme_amd.ranked_motifs(torch.rand(3, 1, 2), [side] * 3, 1, pairs=False)
