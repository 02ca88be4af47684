"""Ranked explanation edges as tm_ranked_edges defines them (include/tempme.h, csrc/ranked_edges.hip), restated in
numpy with plain loops and dictionaries, and the seeded inputs the tests share.

A group's entries are the slots of its rows in group_rows order, entry p * ne + s; an entry is live iff its node
record is nonzero and its edge id positive; an edge of the group is a distinct edge id among its live entries.
"""
import math

import numpy as np

TM_E_ARG = -4
QNAN_BITS = 0x7FC00000


def beats(f, cur):
    """f replaces cur as the maximum: fp32 value comparison, a NaN loses to every number (-0 == +0: no change)."""
    if math.isnan(f):
        return False
    if math.isnan(cur):
        return True
    return f > cur


def canonical_bits(f):
    """uint32 bits of a result score: the value's own, a zero as +0.0, a NaN as the quiet NaN 0x7FC00000."""
    if math.isnan(f):
        return QNAN_BITS
    if f == 0.0:
        return 0
    return int(np.float32(f).view(np.uint32))


def order_key(score, eid):
    """score descending with NaN last, equal scores (so -0 and +0 too) by edge id ascending"""
    if math.isnan(score):
        return (1, 0.0, eid)
    return (0, -float(score), eid)


def ranked_edges_ref(imp, node, eid, group_rows, k):
    """imp float32 / node, eid int32 [rows, ne] ([hop-1 | hop-2] side by side); group_rows int32 [G, R] ->
    (eid int32 [G, k], score bits uint32 [G, k], slot int32 [G, k], mult int32 [G, k], count int32 [G], err)."""
    rows, ne = imp.shape
    G, R = group_rows.shape
    o_eid, o_bits = np.zeros((G, k), np.int32), np.zeros((G, k), np.uint32)
    o_slot, o_mult = np.full((G, k), -1, np.int32), np.zeros((G, k), np.int32)
    o_count, err = np.zeros(G, np.int32), 0
    for g in range(G):
        edges = {}
        for p in range(R):
            row = int(group_rows[g, p])
            if row == -1:
                continue
            if row < -1 or row >= rows:
                err = TM_E_ARG
                continue
            for s in range(ne):
                e = int(eid[row, s])
                if node[row, s] == 0 or e <= 0:
                    continue
                f, idx = float(imp[row, s]), p * ne + s
                if e not in edges:
                    edges[e] = [f, idx, 1]
                    continue
                cur = edges[e]
                cur[2] += 1
                if idx < cur[1]:
                    cur[1] = idx
                if beats(f, cur[0]):
                    cur[0] = f
        ranked = sorted(edges.items(), key=lambda it: order_key(it[1][0], it[0]))
        o_count[g] = len(ranked)
        for j, (e, (f, idx, m)) in enumerate(ranked[:k]):
            o_eid[g, j], o_bits[g, j], o_slot[g, j], o_mult[g, j] = e, canonical_bits(f), idx, m
    return o_eid, o_bits, o_slot, o_mult, o_count, err


MODES = ("edge", "slot", "beta")


def make_records(rng, rows, n, hops, eid_hi, mode="edge", dead=0.2):
    """Seeded records [rows, ne]: edge ids in 1..eid_hi (a small range: duplicates are frequent), about ``dead`` of
    the node ids 0, scores round(u * 8) / 8 so that different edges tie often: drawn per edge id ("edge": an edge
    carries one score everywhere, as training=False gives) or per slot ("slot": ties and several scores per edge);
    "beta": unquantised per slot (one edge, several scores, as the Beta draw gives)."""
    ne = n + n * n if hops == 2 else n
    eid = rng.integers(1, eid_hi + 1, (rows, ne)).astype(np.int32)
    node = rng.integers(1, 50, (rows, ne)).astype(np.int32)
    node[rng.uniform(size=(rows, ne)) < dead] = 0
    if mode == "beta":
        imp = rng.uniform(size=(rows, ne)).astype(np.float32)
    elif mode == "slot":
        imp = (np.round(rng.uniform(size=(rows, ne)) * 8) / 8).astype(np.float32)
    else:
        per_edge = (np.round(rng.uniform(size=eid_hi + 1) * 8) / 8).astype(np.float32)
        imp = per_edge[eid]
    return imp, node, eid


def pair_groups(B):
    """group_rows of ranked_edges(pairs=True): [2 B, 2], (src_i, tgt_i) for every i, then (src_i, bgd_i)."""
    i = np.arange(B, dtype=np.int32)
    return np.concatenate([np.stack([i, i + B], 1), np.stack([i, i + 2 * B], 1)]).astype(np.int32)
