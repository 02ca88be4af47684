"""Ranked motif instances as tm_ranked_motifs and tm_motif_mask define them (include/tempme.h,
csrc/ranked_motifs.hip), restated in numpy with plain loops and dictionaries, and the seeded inputs the tests share.

A group's entries are the walks of its rows in group_rows order, entry p * W + w; an entry is live iff the first edge
id of its walk is positive and its category is one of the 12; a motif instance of the group is a distinct ordered
triple of edge ids among its live entries.
"""
import math

import numpy as np

from ranked_edges_ref import QNAN_BITS, TM_E_ARG, beats, canonical_bits, pair_groups  # noqa: F401

N_CATS = 12
MODES = ("instance", "walk", "beta")


def triple_key(t):
    """the triple's ids as unsigned 32-bit values, for the lexicographic order"""
    return tuple(int(x) & 0xFFFFFFFF for x in t)


def order_key(score, t):
    """score descending with NaN last, equal scores (so -0 and +0 too) by the triple ascending"""
    if math.isnan(score):
        return (1, 0.0, triple_key(t))
    return (0, -float(score), triple_key(t))


def ranked_motifs_ref(eid3, cat, imp, group_rows, k):
    """eid3 int32 [rows, W, 3], cat int32 [rows, W], imp float32 [rows, W], group_rows int32 [G, R] -> dict of
    eid int32 [G, k, 3], score (bits, uint32) / walk / mult / cat int32 [G, k], count int32 [G], cat_n int32 [G, 12],
    cat_max (bits, uint32) [G, 12], cat_sum (bits, uint64) [G, 12], err."""
    rows, W = imp.shape
    G, R = group_rows.shape
    o = dict(eid=np.zeros((G, k, 3), np.int32), score=np.zeros((G, k), np.uint32),
             walk=np.full((G, k), -1, np.int32), mult=np.zeros((G, k), np.int32), cat=np.full((G, k), -1, np.int32),
             count=np.zeros(G, np.int32), cat_n=np.zeros((G, N_CATS), np.int32),
             cat_max=np.zeros((G, N_CATS), np.uint32), cat_sum=np.zeros((G, N_CATS), np.uint64))
    err = 0
    for g in range(G):
        inst = {}
        c_n, c_max, c_sum = [0] * N_CATS, [math.nan] * N_CATS, [np.float64(0.0)] * N_CATS
        for p in range(R):
            row = int(group_rows[g, p])
            if row == -1:
                continue
            if row < -1 or row >= rows:
                err = TM_E_ARG
                continue
            for w in range(W):
                c = int(cat[row, w])
                if c < 0 or c >= N_CATS:
                    err = TM_E_ARG
                    continue
                if eid3[row, w, 0] <= 0:
                    continue
                f, idx = float(imp[row, w]), p * W + w
                c_n[c] += 1
                if beats(f, c_max[c]):
                    c_max[c] = f
                if not math.isnan(f):
                    c_sum[c] = c_sum[c] + np.float64(imp[row, w])        # one accumulator, ascending entry order
                t = tuple(int(x) for x in eid3[row, w])
                if t not in inst:
                    inst[t] = [f, idx, 1, c]                             # entries come in ascending index order
                    continue
                cur = inst[t]
                cur[2] += 1
                if beats(f, cur[0]):
                    cur[0] = f
        ranked = sorted(inst.items(), key=lambda it: order_key(it[1][0], it[0]))
        o["count"][g] = len(ranked)
        for j, (t, (f, idx, m, c)) in enumerate(ranked[:k]):
            o["eid"][g, j], o["score"][g, j], o["walk"][g, j], o["mult"][g, j], o["cat"][g, j] = \
                t, canonical_bits(f), idx, m, c
        for c in range(N_CATS):
            o["cat_n"][g, c] = c_n[c]
            o["cat_max"][g, c] = canonical_bits(c_max[c]) if c_n[c] else 0
            o["cat_sum"][g, c] = np.float64(c_sum[c]).view(np.uint64)
    o["err"] = err
    return o


def motif_mask_ref(ranked_eid, count, node, eid, m_list):
    """ranked_eid int32 [rows, k, 3], count int32 [rows], node / eid int32 [rows, ne] -> int32 [Gm, rows, ne]: a slot
    keeps its node id iff it is nonzero and its edge id is positive and one of the nonzero ids in the first
    min(m, count, k) triples of its row."""
    rows, k, _ = ranked_eid.shape
    out = np.zeros((len(m_list),) + node.shape, np.int32)
    for gi, m in enumerate(m_list):
        for r in range(rows):
            top = min(int(m), int(count[r]), k)
            ids = {int(x) for t in ranked_eid[r, :top] for x in t if x != 0}
            for s in range(node.shape[1]):
                if node[r, s] != 0 and eid[r, s] > 0 and int(eid[r, s]) in ids:
                    out[gi, r, s] = node[r, s]
    return out


def make_walks(rng, rows, W, eid_hi, mode="instance", dead=0.15, short=0.2):
    """Seeded walks: edge ids in 1..eid_hi (a small range: duplicate triples and ties are frequent), about ``dead`` of
    the walks padding (all zero), about ``short`` of the rest with a zero third id; a category per triple; scores
    round(u * 8) / 8 drawn per triple ("instance": one score wherever the instance sits) or per walk ("walk": ties and
    several scores per instance), or unquantised per walk ("beta").  -> eid3 [rows, W, 3], cat, imp [rows, W]."""
    eid3 = rng.integers(1, eid_hi + 1, (rows, W, 3)).astype(np.int32)
    eid3[rng.uniform(size=(rows, W)) < short, 2] = 0
    eid3[rng.uniform(size=(rows, W)) < dead] = 0
    h = (eid3[..., 0].astype(np.int64) * 7919 + eid3[..., 1] * 104729 + eid3[..., 2] * 1299709)
    cat = (h % N_CATS).astype(np.int32)
    cat[eid3[..., 0] == 0] = 0
    if mode == "beta":
        imp = rng.uniform(size=(rows, W)).astype(np.float32)
    elif mode == "walk":
        imp = (np.round(rng.uniform(size=(rows, W)) * 8) / 8).astype(np.float32)
    else:
        table = (np.round(rng.uniform(size=4099) * 8) / 8).astype(np.float32)
        imp = table[h % 4099]
    return eid3, cat, imp


def walks_from_subgraph(rng, sub_eid, W):
    """Seeded walks whose edge ids are drawn from each row's own subgraph edge ids (sub_eid int [rows, ne]; a row
    without a positive id gets padding walks only): what motif_threshold_test needs around a base-model case that
    carries subgraphs but no walks.  With W >= 4 the last two walks repeat the first two.
    -> node6 [rows, W, 6] int32, eid3, ts3 float32 [rows, W, 3], cat, imp."""
    rows = sub_eid.shape[0]
    eid3 = np.zeros((rows, W, 3), np.int32)
    for r in range(rows):
        pool = np.unique(sub_eid[r][sub_eid[r] > 0]).astype(np.int32)
        if pool.size == 0:
            continue
        pick = pool[:max(1, min(pool.size, 6))]                          # few ids: instances repeat within a row
        eid3[r] = pick[rng.integers(0, pick.size, (W, 3))]
        eid3[r, rng.uniform(size=W) < 0.2, 2] = 0
        eid3[r, rng.uniform(size=W) < 0.15] = 0
        if W >= 4:
            eid3[r, W - 2:] = eid3[r, :2]                                # at most W - 2 distinct instances in a row
    live = eid3[..., 0] > 0
    cat = np.where(live, rng.integers(0, N_CATS, (rows, W)), 0).astype(np.int32)
    node6 = np.where(live[..., None], rng.integers(1, 50, (rows, W, 6)), 0).astype(np.int32)
    ts3 = np.where(live[..., None], rng.uniform(0, 1e6, (rows, W, 3)), 0).astype(np.float32)
    imp = (np.round(rng.uniform(size=(rows, W)) * 8) / 8).astype(np.float32)
    return node6, eid3, ts3, cat, imp


def rows_each(rows):
    return np.arange(rows, dtype=np.int32).reshape(rows, 1)
