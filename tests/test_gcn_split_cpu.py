"""tm_weight_gcn_split (the host form of the pack job that builds EncW::g13, event_gcn's first layer for the
zero-node walk kernel's bf16 MFMA form): per (output tile t, pair step u, part hi / mid / lo) one fragment of
64 lanes x 8 bf16.  Lane l = (group g = l >> 4, row o = l & 15), element j holds W[16t + o][f(u, g, j)] with
f(u, g, j) = 16 (2u + (j >> 2)) + 4g + (j & 3): elements 0..3 come from input tile 2u, 4..7 from tile 2u + 1, each
in the lane order lin_event's D tiles have.  Every element recomposes to the weight bit for bit; columns >= dn
(the padding of the last tile, and the empty second half of the last step of an odd tile count) and rows >= nout
are zero in all three parts.

Sizes: dn = 172 (11 tiles: the last step pairs tile 10 with nothing, and tile 10 has 4 padded columns), 160 (a
multiple of 32: 10 full tiles, no padding at all), 180 (12 tiles, an even count, 12 padded columns) and 20 (two
tiles, one step); nout = 64 (the kernel's) and 40 (a padded output tile).
"""
import ctypes as C

import numpy as np
import pytest


def f(u, g, j):
    return 16 * (2 * u + (j >> 2)) + 4 * g + (j & 3)


def pack(w):
    import tempme_amd
    nout, dn = w.shape
    nt, ns = (nout + 15) // 16, ((dn + 15) // 16 + 1) // 2
    out = np.full((nt, ns, 3, 64, 8), 0xFFFF, np.uint16)        # every element must be written
    w = np.ascontiguousarray(w, dtype=np.float32)
    tempme_amd.lib().tm_weight_gcn_split(w.ctypes.data_as(C.c_void_p), nout, dn, out.ctypes.data_as(C.c_void_p))
    return out


def f32(bits16):
    return (bits16.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("nout,dn", [(64, 172), (64, 160), (64, 180), (64, 20), (40, 172)])
def test_pack_recomposes_to_the_permuted_weights(nout, dn):
    rng = np.random.RandomState(dn + nout)
    w = rng.uniform(-1, 1, (nout, dn)).astype(np.float32) / np.float32(np.sqrt(dn))
    w[rng.randint(0, nout, 50), rng.randint(0, dn, 50)] = 0.0
    w[0, dn - 1] = -0.0
    p = pack(w)
    nt, ns = p.shape[:2]
    assert ns == ((dn + 15) // 16 + 1) // 2 and nt == (nout + 15) // 16
    # the expected matrix: [t, u, lane, j] -> W[16t + (lane & 15)][f(u, lane >> 4, j)], zero outside W
    t, u, lane, j = np.meshgrid(np.arange(nt), np.arange(ns), np.arange(64), np.arange(8), indexing="ij")
    row, col = 16 * t + (lane & 15), f(u, lane >> 4, j)
    inside = (row < nout) & (col < dn)
    want = np.where(inside, w[np.minimum(row, nout - 1), np.minimum(col, dn - 1)], np.float32(0.0)).astype(np.float32)
    hi, mid, lo = (f32(p[:, :, k]) for k in range(3))
    got = (hi + mid).astype(np.float32) + lo
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # outside W all three parts are +0, not merely a sum of zero
    for k in range(3):
        assert not p[:, :, k][~inside].any()
    # every column of W lands exactly once per output row
    assert inside.sum() == nout * dn
    # the parts are a split3: each at most half a bf16 step of the one before
    assert (np.abs(mid) <= np.abs(hi) * 2.0 ** -8).all() and (np.abs(lo) <= np.abs(hi) * 2.0 ** -16).all()


def test_empty_half_of_the_last_step_is_zero():
    w = np.ones((64, 172), np.float32)
    p = pack(w)
    assert p.shape[:2] == (4, 6)
    assert not p[:, 5, :, :, 4:].any()                      # tile 11 does not exist
    g = np.arange(64) >> 4
    assert (p[:, 5, 0, g < 3, :4] == 0x3F80).all()           # tile 10, columns 160..171
    assert not p[:, 5, :, g == 3, :4].any()                  # columns 172..175: padding
    assert (p[:, :5, 0] == 0x3F80).all() and not p[:, :5, 1:].any()


def test_matches_split3_element_for_element():
    import tempme_amd
    rng = np.random.RandomState(9)
    w = (rng.standard_normal((64, 172)) * 10.0 ** rng.uniform(-6, 4, (64, 172))).astype(np.float32)
    p = pack(w)
    parts = [np.zeros(w.shape, np.uint16) for _ in range(3)]
    q = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tempme_amd.lib().tm_weight_split3(q(w), w.size, q(parts[0]), q(parts[1]), q(parts[2]))
    for t in range(4):
        for u in range(6):
            for g in range(4):
                for j in range(8):
                    c = f(u, g, j)
                    if c >= 172:
                        continue
                    lanes = 16 * g + np.arange(16)
                    for k in range(3):
                        assert np.array_equal(p[t, u, k, lanes, j], parts[k][16 * t:16 * t + 16, c])
