"""tm_weight_lin_split (the host form of the pack job that builds EncW::ev3, lin_event's weights for the walk
kernel's bf16 MFMA form): tile-major, per (output tile t, K step s, part hi / mid / lo) one fragment.  A 32-wide
step's fragment is 64 lanes x 8 bf16, lane l = (group g = l >> 4, row o = l & 15), element j = W[16t + o][32s + 8g + j].
When r = kev mod 32 is in 1..16 the pack ends in one 16-deep step instead: fragments of 64 lanes x 4 bf16 in
v_mfma_f32_16x16x16_bf16's A-operand lane order, element j = W[16t + o][32s + 4g + j].  With r = 0 or r > 16 every
step is 32 wide.  Every element recomposes to the weight bit for bit; rows >= dn and columns >= kev are zero in all
three parts.  ns3 = ceil(kev / 32) and the pack's size are the ones the kernel indexes with: the fragment of
(t, s, part) starts at t * tile + s * 1536 + part * 512 bf16 (the 16-deep step: part * 256), tile = the sum of the
steps' three fragments, and the kernel takes the 16-deep form exactly when its count of 16-wide quads
ceil(kev / 16) is odd.

Widths (dn = 172, kev = de + 3 + dn): de = 32 (r = 15, the headline), 33 (r = 16: the step is full), 1 (r = 16 with 6
steps), 148 (r = 3: one lane group holds all the step's real features), 36 (r = 19) and 164 (r = 19 with 11 steps):
32-wide tail with padding, 49 and 17 (r = 0: no padding at all).  dn = 40 (a padded output tile) at kev = 79.
"""
import ctypes as C

import numpy as np
import pytest

CASES = [(172, 32), (172, 33), (172, 1), (172, 148), (172, 36), (172, 164), (172, 49), (172, 17)]


def layout(kev):
    """(32-wide steps, 16-deep steps, bf16 per tile) as documented at EncW::ev3."""
    ns3, r = (kev + 31) // 32, kev % 32
    tail = 1 <= r <= 16
    nf = ns3 - tail
    return nf, int(tail), nf * 1536 + tail * 768


def pack(w, kev):
    import tempme_amd
    lib = tempme_amd.lib()
    nout = w.shape[0]
    n = lib.tm_weight_lin_split(None, nout, kev, None)
    out = np.full(n, 0xFFFF, np.uint16)                        # every element must be written
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert lib.tm_weight_lin_split(w.ctypes.data_as(C.c_void_p), nout, kev, out.ctypes.data_as(C.c_void_p)) == n
    return out


def f32(bits16):
    return (bits16.astype(np.uint32) << 16).view(np.float32)


def weights(nout, kev, seed):
    rng = np.random.RandomState(seed)
    w = rng.uniform(-1, 1, (nout, kev)).astype(np.float32) / np.float32(np.sqrt(kev))
    w[rng.randint(0, nout, 50), rng.randint(0, kev, 50)] = 0.0
    w[0, kev - 1] = -0.0
    return w


def steps(p, nout, kev):
    """The pack as [(step s, its depth per lane d, array [nt, 3, 64, d])]."""
    nt = (nout + 15) // 16
    nf, tail, tile = layout(kev)
    assert p.size == nt * tile
    p = p.reshape(nt, tile)
    out = [(s, 8, p[:, s * 1536:(s + 1) * 1536].reshape(nt, 3, 64, 8)) for s in range(nf)]
    if tail:
        out.append((nf, 4, p[:, nf * 1536:].reshape(nt, 3, 64, 4)))
    return out


@pytest.mark.parametrize("dn,de", CASES + [(40, 36)])
def test_pack_has_the_documented_layout(dn, de):
    kev = de + 3 + dn
    r, ns3 = kev % 32, (kev + 31) // 32
    nf, tail, tile = layout(kev)
    # the kernel's view: NQE = ceil(kev / 16) quads, NS = (NQE + 1) / 2 steps, the last one 16 deep iff NQE is odd
    nqe = (kev + 15) // 16
    assert (nqe + 1) // 2 == ns3 == nf + tail and (nqe % 2 == 1) == bool(tail) == (1 <= r <= 16)
    w = weights(dn, kev, kev)
    st = steps(pack(w, kev), dn, kev)
    assert len(st) == ns3 and [d for _, d, _ in st] == [8] * nf + [4] * tail
    covered = 0
    for s, d, frag in st:
        nt = frag.shape[0]
        t, lane, j = np.meshgrid(np.arange(nt), np.arange(64), np.arange(d), indexing="ij")
        row, col = 16 * t + (lane & 15), 32 * s + d * (lane >> 4) + j
        inside = (row < dn) & (col < kev)
        covered += int(inside.sum())
        want = np.where(inside, w[np.minimum(row, dn - 1), np.minimum(col, kev - 1)], np.float32(0)).astype(np.float32)
        hi, mid, lo = (f32(frag[:, k]) for k in range(3))
        got = (hi + mid).astype(np.float32) + lo
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "step %d" % s
        for k in range(3):                                     # outside W all three parts are +0
            assert not frag[:, k][~inside].any()
        assert (np.abs(mid) <= np.abs(hi) * 2.0 ** -8).all() and (np.abs(lo) <= np.abs(hi) * 2.0 ** -16).all()
    assert covered == dn * kev                                 # every weight lands exactly once


def test_the_16_deep_step_of_the_headline_width():
    """kev = 207: step 6 holds k = 192..207, 15 real features and one padded lane element (group 3, j = 3)."""
    w = np.ones((172, 207), np.float32)
    st = steps(pack(w, 207), 172, 207)
    assert len(st) == 7 and st[6][1] == 4
    frag = st[6][2]
    g = np.arange(64) >> 4
    assert (frag[:10, 0] == 0x3F80).sum() == 10 * (64 * 4 - 16)            # 16 rows x the one padded column
    assert not frag[:, 0, g == 3, 3].any() and (frag[:10, 0, g == 3, :3] == 0x3F80).all()
    assert not frag[:, 1:].any()
    assert (frag[10, 0, (np.arange(64) & 15) < 12, :3] == 0x3F80).all()     # rows 160..171
    assert not frag[10, 0, (np.arange(64) & 15) >= 12].any()               # rows 172..175: padding


def test_matches_split3_element_for_element():
    import tempme_amd
    rng = np.random.RandomState(9)
    w = (rng.standard_normal((172, 207)) * 10.0 ** rng.uniform(-6, 4, (172, 207))).astype(np.float32)
    parts = [np.zeros(w.shape, np.uint16) for _ in range(3)]
    q = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tempme_amd.lib().tm_weight_split3(q(w), w.size, q(parts[0]), q(parts[1]), q(parts[2]))
    for s, d, frag in steps(pack(w, 207), 172, 207):
        for t in range(11):
            rows = np.arange(16 * t, min(16 * t + 16, 172))
            for g in range(4):
                for j in range(d):
                    c = 32 * s + d * g + j
                    if c >= 207:
                        continue
                    for k in range(3):
                        assert np.array_equal(frag[t, k, 16 * g + np.arange(len(rows)), j], parts[k][rows, c])
