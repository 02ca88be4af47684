"""tm_weight_split3 (the host function lin_event's bf16 split pack is built with): every fp32 value is the sum
of three bf16 parts, hi + mid + lo, added in that order in fp32, bit for bit.

What happens to a low part that underflows: bf16 has fp32's exponent range but only 7 mantissa bits, so its
smallest denormal step is 2^-133 where fp32's is 2^-149.  A residual part is at most 2^-8 (mid) or 2^-16 (lo) of
the value, so for |v| < 2^-110 a residual can need bits below 2^-133; it is then rounded to the nearest multiple
of 2^-133 (mostly to zero), and the sum is within 2^-134 of v instead of equal to it.  From 2^-110 up the split
is exact.  lin_event's weights are O(1/sqrt(207)); the walk kernel never sees the underflow range in practice.
"""
import ctypes as C

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
TINY_EXACT = np.float32(2.0 ** -110)     # the split is exact from here up
BF16_STEP = 2.0 ** -133                  # bf16's smallest denormal


def split(v):
    import tempme_amd
    v = np.ascontiguousarray(v, dtype=np.float32)
    parts = [np.zeros(v.shape, np.uint16) for _ in range(3)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tempme_amd.lib().tm_weight_split3(p(v), v.size, p(parts[0]), p(parts[1]), p(parts[2]))
    return parts


def f32(bits16):
    return (bits16.astype(np.uint32) << 16).view(np.float32)


def recompose(parts):
    h, m, lo = (f32(x) for x in parts)
    with np.errstate(over="ignore", invalid="ignore"):
        return (h + m).astype(np.float32) + lo


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_exact(v):
    v = np.asarray(v, np.float32)
    parts = split(v)
    for x in parts:
        assert np.isfinite(f32(x)).all(), "a part of a finite value is not finite"
    assert np.array_equal(bits(recompose(parts)), bits(v))
    return parts


def test_random_normals():
    rng = np.random.RandomState(0)
    check_exact(rng.standard_normal(200000))
    check_exact(rng.standard_normal(20000) * np.float32(1e20))
    check_exact(rng.standard_normal(20000) * np.float32(1e-20))


def test_lin_event_scaled_weights():
    rng = np.random.RandomState(1)
    s = 1.0 / np.sqrt(207.0)
    h, m, lo = check_exact(rng.uniform(-s, s, 172 * 207))
    # the parts shrink by 2^-8 each (round to nearest: the residual is at most half a bf16 step)
    hf, mf, lf = np.abs(f32(h)), np.abs(f32(m)), np.abs(f32(lo))
    assert (mf <= hf * 2.0 ** -8).all() and (lf <= hf * 2.0 ** -16).all()


def test_signed_zero():
    # a zero part carries the value's sign: (-0) + (-0) + (-0) = -0, where (-0) + (+0) would be +0
    for x in check_exact([0.0, -0.0]):
        assert x.tolist() == [0x0000, 0x8000]


def test_high_part_is_round_to_nearest_even():
    v = np.array([1.0, 1.00390625, 1.01171875, 3.1415927, -2.7182817], np.float32)   # 1 + 2^-8: a tie, to even
    u = bits(v)
    want = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    assert np.array_equal(split(v)[0], want)


def test_small_values_and_denormals():
    rng = np.random.RandomState(2)
    # exact down to 2^-110
    check_exact(TINY_EXACT * (1 + rng.uniform(0, 1, 5000)).astype(np.float32))
    check_exact(-TINY_EXACT * (1 + rng.uniform(0, 1, 5000)).astype(np.float32))
    # below: +-1e-38 (normal, next to the smallest normal 1.18e-38) and fp32 denormals; a low part that
    # underflows bf16's denormal step is rounded to it: finite parts, the sum within half a step of the value
    den = (rng.randint(1, 1 << 23, 5000).astype(np.uint32)).view(np.float32)
    v = np.concatenate([np.array([1e-38, -1e-38, 1.17549435e-38, 1e-45, -1e-45], np.float32), den, -den,
                        TINY_EXACT * rng.uniform(2.0 ** -16, 1, 5000).astype(np.float32)]).astype(np.float32)
    parts = split(v)
    for x in parts:
        assert np.isfinite(f32(x)).all()
    h, m, lo = (f32(x).astype(np.float64) for x in parts)
    assert (np.abs(h + m + lo - v.astype(np.float64)) <= BF16_STEP / 2).all()
    # every part is a multiple of bf16's step, so an fp32 denormal below it loses its low bits
    assert np.array_equal(np.mod(np.abs(lo), BF16_STEP), np.zeros_like(lo))
    # and the high part alone is still the value rounded to bf16
    assert (np.abs(h - v.astype(np.float64)) <= np.maximum(np.abs(v.astype(np.float64)) * 2.0 ** -8, BF16_STEP / 2)).all()


def test_largest_values_never_reach_inf():
    # 0x7f7f8000 is the smallest value whose bf16 round-to-nearest would be the infinity pattern 0x7f80
    edge = np.array([0x7F7F8000, 0x7F7F7FFF, 0x7F7F8001, 0x7F7FFFFF], np.uint32).view(np.float32)
    v = np.concatenate([edge, -edge, [FLT_MAX, -FLT_MAX]]).astype(np.float32)
    h, m, lo = check_exact(v)
    assert ((h & 0x7FFF) <= 0x7F7F).all(), "high part above the largest finite bf16"
    assert (h[[0, 2, 3]] == 0x7F7F).all() and h[1] == 0x7F7F      # truncated, not rounded up
    rng = np.random.RandomState(3)
    big = (rng.randint(0x7F000000, 0x7F7FFFFF, 20000).astype(np.uint32)).view(np.float32)
    check_exact(np.concatenate([big, -big]))


def test_no_part_is_ever_inf_for_finite_input():
    rng = np.random.RandomState(4)
    u = rng.randint(0, 1 << 32, 400000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7F800000) != 0x7F800000]                          # every finite bit pattern class
    for x in split(u.view(np.float32)):
        assert ((x & 0x7F80) != 0x7F80).all()


def test_non_finite_goes_through_as_high_part():
    v = np.array([np.inf, -np.inf, np.nan], np.float32)
    h, m, lo = split(v)
    assert h[0] == 0x7F80 and h[1] == 0xFF80 and np.isnan(f32(h[2:3]))[0]
    assert not m.any() and not lo.any()
