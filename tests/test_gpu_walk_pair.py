"""walk_kernel's pair pass (zero-node table-mode instances): a walk's positions 0 and 1 run in one pass as two
column sets through one stream of lin_event's weight fragments (encode_pair), a unit is the slot pass and one pass
per walk.  Per column the arithmetic is the single-position pass's -- the same products in the same order from the
same table row -- so `imp` of the pair pass equals `imp` of the single-position pass (the instances
tm_debug_set(TM_DEBUG_WALK_SINGLE, 1) selects) as uint32, bit for bit:

* de = 32, zero node features, table mode, tests/test_gpu_lin_split.py's synthetic walks, the `plain` and `neg`
  weight sets of tests/test_gpu_gcn_split.py;
* split form: SMALL (1 x 7 events = 8.75 units, the last one partial), M = 1, 2, 3 (2 passes per wave);
* persistent form, one unit per wave: BIG (3 x 137 events = 514 units), M = 1 and 3 (2 and 4 passes per unit);
* persistent form through tickets: BIG with the grid capped at 8 workgroups (about 16 units per wave), M = 3 --
  nothing of one unit (a column set, a table row, the next pass's scalars) may reach the next;
* null patterns on walks the pipeline itself sampled from tests/test_gpu_walk_mix.py's early-timeline events: the
  inputs are asserted to hold walks null at position 0 with position 1 valid, the reverse, and wholly null slots
  (that module's docstring: positions 0 and 1 are never both null under a valid slot);
* a paired instance's persistent launch equals the per-group split launches (the form equality, here at M = 2).
"""
import contextlib

import numpy as np
import pytest

from tests import test_gpu_walk_mix as mix
from tests.test_gpu_gcn_split import _launch
from tests.test_gpu_lin_split import BIG, N, SMALL, _walks

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _debug(**opts):
    """tm_debug_set options (single=, blocks=) for the launches inside, reset afterwards."""
    from tempme_amd import _lib as L
    ids = {"single": L.TM_DEBUG_WALK_SINGLE, "blocks": L.TM_DEBUG_WALK_BLOCKS}
    try:
        for k, v in opts.items():
            L.check(L.lib().tm_debug_set(ids[k], int(v)), "tm_debug_set")
        yield
    finally:
        for k in opts:
            L.check(L.lib().tm_debug_set(ids[k], 0), "tm_debug_set")


def _both(variant, shape, M, blocks=0):
    """imp of the pair pass and of the single-position pass on the same walks, as uint32."""
    G, B = shape
    w = _walks(G, B, M)
    with _debug(blocks=blocks):
        pair = _launch("de32", variant, w, True, M)
        with _debug(single=1):
            single = _launch("de32", variant, w, True, M)
    assert np.isfinite(pair).all() and (pair > 0).all()
    return pair.view(np.uint32), single.view(np.uint32)


def _same(pair, single):
    bad = pair != single
    print("%d of %d walks differ" % (bad.sum(), bad.size))
    assert np.array_equal(pair, single)


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("variant", ["plain", "neg"])
def test_split_form(variant, M):
    """8.75 units, one wave per (unit, walk): the slot pass and one pair pass."""
    assert (SMALL[0] * SMALL[1] * N + 15) // 16 == 9 and (SMALL[0] * SMALL[1] * N) % 16
    _same(*_both(variant, SMALL, M))


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("variant", ["plain", "neg"])
def test_persistent_form_one_unit_per_wave(variant, M):
    """514 units on 514 waves: 1 + M passes."""
    assert (BIG[0] * BIG[1] * N + 15) // 16 == 514
    _same(*_both(variant, BIG, M))


@pytest.mark.parametrize("variant", ["plain", "neg"])
def test_persistent_form_through_tickets(variant):
    """514 units on 32 waves, about 16 units each: the pair pass's inputs are requested a whole pass ahead, the
    next unit's slot-pass inputs in the last pair pass."""
    _same(*_both(variant, BIG, 3, blocks=8))


@pytest.mark.parametrize("variant", ["plain", "neg"])
def test_persistent_launch_equals_split_launches(variant):
    """M = 2, pair pass: 514 units in one call against the same rows as three split-form calls, bit for bit."""
    G, B = BIG
    M = 2
    w = _walks(G, B, M)
    assert (B * N + 15) // 16 * M <= 3 * 512 and (B * N + 15) // 16 < 512 <= (G * B * N + 15) // 16
    imp = _launch("de32", variant, w, True, M)
    parts = np.concatenate([_launch("de32", variant, w, True, M, groups=slice(g, g + 1)) for g in range(G)])
    assert np.array_equal(parts.view(np.uint32), imp.view(np.uint32))


def _check_nulls(eid3):
    p = eid3 != 0
    assert (~p[..., 0] & p[..., 1] & p[..., 2]).sum() >= mix.FEW, "null position 0, position 1 valid"
    assert (p[..., 0] & ~p[..., 1] & p[..., 2]).sum() >= mix.FEW, "null position 1, position 0 valid"
    assert (~p[..., 2]).reshape(-1, mix.N, p.shape[2] // mix.N).all(-1).sum() >= mix.FEW, "whole null slots"
    assert p.all(-1).sum() >= mix.FEW, "complete walks"


def _pipeline_both(M, E, B, blocks=0):
    g, late, _ = mix._graph("zeros")
    ev = mix.events(g, late, E) + (np.arange(E),)
    pair, walks = mix._run("zeros", True, mix.W1_SCALE, M, ev, B, walk_blocks=blocks)
    with _debug(single=1):
        single, walks1 = mix._run("zeros", True, mix.W1_SCALE, M, ev, B, walk_blocks=blocks)
    for a, b in zip(walks, walks1):
        assert np.array_equal(a, b)
    _check_nulls(walks[1])
    return pair.view(np.uint32), single.view(np.uint32)


@pytest.mark.parametrize("M", [1, 3])
def test_null_positions_split_form(M):
    """Sampled walks of the timeline's start (saturated attention: a swapped column set changes the output)."""
    _same(*_pipeline_both(M, 7, 7))


def test_null_positions_through_tickets():
    """The same over 140 events (525 units) on 32 waves, M = 3."""
    _same(*_pipeline_both(3, 140, 70, blocks=8))
