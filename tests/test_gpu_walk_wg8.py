"""walk_kernel's paired persistent zero-node instances run 8-wave workgroups, one per CU, with event_gcn's whole
split pack (EncW::g13, all six pair steps) resident in LDS (the pooled persistent ones too, below); every other
instance keeps 4-wave workgroups and half of the pack resident.  The pair steps are accumulated in one fixed order
whatever is resident, so `imp` of the paired 8-wave launch equals `imp` of the single-position instance (tm_debug_set(TM_DEBUG_WALK_SINGLE, 1): 4 waves, half
resident, three of the six pair steps streamed) as uint32, bit for bit:

* de = 32, zero node features, table mode, tests/test_gpu_lin_split.py's synthetic walks, the `plain` and `neg`
  weight sets of tests/test_gpu_gcn_split.py;
* workgroup tails at the smallest sizes the persistent form runs at (512 units and up): 520 units = 65 full
  workgroups; 513 = one live wave in the last workgroup (its other seven leave after the barrier); 519 = seven live
  waves; BIG's 514;
* tickets: BIG at M = 3 on one workgroup (all 8 stashes in one LDS, about 64 units per wave) and on 3 workgroups (24
  waves: no divisor of 514) -- nothing of one wave's stash or one unit's state may reach another;
* the form equality: BIG's persistent launch (8 waves) at M = 2 equals the three per-group split-form launches (4
  waves, half resident);
* sampled walks with null positions: tests/test_gpu_walk_mix.py's early-timeline pipeline run at M = 3 over 140
  events (525 units), one unit per wave and through tickets on 3 workgroups; the inputs are asserted to hold walks
  null at position 0, null at position 1 and wholly null slots.

The pooled persistent zero-node instances (tm_encoder_pool_fwd, single-position passes) take the same 8-wave form.
No 4-wave launch gives their output bit for bit (the pooled split form adds a slot's walks elsewhere, and differs from
the persistent form in the last bits in the 4-wave build too), so here the persistent launch one unit per wave is held
to the same launch through tickets on one and on three workgroups at M = 3 (7 passes per unit), and
tests/test_gpu_enhance.py holds both forms to the golden embeddings.
"""
import contextlib
import functools

import numpy as np
import pytest

from tests import test_gpu_walk_mix as mix
from tests.test_gpu_gcn_split import _launch
from tests.test_gpu_lin_split import BIG, N, _walks

pytestmark = pytest.mark.gpu

PERSISTENT = 512     # units from which a launch takes the persistent form (walk_split)


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


def _units(shape):
    return (shape[0] * shape[1] * N + 15) // 16


@functools.lru_cache(maxsize=None)
def _single(variant, shape, M):
    """imp of the single-position instance (the reference, computed once per input), as uint32."""
    with _debug(single=1):
        imp = _launch("de32", variant, _walks(shape[0], shape[1], M), True, M)
    assert np.isfinite(imp).all() and (imp > 0).all()
    imp = imp.view(np.uint32)
    imp.setflags(write=False)
    return imp


def _pair(variant, shape, M, blocks=0):
    with _debug(blocks=blocks):
        return _launch("de32", variant, _walks(shape[0], shape[1], M), True, M).view(np.uint32)


def _same(pair, single):
    bad = pair != single
    print("%d of %d walks differ" % (bad.sum(), bad.size))
    assert np.array_equal(pair, single)


# (groups, events per group), units, M
TAILS = [((1, 416), 520, 3), ((1, 410), 513, 1), ((1, 410), 513, 3), ((1, 415), 519, 3), (BIG, 514, 1), (BIG, 514, 3)]


@pytest.mark.parametrize("shape,units,M", TAILS)
@pytest.mark.parametrize("variant", ["plain", "neg"])
def test_workgroup_tails(variant, shape, units, M):
    """One unit per wave: full workgroups (520 = 65 x 8), one live wave in the last (513), seven (519), two (514)."""
    assert _units(shape) == units and units >= PERSISTENT
    assert 520 % 8 == 0 and 513 % 8 == 1 and 519 % 8 == 7
    _same(_pair(variant, shape, M), _single(variant, shape, M))


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("variant", ["plain", "neg"])
def test_tickets(variant, blocks):
    """514 units on one workgroup (8 waves, about 64 units each, all stashes in one LDS) and on three (24 waves, no
    divisor of 514), M = 3."""
    assert _units(BIG) == 514 and 514 % (8 * blocks)
    _same(_pair(variant, BIG, 3, blocks=blocks), _single(variant, BIG, 3))


@pytest.mark.parametrize("variant", ["plain", "neg"])
def test_persistent_launch_equals_split_launches(variant):
    """M = 2: 514 units in one persistent call against the same rows as three split-form calls, bit for bit."""
    G, B = BIG
    M = 2
    w = _walks(G, B, M)
    assert (B * N + 15) // 16 * M <= 3 * PERSISTENT and (B * N + 15) // 16 < PERSISTENT <= _units(BIG)
    imp = _launch("de32", variant, w, True, M)
    parts = np.concatenate([_launch("de32", variant, w, True, M, groups=slice(g, g + 1)) for g in range(G)])
    assert np.array_equal(parts.view(np.uint32), imp.view(np.uint32))


def _check_nulls(eid3):
    p = eid3 != 0
    assert (~p[..., 0] & p[..., 1] & p[..., 2]).sum() >= mix.FEW, "null position 0, position 1 valid"
    assert (p[..., 0] & ~p[..., 1] & p[..., 2]).sum() >= mix.FEW, "null position 1, position 0 valid"
    assert (~p[..., 2]).reshape(-1, mix.N, p.shape[2] // mix.N).all(-1).sum() >= mix.FEW, "whole null slots"
    assert p.all(-1).sum() >= mix.FEW, "complete walks"


E_NULL, B_NULL, M_NULL = 140, 70, 3


def _pipeline(blocks):
    g, late, _ = mix._graph("zeros")
    ev = mix.events(g, late, E_NULL) + (np.arange(E_NULL),)
    return mix._run("zeros", True, mix.W1_SCALE, M_NULL, ev, B_NULL, walk_blocks=blocks)


@functools.lru_cache(maxsize=None)
def _pipeline_single():
    with _debug(single=1):
        imp, walks = _pipeline(0)
    _check_nulls(walks[1])
    assert 3 * E_NULL * mix.N == walks[1].shape[0] * walks[1].shape[1] * walks[1].shape[2] // M_NULL
    assert (3 * E_NULL * mix.N + 15) // 16 == 525 >= PERSISTENT
    imp = imp.view(np.uint32)
    imp.setflags(write=False)
    return imp, walks


@pytest.mark.parametrize("blocks", [0, 3])
def test_null_positions(blocks):
    """Sampled walks of the timeline's start (saturated attention: a swapped column set changes the output), 525
    units: one per wave (the last workgroup has five live waves), and through tickets on 24 waves."""
    single, walks1 = _pipeline_single()
    pair, walks = _pipeline(blocks)
    for a, b in zip(walks, walks1):
        assert np.array_equal(a, b)
    _same(pair.view(np.uint32), single)


def _pooled(variant, shape, M, blocks=0, groups=None):
    """[G, B, 76] of one tm_encoder_pool_fwd call (walk weights by tm_walk_importance, per group) over the groups."""
    import torch
    from tests.test_gpu_gcn_split import _model
    ex = _model("de32", variant)[0]
    walks = _walks(shape[0], shape[1], M)
    if groups is not None:
        walks = tuple(a[groups] for a in walks)
    G, B, W = walks[1].shape[:3]
    dev = torch.device("cuda", 0)
    node6, eid3, ts3, cat, cut, cnt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in walks)
    with _debug(blocks=blocks):
        out = ex.enhance_groups(node6, eid3, ts3, cat, cut, cnt, G, B, W, M=M, etab=ex.dropin_edge_table())
        torch.cuda.synchronize()
    assert ex._node_zero
    out = out.cpu().numpy()
    assert out.shape == (G, B, 76) and np.isfinite(out).all() and (out[..., :64] > 0).any()
    return out.view(np.uint32)


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("variant", ["plain", "neg"])
def test_pooled_tickets(variant, blocks):
    """M = 3 (7 passes per unit): 514 units one per wave against the same launch on one workgroup and on three."""
    _same(_pooled(variant, BIG, 3, blocks=blocks), _pooled(variant, BIG, 3))
