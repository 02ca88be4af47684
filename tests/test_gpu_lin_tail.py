"""GPU: lin_event's last K step at every remainder r = kev mod 32 (dn = 172, kev = de + 175, so r = (de + 15) mod 32).
With 1 <= r <= 16 the split pack EncW::ev3 ends in one 16-deep step: each lane generates 4 features for it, reads
8-byte weight fragments and multiplies on v_mfma_f32_16x16x16_bf16; with r = 0 or r > 16 every step is 32 wide
(tests/test_lin_tail_cpu.py: the pack).  Widths, one per class that the instance table supports
(edge_width_inputs.WIDTHS):

  r = 15   de = 32    nqe 13, table        the headline width: one padded lane element in the 16-deep step
  r = 16   de = 33    nqe 13, table        the 16-deep step full
  r = 16   de = 1     nqe 11, plain        the same with 6 K steps, no table
  r = 3    de = 148   nqe 21, streamed     streamed edge features, the 16-deep step nearly empty
  r = 19   de = 36    nqe 14, table        32-wide last step with padding
  r = 0    de = 49    nqe 14, plain        no padding at all

* every width and mode in the split form (140 slots = 8.75 units, M = 1 and 3) against oracle/encoder_ref.forward in
  float64 at the contract rtol 1e-5, atol 1e-6 (test_gpu_edge_width.py's): zero-node table mode (the headline
  family), two-branch table mode, plain mode, streamed edge features;
* the 16-deep-tail table widths 32 and 33, zero node features, `imp` as uint32: the pair pass against the
  single-position pass (TM_DEBUG_WALK_SINGLE) in the split form and at 513 and 514 units persistent (one and two
  live waves in the last workgroup), through tickets on one and on three workgroups, and the persistent launch
  against the groups' split launches at M = 2;
* the other families with a 16-deep last step -- de = 1 (plain), 148 (streamed), 33 with non-zero node features
  (two-branch table mode), all single-position passes -- as uint32 at 514 units and M = 2: the persistent launch
  against the groups' split launches, and tickets on one and on three workgroups against one unit per wave;
* the pooled forward at 514 units, one unit per wave against tickets on one and three workgroups;
* null patterns: the synthetic walks hold walks null at position 0, at position 1 and whole null slots (asserted
  here), whose dt = 0 features meet the 16-deep step's padded element; the pipeline's own early-timeline walks
  (test_gpu_walk_pair.py's check of the inputs) through tickets on one workgroup.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import edge_width_inputs as EW
from edge_width_inputs import ATOL, BIG, N, RTOL, SMALL, WIDTHS, _walks

pytestmark = pytest.mark.gpu

B513 = (2, 205)         # 8200 slots = 512.5 units: 513, one live wave in the last 8-wave workgroup (BIG: 514, two)
FEW = 5                 # walks of each null pattern that every input must hold at least
TAIL_TABLE = (32, 33)   # 16-deep last step, per-edge-id table: the pair pass's widths
# de, node features, table mode
CASES = [(32, "zeros", True), (33, "zeros", True), (33, "uniform", True), (33, "uniform", False), (1, "uniform", False),
         (148, "uniform", False), (36, "zeros", True), (49, "uniform", False)]


def r_of(de):
    return (de + 3 + EW.DN) % 32


def test_widths_reach_every_remainder_class():
    assert [r_of(de) for de in (32, 33, 1, 148, 36, 49)] == [15, 16, 16, 3, 19, 0]
    for de, _, table in CASES:
        nqe = (de + 3 + EW.DN + 15) // 16
        assert WIDTHS[de]["fused"] and WIDTHS[de]["nqe"] == nqe and (nqe % 2 == 1) == (1 <= r_of(de) <= 16)
        assert WIDTHS[de]["table"] or not table
    assert WIDTHS[148]["load_ef"] == "streamed" and not WIDTHS[1]["table"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


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


def _launch(dev, de, node_feat, walks, table, M, groups=None, **debug):
    """imp [G, B, W] of one tm_encoder_fwd_tab call over the groups (default: all of them)."""
    ex = EW.model(de, node_feat, dev)[0]
    if groups is not None:
        walks = tuple(a[groups] for a in walks)
    G, B, W = walks[1].shape[:3]
    etab = None
    if table:
        etab = ex.dropin_edge_table()
        assert etab is not None, "no table mode for these dims"
    node6, eid3, ts3, cat, cut, cnt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in walks)
    with _debug(**debug):
        out = ex.encoder_fwd(node6, eid3, ts3, cat, cut, cnt, G, B, W, M=M, etab=etab)
        torch.cuda.synchronize()
    assert ex._node_zero == (node_feat == "zeros")
    return out.cpu().numpy().reshape(G, B, W)


@functools.lru_cache(maxsize=None)
def _oracle64(de, node_feat, G, B, M):
    _, sd, nf, ef = EW.model(de, node_feat)
    return EW.oracle(sd, nf, ef, G, B, M, double=True)


def _nulls(eid3, M):
    p = eid3 != 0
    assert (~p[..., 0] & p[..., 1] & p[..., 2]).sum() >= FEW, "null position 0, position 1 valid"
    assert (p[..., 0] & ~p[..., 1] & p[..., 2]).sum() >= FEW, "null position 1, position 0 valid"
    assert (~p[..., 2]).reshape(p.shape[0], p.shape[1], N, M).all(-1).sum() >= FEW, "whole null slots"
    assert p.all(-1).sum() >= FEW, "complete walks"


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("de,node_feat,table", CASES)
def test_split_form_vs_float64_oracle(dev, de, node_feat, table, M):
    G, B = SMALL
    w = _walks(G, B, M)
    assert (G * B * N + 15) // 16 == 9 and (G * B * N) % 16
    _nulls(w[1], M)
    imp = _launch(dev, de, node_feat, w, table, M)
    ref = _oracle64(de, node_feat, G, B, M)
    d = np.abs(imp - ref)
    print("de %d (r = %d) %s table %d M %d: max |diff| %.3g, worst diff / bound %.3g"
          % (de, r_of(de), node_feat, table, M, d.max(), (d / (ATOL + RTOL * np.abs(ref))).max()))
    np.testing.assert_allclose(imp, ref, rtol=RTOL, atol=ATOL)


def _same(a, b):
    a, b = a.view(np.uint32), b.view(np.uint32)
    print("%d of %d walks differ" % ((a != b).sum(), a.size))
    assert np.array_equal(a, b)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("de", TAIL_TABLE)
def test_pair_pass_equals_single_position_split_form(dev, de, M):
    w = _walks(*SMALL, M)
    _same(_launch(dev, de, "zeros", w, True, M), _launch(dev, de, "zeros", w, True, M, single=1))


@functools.lru_cache(maxsize=None)
def _single_persistent(de, shape):
    """The single-position pass's imp at M = 3, one unit per wave: the reference of the persistent forms."""
    w = _walks(*shape, 3)
    _nulls(w[1], 3)
    imp = _launch(torch.device("cuda", 0), de, "zeros", w, True, 3, single=1)
    assert np.isfinite(imp).all() and (imp > 0).all()
    imp.setflags(write=False)
    return imp


@pytest.mark.parametrize("shape,units", [(B513, 513), (BIG, 514)])
@pytest.mark.parametrize("de", TAIL_TABLE)
def test_pair_pass_equals_single_position_persistent(dev, de, shape, units):
    assert (shape[0] * shape[1] * N + 15) // 16 == units and (shape[1] * N + 15) // 16 < 512
    _same(_launch(dev, de, "zeros", _walks(*shape, 3), True, 3), _single_persistent(de, shape))


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("de", TAIL_TABLE)
def test_tickets(dev, de, blocks):
    """514 units on one and on three workgroups: nothing of one unit's 16-deep step reaches the next unit."""
    _same(_launch(dev, de, "zeros", _walks(*BIG, 3), True, 3, blocks=blocks), _single_persistent(de, BIG))


@pytest.mark.parametrize("de", TAIL_TABLE)
def test_persistent_launch_equals_split_launches(dev, de):
    G, B = BIG
    M = 2
    w = _walks(G, B, M)
    assert (B * N + 15) // 16 * M <= 3 * 512 and (B * N + 15) // 16 < 512 <= (G * B * N + 15) // 16
    imp = _launch(dev, de, "zeros", w, True, M)
    parts = np.concatenate([_launch(dev, de, "zeros", w, True, M, groups=slice(g, g + 1)) for g in range(G)])
    _same(parts, imp)


# the other instance families with a 16-deep last step, single-position passes: plain mode (nqe 11: the ring hands
# event_gcn's first fp32 fragments over in `pre`), streamed edge features (nqe 21: the edge-feature ring runs beside the
# half-size fragments) and the two-branch table mode (nqe 13, non-zero node features)
OTHER = [(1, "uniform", False), (148, "uniform", False), (33, "uniform", True)]


@functools.lru_cache(maxsize=None)
def _persistent(de, node_feat, table):
    """imp of the persistent form at M = 2, 514 units, one unit per wave."""
    w = _walks(*BIG, 2)
    _nulls(w[1], 2)
    imp = _launch(torch.device("cuda", 0), de, node_feat, w, table, 2)
    assert np.isfinite(imp).all() and (imp > 0).all()
    imp.setflags(write=False)
    return imp


@pytest.mark.parametrize("de,node_feat,table", OTHER)
def test_other_instances_persistent_launch_equals_split_launches(dev, de, node_feat, table):
    G, B = BIG
    assert (B * N + 15) // 16 * 2 <= 3 * 512 and (B * N + 15) // 16 < 512 <= (G * B * N + 15) // 16
    w = _walks(G, B, 2)
    parts = np.concatenate([_launch(dev, de, node_feat, w, table, 2, groups=slice(g, g + 1)) for g in range(G)])
    _same(parts, _persistent(de, node_feat, table))


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("de,node_feat,table", OTHER)
def test_other_instances_tickets(dev, de, node_feat, table, blocks):
    """514 units on one and on three workgroups against one unit per wave."""
    _same(_launch(dev, de, node_feat, _walks(*BIG, 2), table, 2, blocks=blocks), _persistent(de, node_feat, table))


def _pooled(dev, de, blocks):
    ex = EW.model(de, "zeros", dev)[0]
    walks = _walks(*BIG, 3)
    G, B, W = walks[1].shape[:3]
    node6, eid3, ts3, cat, cut, cnt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in walks)
    with _debug(blocks=blocks), torch.no_grad():
        out = ex.enhance_groups(node6, eid3, ts3, cat, cut, cnt, G, B, W, M=3, etab=ex.dropin_edge_table())
        torch.cuda.synchronize()
    assert ex._node_zero
    out = out.cpu().numpy()
    assert out.shape == (G, B, 76) and np.isfinite(out).all() and (out[..., :64] > 0).any()
    return out


@pytest.mark.parametrize("de", TAIL_TABLE)
def test_pooled_forward_tickets(dev, de):
    """The pooled persistent instance (single-position passes) at 514 units: one unit per wave against tickets."""
    ref = _pooled(dev, de, 0)
    for blocks in (1, 3):
        _same(_pooled(dev, de, blocks), ref)


def test_null_positions_of_sampled_walks_through_tickets():
    """The pipeline's early-timeline walks (de = 32; test_gpu_walk_pair asserts the null patterns on the sampled
    walks), 525 units on one workgroup, pair pass against single position."""
    from tests import test_gpu_walk_pair as wp   # its pipeline run and its check of the sampled walks
    wp._same(*wp._pipeline_both(3, 140, 70, blocks=1))
