"""walk_kernel's lin_event on bf16 MFMA (v_mfma_f32_16x16x32_bf16, both operands split exactly into three bf16
parts, six products per (tile, 32-wide K step), fp32 accumulation) against oracle/encoder_ref.forward (CPU,
torch fp32) at the project's contract rtol=1e-5, atol=1e-6, on synthetic walks that reach every path of the new
K loop at the smallest shapes:

* edge dimension: de = 32 (table mode starts at an aligned step: step 0 is skipped), de = 1 (the dims of
  tests/encoder_inputs.py: edge feature, counts and cosines share step 0; no table mode exists), de = 172 with
  node features (two-branch instance, 22 K steps of 16 = 11 of 32: table mode's shared first step with the edge
  lanes zeroed, plain mode's streamed edge features);
* table mode and plain mode, M = 1 and 3 walks per slot;
* 7 events = 140 slots = 8 units and three quarters (split form, last unit partial) and 3 groups x 137 events =
  8220 slots = 514 units less a quarter (persistent form, just over its 512-unit threshold, last unit partial);
* null positions (edge id 0 / node 0 at position 0, at position 1, in whole slots);
* dt = 0, 1 and 1e8 exactly, and random in between; edge counts 0, 1, 2, 3 and 60.

Also: the persistent launch of three groups equals the three groups' split launches bit for bit; table mode
agrees with the per-walk product within the contract; and the error against the oracle evaluated in float64 stays
within twice what the fp32-MFMA lin_event measured on the same input (PARENT_MAX_ERR64).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6
N = 20
CONFIGS = {"de32": (32, 172, "zeros"), "de1": (1, 172, "uniform"), "de172": (172, 172, "uniform")}
N_NODES, N_EDGES = 60, 500
SMALL = (1, 7)          # groups, events per group: 140 slots
BIG = (3, 137)          # 8220 slots = 513.75 units

# max |imp - float64 oracle| of the fp32-MFMA lin_event (the parent commit's build of the library) on
# budget_case()'s input, measured once on an MI355X with this file's test_error_budget (it prints the figure
# before it asserts); DESIGN section 6j records the run
PARENT_MAX_ERR64 = 5.383e-08


@functools.lru_cache(maxsize=None)
def _model(cfg):
    import tempme_amd as tm
    de, dn, node_feat = CONFIGS[cfg]
    rng = np.random.RandomState(5)
    e_feat = rng.uniform(0, 1, (N_EDGES + 1, de)).astype(np.float32)
    e_feat[0] = 0
    n_feat = np.zeros((N_NODES + 1, dn), np.float32)
    if node_feat != "zeros":
        n_feat[1:] = rng.uniform(0, 1, (N_NODES, dn))
    dev = torch.device("cuda", 0)

    class Base:
        n_feat_th = torch.from_numpy(n_feat)
        e_feat_th = torch.from_numpy(e_feat)
        node_raw_features = torch.nn.Embedding.from_pretrained(n_feat_th, padding_idx=0, freeze=True)
        edge_raw_features = torch.nn.Embedding.from_pretrained(e_feat_th, padding_idx=0, freeze=True)

    torch.manual_seed(7)
    ex = tm.TempME(Base(), "tgn", "synthetic", 40, 64, device=dev,
                   null_model={k: 1 / 12 for k in range(1, 13)}).to(dev).eval()
    sd = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    return ex, sd, torch.from_numpy(n_feat), torch.from_numpy(e_feat)


@functools.lru_cache(maxsize=None)
def _walks(G, B, M):
    """Synthetic walks [G, B, W, ...] with find_k_walks' layout: the M walks of a slot share position 2."""
    rng = np.random.RandomState(100 * G + 10 * B + M)
    S, W = N, N * M
    sh = (G, B, S, M)
    node6 = rng.randint(1, N_NODES + 1, sh + (6,)).astype(np.int32)
    eid3 = rng.randint(1, N_EDGES + 1, sh + (3,)).astype(np.int32)
    cnt = rng.choice(np.array([0, 1, 2, 3, 60], np.float32), sh + (3, 3))
    cat = rng.randint(0, 12, sh).astype(np.int32)
    # position 2's time per slot, then each position's dt of a kind: 0, 1, 1e8, random
    t2 = rng.choice(np.array([1e8, 5.0, 1.25, -1.0], np.float32), (G, B, S, 1))
    t2 = np.where(t2 < 0, rng.uniform(0, 1e8, t2.shape).astype(np.float32), t2).astype(np.float32)
    t2 = np.broadcast_to(t2, sh)
    ts3 = np.empty(sh + (3,), np.float32)
    ts3[..., 2] = t2
    for p in (0, 1):
        kind = rng.randint(0, 4, sh)
        tp = np.where(kind == 0, t2, np.where(kind == 1, np.maximum(t2 - np.float32(1.0), 0),
                      np.where(kind == 2, np.float32(0.0), (t2 * rng.uniform(0, 1, sh)).astype(np.float32))))
        ts3[..., p] = tp.astype(np.float32)
    # position 2 is the slot's: the M walks share its edge, nodes and counts
    node6[..., 4:6] = node6[..., :1, 4:6]
    eid3[..., 2] = eid3[..., :1, 2]
    cnt[..., 2, :] = cnt[..., :1, 2, :]
    # null positions: position 0, position 1, whole slots
    null = rng.randint(0, 8, sh)
    for p, sel in ((0, null == 0), (1, null == 1)):
        eid3[..., p][sel] = 0
        node6[..., 2 * p][sel] = 0
        node6[..., 2 * p + 1][sel] = 0
        cnt[..., p, :][sel] = 0
    slot_null = np.broadcast_to((rng.randint(0, 10, (G, B, S, 1)) == 0), sh)
    eid3[slot_null] = 0
    node6[slot_null] = 0
    cnt[slot_null] = 0
    assert (ts3[..., 2] - ts3[..., 0] == 1e8).any() and (ts3[..., 2] - ts3[..., 1] == 1.0).any()
    assert (ts3[..., 2] == ts3[..., 0]).any() and (cnt == 60).any() and slot_null.any()
    cut = (2.0 ** 27 + 16.0 * rng.randint(0, 1000, (G, B))).astype(np.float64)   # past every walk time, exact in fp32
    r = lambda a, *tail: np.ascontiguousarray(a.reshape((G, B, W) + tail))   # noqa: E731
    return r(node6, 6), r(eid3, 3), r(ts3, 3), r(cat), cut, r(cnt, 3, 3)


def _launch(cfg, walks, table, M, groups=None):
    """imp [G, B, W] of one tm_encoder_fwd_tab call over the groups (default: all of them)."""
    ex, _, _, _ = _model(cfg)
    dev = torch.device("cuda", 0)
    if groups is not None:
        walks = tuple(a[groups] for a in walks)
    G, B, W = walks[1].shape[:3]
    etab = None
    if table:
        etab = ex.dropin_edge_table()
        assert etab is not None, "no table mode for these dims"
    node6, eid3, ts3, cat, cut, cnt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in walks)
    out = ex.encoder_fwd(node6, eid3, ts3, cat, cut, cnt, G, B, W, M=M, etab=etab)
    torch.cuda.synchronize()
    assert ex._node_zero == (CONFIGS[cfg][2] == "zeros")
    return out.cpu().numpy().reshape(G, B, W)


@functools.lru_cache(maxsize=None)
def _oracle(cfg, G, B, M, double=False):
    from oracle import encoder_ref as er
    _, sd, nf, ef = _model(cfg)
    if double:
        sd = {k: v.double() for k, v in sd.items()}
    node6, eid3, ts3, cat, cut, cnt = _walks(G, B, M)
    out = [er.forward(sd, nf, ef, node6[g], eid3[g], ts3[g], cat[g], cut[g], cnt[g].astype(np.float64)).numpy()[..., 0]
           for g in range(G)]
    return np.stack(out)


def _close(a, ref):
    d = np.abs(a - ref)
    print("max |diff| %.3g, worst diff / bound %.3g (ref spread %.3g)"
          % (d.max(), (d / (ATOL + RTOL * np.abs(ref))).max(), ref.max() - ref.min()))
    np.testing.assert_allclose(a, ref, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("cfg,table", [("de32", True), ("de32", False), ("de1", False), ("de172", True),
                                       ("de172", False)])
def test_split_form_vs_oracle(cfg, table, M):
    """8.75 units, the split form: every instance of the K loop against the fp32 oracle."""
    G, B = SMALL
    imp = _launch(cfg, _walks(G, B, M), table, M)
    _close(imp, _oracle(cfg, G, B, M))


def test_no_table_mode_for_de1():
    assert _model("de1")[0].dropin_edge_table() is None


@pytest.mark.parametrize("cfg", ["de32", "de172"])
def test_table_mode_agrees_with_per_walk_product(cfg):
    G, B = SMALL
    w = _walks(G, B, 3)
    _close(_launch(cfg, w, True, 3), _launch(cfg, w, False, 3))


@pytest.mark.parametrize("M", [1, 3])
def test_persistent_form_vs_oracle_and_split_form(M):
    """514 units in one call (persistent form); the same rows as three calls of 172 units (split form: the
    std is per group, so a group's results do not depend on the call): equal bit for bit."""
    G, B = BIG
    w = _walks(G, B, M)
    units = (G * B * N + 15) // 16
    assert units == 514 and (G * B * N) % 16 != 0 and (B * N + 15) // 16 * M <= 3 * 512
    imp = _launch("de32", w, True, M)
    _close(imp, _oracle("de32", G, B, M))
    parts = np.concatenate([_launch("de32", w, True, M, groups=slice(g, g + 1)) for g in range(G)])
    assert np.array_equal(parts.view(np.uint32), imp.view(np.uint32))


def budget_case():
    return "de32", SMALL, 3


def test_error_budget():
    """The split lin_event is no worse than the fp32 one against the float64 oracle: at most twice the parent
    build's measured maximum error on this input (the factor covers the summation order inside one bf16 MFMA,
    which the CPU model of the split does not know).  Measured: parent build 5.383e-08, this build 5.383e-08
    (both one rounding of a sigmoid output near 0.5)."""
    cfg, (G, B), M = budget_case()
    imp = _launch(cfg, _walks(G, B, M), True, M).astype(np.float64)
    err = np.abs(imp - _oracle(cfg, G, B, M, True).astype(np.float64)).max()
    print("max |imp - float64 oracle| = %.4g (fp32-MFMA parent: %s)" % (err, PARENT_MAX_ERR64))
    assert err <= 2 * PARENT_MAX_ERR64
