"""GPU: every kernel instance the edge-feature width selects (edge_width_inputs.WIDTHS; dn = 172, hid_dim = 64,
if_cat_feature = True), at the widths no other GPU test uses.  test_edge_width_cpu.py shows which instance a width
reaches, that the fp32 oracle is within 0.1 of the contract bound on these inputs, and that a dropped edge-feature,
count or time column moves it by at least 5 bounds.

* eval forward, split form (140 slots = 8.75 units): walk_kernel<12 | 13 | 14 | 21 | 22> plain, table, zero-node and
  streamed, and the unfused gcn_kernel + head_kernel at de = 50, against oracle/encoder_ref.forward (fp32) at the
  contract rtol 1e-5, atol 1e-6;
* table mode against the per-walk product, the edge table's values, and the explanation through the per-edge-id gate
  table (gate_reg_kernel<12>, <13>, <22>, <13, 3, 13 | 14>, <22, 11, 22> and the LDS gate_table_kernel);
* the persistent form at de = 4 and 164, bit for bit against the split form;
* the pooled forward (the POOL instances) at de = 4, 36 and 164, and its LDS-tiled path (gcn_kernel +
  head_pool_kernel) at de = 50 and at hid_dim 32.
"""
import numpy as np
import pytest
import torch

import edge_width_inputs as EW
from edge_width_inputs import ATOL, BIG, N, RTOL, SMALL, WIDTHS, _walks

pytestmark = pytest.mark.gpu

TABLE_WIDTHS = tuple(de for de in EW.NEW_WIDTHS if WIDTHS[de]["table"])
EXPLAIN_WIDTHS = (16, 20, 24, 33, 36, 37, 148, 164, 168, 176)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


def profiled(fn):
    from test_gpu_enhance_train import profiled as p
    return p(fn)


def _launch(dev, de, node_feat, walks, table, M, groups=None):
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
    out = ex.encoder_fwd(node6, eid3, ts3, cat, cut, cnt, G, B, W, M=M, etab=etab)
    torch.cuda.synchronize()
    assert ex._node_zero == (node_feat == "zeros")
    return out.cpu().numpy().reshape(G, B, W)


def _close(a, ref, what=""):
    d = np.abs(a - ref)
    print("%s max |diff| %.3g, worst diff / bound %.3g (ref spread %.3g)"
          % (what, d.max(), (d / (ATOL + RTOL * np.abs(ref))).max(), ref.max() - ref.min()))
    np.testing.assert_allclose(a, ref, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ eval forward, split form
FWD_CASES = [(de, t) for de in EW.NEW_WIDTHS for t in ((False, True) if WIDTHS[de]["table"] else (False,))]


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("node_feat", ["uniform", "zeros"])
@pytest.mark.parametrize("de,table", FWD_CASES)
def test_split_form_vs_oracle(dev, de, table, node_feat, M):
    G, B = SMALL
    imp, count = profiled(lambda: _launch(dev, de, node_feat, _walks(G, B, M), table, M))
    if WIDTHS[de]["fused"]:
        assert count("walk_kernel") == 1 and count("gcn_kernel") == 0 and count("head_kernel") == 0
    else:
        assert count("walk_kernel") == 0 and count("gcn_kernel") == 1 and count("head_kernel") == 1
    _close(imp, EW.oracle32(de, node_feat, G, B, M), "de %d %s table %d M %d:" % (de, node_feat, table, M))


@pytest.mark.parametrize("de", list(EW.NEW_WIDTHS))
def test_table_exists_exactly_where_widths_says(dev, de):
    ex = EW.model(de, "uniform", dev)[0]
    assert (ex.dropin_edge_table() is None) == (not WIDTHS[de]["table"])


# ------------------------------------------------------------------ table mode
@pytest.mark.parametrize("node_feat", ["uniform", "zeros"])
@pytest.mark.parametrize("de", TABLE_WIDTHS)
def test_table_mode_agrees_with_per_walk_product(dev, de, node_feat):
    G, B = SMALL
    w = _walks(G, B, 3)
    _close(_launch(dev, de, node_feat, w, True, 3), _launch(dev, de, node_feat, w, False, 3),
           "de %d %s table vs per-walk:" % (de, node_feat))


def _check_etab(ex, etab, e_feat, de):
    w = ex.event_conv.lin_event.weight.detach().double().cpu()
    want = e_feat.double()[:etab.shape[0]] @ w[:, :de].T + ex.event_conv.lin_event.bias.detach().double().cpu()
    got = etab.double().cpu()
    assert tuple(got.shape) == (want.shape[0], 176)
    d = (got[:, :172] - want).abs()
    print("de %d etab [%d rows]: worst diff / bound %.3g" % (de, got.shape[0], float((d / (1e-6 + 1e-5 * want.abs())).max())))
    np.testing.assert_allclose(got[:, :172].numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
    assert (got[:, 172:] == 0).all()


@pytest.mark.parametrize("de", TABLE_WIDTHS)
def test_edge_feature_table_values(dev, de):
    """tm_edge_feature_table (the drop-in's table, no gate): W[:, :de] E[e] + b in fp64, zero past dn; 501 rows =
    7 full 64-row blocks and a partial one."""
    ex, _, _, ef = EW.model(de, "uniform", dev)
    etab = ex.dropin_edge_table()
    assert etab.shape[0] == EW.N_EDGES + 1 and etab.shape[0] % 64 != 0
    _check_etab(ex, etab, ef, de)


@pytest.mark.parametrize("de", EXPLAIN_WIDTHS)
def test_edge_tables_and_explanation_vs_oracle(dev, de):
    """The pipeline on a small graph: tm_edge_tables builds the gate table (and the edge table where the width has
    one) over max_eid + 1 edge ids, not a multiple of 64; the importances and the explanation of hop 1 and hop 2
    against oracle/encoder_ref on the C oracle's samples, within the contract; the edge table against fp64."""
    import tempme_amd as tm
    from oracle import encoder_ref as er
    from oracle import oracle as orc
    from tempme_amd.pipeline import ExplainPipeline
    from tempme_amd.workload import enron_like, split
    g = enron_like(n_nodes=60, n_edges=3000, de=de, node_feat="uniform", seed=3)
    (src, dst, ts, eidx), rows, pool = split(g)
    Nn, B = 8, 16
    f = tm.NeighborFinder.from_edges(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"],
                                     device=dev, seed=1)
    assert (f.graph.max_eid + 1) % 64 != 0
    torch.manual_seed(de)
    ex = tm.TempME(EW.Base(g["n_feat"], g["e_feat"]), "tgn", "enron_sampled", 40, 64, device=dev,
                   null_model={k: 1 / 12 for k in range(1, 13)}).to(dev).eval()
    pipe = ExplainPipeline(ex, f.graph, torch.from_numpy(pool), Nn, 3, B, seed=1)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:B], dtype=dt)).to(dev)  # noqa: E731
    imp, h1, h2 = pipe.run(t(src, np.int32), t(dst, np.int32), t(ts, np.float64), t(eidx, np.int32),
                           torch.arange(B, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    pipe.check_errors()
    assert (pipe.etab is not None) == WIDTHS[de]["table"] and pipe.gf.numel() == f.graph.max_eid + 1
    og = orc.OracleGraph(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"])
    o = orc.event_pipeline(og, 1, tm.SPLIT_TEST, Nn, 3, src[:B], dst[:B], ts[:B], eidx[:B], np.arange(B), pool)
    assert np.array_equal(pipe.buf.eid3.cpu().numpy().swapaxes(0, 1), o["eid3"]), "sampled walks differ from oracle"
    sd = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    nf, ef = torch.from_numpy(g["n_feat"]), torch.from_numpy(g["e_feat"])
    for s in range(3):
        ref = er.forward(sd, nf, ef, o["node6"][:, s], o["eid3"][:, s], o["ts3"][:, s], o["cat"][:, s], ts[:B],
                         o["cnt"][:, s].astype(np.float64))
        _close(imp[s].cpu().numpy(), ref.numpy()[..., 0], "de %d side %d imp:" % (de, s))
        e0, e1 = er.edge_importance(sd, ef, ref, o["eid3"][:, s], o["ts3"][:, s],
                                    [o["sub1_node"][:, s], o["sub2_node"][:, s]],
                                    [o["sub1_eid"][:, s], o["sub2_eid"][:, s]])
        assert float(e0.max()) > 0 and float(e1.max()) > 0
        _close(h1[s].cpu().numpy(), e0.numpy(), "de %d side %d hop 1:" % (de, s))
        _close(h2[s].cpu().numpy(), e1.numpy(), "de %d side %d hop 2:" % (de, s))
    if pipe.etab is not None:
        _check_etab(ex, pipe.etab, ef, de)


# ------------------------------------------------------------------ persistent form
@pytest.mark.parametrize("de", [4, 164])
def test_persistent_form_vs_oracle_and_split_form(dev, de):
    """514 units in one call (persistent form) against the oracle, and bit for bit against the three groups' own
    calls of 172 units (split form): narrow with an even K-step count (de = 4), streamed (de = 164)."""
    G, B = BIG
    M = 3
    w = _walks(G, B, M)
    units = (G * B * N + 15) // 16
    assert units == 514 and (G * B * N) % 16 != 0 and (B * N + 15) // 16 * M <= 3 * 512
    imp = _launch(dev, de, "uniform", w, False, M)
    _close(imp, EW.oracle32(de, "uniform", G, B, M), "de %d persistent:" % de)
    parts = np.concatenate([_launch(dev, de, "uniform", w, False, M, groups=slice(g, g + 1)) for g in range(G)])
    assert np.array_equal(parts.view(np.uint32), imp.view(np.uint32))


# ------------------------------------------------------------------ pooled forward (POOL instances)
def _pooled_vs_fp64(de, table, zero_nodes, hid_dim=64):
    """enhance_groups against tests/enhance_train_ref.groups in fp64: 10 times the restatement's own fp32-vs-fp64
    distance at this shape (the convention of test_gpu_enhance_train.py), and twice the same bits.  Returns the
    profile's launch count per name of the first run."""
    import enhance_train_ref as TR
    from test_gpu_enhance_train import SHAPES, build
    ex, d = build(shape=SHAPES["2x3x7"], de=de, zero_nodes=zero_nodes, hid_dim=hid_dim)
    ex.eval()
    sd, tg, ic = d["sd"], ex.use_temporal_guidance, ex.if_cat
    r64 = TR.groups({k: v.double() for k, v in sd.items()}, d, tg, ic)
    tol = 10 * float((TR.groups(sd, d, tg, ic).double() - r64).abs().max())
    etab = ex.dropin_edge_table() if table else None
    assert (etab is not None) == table

    def fwd():
        with torch.no_grad():
            return ex.enhance_groups(*d["args"], etab=etab).clone()
    a, count = profiled(fwd)
    assert ex._node_zero == zero_nodes
    b = fwd()
    dist = float((a.cpu().double() - r64).abs().max())
    print("de %d hid_dim %d table %d zero_nodes %d: pooled vs fp64 %.3g, tolerance %.3g, ratio %.3g"
          % (de, hid_dim, table, zero_nodes, dist, tol, dist / tol))
    assert tuple(a.shape) == (d["G"], d["B"], ex.mlp_dim)
    assert dist <= tol
    assert torch.equal(a, b)
    return count


@pytest.mark.parametrize("de,table,zero_nodes", [(4, False, False), (4, False, True), (36, False, False),
                                                 (36, True, False), (36, True, True), (164, False, False)])
def test_pooled_forward_vs_fp64(dev, de, table, zero_nodes):
    count = _pooled_vs_fp64(de, table, zero_nodes)
    assert count("walk_pool_kernel") == 1 and count("pool_tail_kernel") == 1 and count("gcn_kernel") == 0


@pytest.mark.parametrize("de,hid_dim,zero_nodes", [(50, 64, False), (50, 64, True), (32, 32, False)])
def test_pooled_forward_tiled_path_vs_fp64(dev, de, hid_dim, zero_nodes):
    """The same at dims the fused kernel refuses (15 K steps of 16 at de = 50; hid_dim 32): gcn_kernel, then
    head_kernel's POOL instance, then the pool tail."""
    count = _pooled_vs_fp64(de, False, zero_nodes, hid_dim)
    assert count("gcn_kernel") == 1
    assert count("head_pool_kernel") == 1
    assert count("pool_tail_kernel") == 1
    assert count("walk_pool_kernel") == 0
