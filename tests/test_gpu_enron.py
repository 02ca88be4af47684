"""GPU parity in the bench regime: the HIP path through the C ABI on
the full-Enron-shaped graph (V=184, E=125,235, timestamps in [0, 1e8)) against

* outputs of the reference itself (tests/golden/enron_goldens.npz, make_goldens.py case_enron):
  sampled fields / categories / marginals / edge counts bit-exact; TempME forward, retrieve_explanation
  (eval) and kl_loss within rtol 1e-5 / atol 1e-6 for the default constructor and the
  use_temporal_guidance=False / use_dependency_aware_sampling=False / hid_dim=32 variants, through both
  the drop-in TempME surface and the bench's ExplainPipeline; one deterministic training iteration
  (losses, logits, every gradient, the Adam update);
* the C / torch-fp32 oracle at the bench shapes: 400 events of full Enron at N=20 and 200 events of the
  1M-edge de=dn=172 graph at N=30 (configs[4]), every sampled field and count bit-exact, the encoder on
  one reference batch per side.
"""
import numpy as np
import pytest
import torch

import enron_inputs as EI
from oracle import encoder_ref as er
from oracle import oracle as orc
from oracle import philox as px
from tests.test_gpu_parity import _Base, _check_events

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z():
    return EI.golden()


@pytest.fixture(scope="module")
def g(z):
    return EI.graph(z)


@pytest.fixture(scope="module")
def finder(dev, g):
    import tempme_amd as tm
    return tm.NeighborFinder.from_edges(g["src"], g["dst"], g["eidx"], g["ts"], g["n_nodes"], device=dev, seed=0,
                                        split=px.SPLIT_TEST)


def _explainer(dev, g, z, tag, **kw):
    import tempme_amd as tm
    ctor = dict(out_dim=40, hid_dim=64)
    ctor.update(kw)
    ex = tm.TempME(_Base(g["n_feat"], g["e_feat"], dev), "tgn", "enron", device=dev, null_model=EI.null(z), **ctor)
    missing, unexpected = ex.load_state_dict(EI.weights(z, tag), strict=False)
    assert not unexpected
    return ex.to(dev).eval()


@pytest.mark.parametrize("N", sorted(EI.SETS))
def test_sampling_matches_reference_enron(finder, z, N):
    _check_events(None, finder, z, f"test_N{N}_", 0, px.SPLIT_TEST, N, 3, z["test_src"], z["test_dst"],
                  z["test_ts"], z["test_eidx"], z["test_sampler_dst"], EI.SETS[N])


@pytest.mark.parametrize("tag", ["N20_base", "N20_notg", "N20_nodep", "N20_h32", "N30_base"])
def test_dropin_tempme_matches_reference_enron(dev, g, z, tag):
    """The drop-in surface as eval_one_epoch calls it (temp_exp_main.py:446-452): TempME.forward x3 from
    the H5 pack's numpy arrays, retrieve_explanation(training=False), kl_loss."""
    N, var = int(tag[1:3]), tag[4:]
    ex = _explainer(dev, g, z, tag, **EI.VARIANTS[var])
    d = EI.walks(z, N)
    imps, subs, walks = [], [], []
    for s in EI.SIDES:
        x = d[s]
        w = (x["node"], x["eid"], x["ts"], x["cat"], x["marg"])
        with torch.no_grad():
            imp = ex(w, d["ts_cut"], x["cnt"])
        np.testing.assert_allclose(imp.cpu().numpy(), z[f"{tag}_imp_{s}"], rtol=RTOL, atol=ATOL, err_msg=s)
        imps.append(imp)
        subs.append((x["sub_node"], x["sub_eid"], x["sub_ts"]))
        walks.append(w)
    expl = ex.retrieve_explanation(subs[0], imps[0], walks[0], subs[1], imps[1], walks[1], subs[2], imps[2],
                                   walks[2], training=False)
    np.testing.assert_allclose(expl[0].detach().cpu().numpy(), z[f"{tag}_expl0"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(expl[1].detach().cpu().numpy(), z[f"{tag}_expl1"], rtol=RTOL, atol=ATOL)
    for k in range(3):
        kl = ex.kl_loss(imps[k], walks[k], target=0.3)
        np.testing.assert_allclose(float(kl), z[f"{tag}_kl"][k], rtol=RTOL, atol=ATOL)
    # every variant runs the HIP eval kernels (tm_weights_variant / tm_weights_create_ex; hid_dim 32 on the
    # LDS-tiled kernels), never the torch formulation
    assert ex._packed is not None, "the HIP encoder did not run"


def test_dropin_staged_numpy_equals_device_tensors(dev, g, z):
    """Host numpy inputs take the pinned staging path (one async copy per call, cast on the host); device
    tensors take the per-array path.  Same kernels on the same values: bit-identical outputs, across
    more calls than the stager has slots (its pinned buffers are reused)."""
    tag = "N20_base"
    ex = _explainer(dev, g, z, tag)
    d = EI.walks(z, 20)
    to_dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    for rep in range(3):
        for s in EI.SIDES:
            x = d[s]
            w_np = (x["node"], x["eid"], x["ts"], x["cat"], x["marg"])
            w_t = (to_dev(x["node"], torch.int32), to_dev(x["eid"], torch.int32), to_dev(x["ts"], torch.float32),
                   to_dev(x["cat"], torch.int32), x["marg"])
            with torch.no_grad():
                a = ex(w_np, d["ts_cut"], x["cnt"])
                b = ex(w_t, to_dev(d["ts_cut"], torch.float64), to_dev(x["cnt"], torch.float32))
            assert torch.equal(a, b), (rep, s)
            sub = (x["sub_node"], x["sub_eid"], x["sub_ts"])
            sub_t = ([to_dev(v, torch.int32) for v in x["sub_node"]], [to_dev(v, torch.int32) for v in x["sub_eid"]],
                     x["sub_ts"])
            e1 = ex.retrieve_edge_imp_node(sub, a, w_np, training=False)
            e2 = ex.retrieve_edge_imp_node(sub_t, a, w_t, training=False)
            assert torch.equal(e1[0], e2[0]) and torch.equal(e1[1], e2[1]), (rep, s)


@pytest.mark.parametrize("edge_table", [True, False])
@pytest.mark.parametrize("N", sorted(EI.SETS))
def test_pipeline_matches_reference_enron(dev, finder, g, z, N, edge_table):
    """The bench's ExplainPipeline (one fused sampling launch, edge tables, table-mode encoder,
    table-driven explanation) on the golden events = the reference's pre_processing -> TempME.forward x3
    -> retrieve_explanation(eval) on the same events (one reference batch)."""
    from tempme_amd.pipeline import ExplainPipeline
    tag = f"N{N}_base"
    ex = _explainer(dev, g, z, tag)
    E = EI.SETS[N]
    pipe = ExplainPipeline(ex, finder.graph, torch.from_numpy(z["test_sampler_dst"]), N, 3, E, seed=0,
                           split=px.SPLIT_TEST, edge_table=edge_table)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:E], dtype=dt)).to(dev)  # noqa: E731
    imp, h1, h2 = pipe.run(t(z["test_src"], np.int32), t(z["test_dst"], np.int32), t(z["test_ts"], np.float64),
                           t(z["test_eidx"], np.int32), torch.arange(E, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    pipe.check_errors()
    for s_i, s in enumerate(EI.SIDES):
        np.testing.assert_allclose(imp[s_i].cpu().numpy(), z[f"{tag}_imp_{s}"][..., 0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(h1.reshape(3 * E, N).cpu().numpy(), z[f"{tag}_expl0"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(h2.reshape(3 * E, N * N).cpu().numpy(), z[f"{tag}_expl1"], rtol=RTOL, atol=ATOL)


def _golden_train_step(dev, g, z):
    """The golden training iteration (make_goldens.py case_enron): -> (explainer after the step, train_step's
    outputs, the parameters before it, the walks record of its N = 20 batch)."""
    from tempme_amd import TempME
    from tempme_amd.train import Batch, train_step
    N, B = 20, EI.SETS[20]
    base = EI.build_tgn(z, g).to(dev)
    ex = TempME(base, "tgn", "enron", out_dim=40, hid_dim=64, temp=0.07, if_cat_feature=True, dropout_p=0.1,
                device=dev, null_model=EI.null(z))
    missing, unexpected = ex.load_state_dict(EI.weights(z, "train"), strict=False)
    assert not unexpected
    ex = ex.to(dev)
    d = EI.walks(z, N)
    pre = f"test_N{N}_"
    sg = [tuple([z[pre + f"subgraph_{s}_{h}_{k}"][:B].astype(np.float64) for h in (0, 1)]
                for k in ("node", "eid", "ts")) for s in EI.SIDES]
    walks = [(d[s]["node"], d[s]["eid"], d[s]["ts"], d[s]["cat"], d[s]["marg"]) for s in EI.SIDES]
    batch = Batch(z["test_src"][:B].astype(np.int64), z["test_dst"][:B].astype(np.int64), d["ts_cut"],
                  z["test_eidx"][:B].astype(np.int64), z[pre + "dst_fake"][:B].astype(np.float64), sg, walks,
                  [d[s]["cnt"] for s in EI.SIDES])
    opt = torch.optim.Adam(ex.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    p0 = {k: v.detach().clone() for k, v in ex.named_parameters()}
    ex.eval()
    out = train_step(ex, base, opt, batch, beta=0.5, prior_p=0.3, if_bern=False)
    return ex, out, p0, d


def test_train_step_matches_reference_enron(dev, g, z):
    """One deterministic iteration of the training loop (temp_exp_main.py:605-632, Explainer.eval(),
    Beta mean) on the reference TGN at Enron dims and timestamps: losses, logits, every gradient that
    reaches the explainer, and the Adam update."""
    ex, out, p0, _ = _golden_train_step(dev, g, z)
    got = np.array([out["loss"].item(), out["pred_loss"].item(), out["kl_loss"].item()])
    np.testing.assert_allclose(got, z["train_losses"], rtol=1e-5, atol=1e-6)
    logits = torch.cat([out["pos_logit"], out["neg_logit"]]).cpu().numpy()
    np.testing.assert_allclose(logits, z["train_logits"], atol=2e-5, rtol=1e-5)
    ref_keys = {k[len("train_grad_"):] for k in z.files if k.startswith("train_grad_")}
    assert {k for k, v in ex.named_parameters() if v.grad is not None} == ref_keys
    for k, v in ex.named_parameters():
        if k not in ref_keys:
            continue
        gr = z[f"train_grad_{k}"].astype(np.float64)
        ga = v.grad.detach().cpu().numpy().astype(np.float64)
        scale = np.abs(gr).max()
        assert np.linalg.norm(ga - gr) <= 2e-4 * np.linalg.norm(gr) + 1e-9, k
        assert np.abs(ga - gr).max() <= 1e-8 + 2e-4 * scale, k
        upd = (v.detach() - p0[k]).cpu().numpy()
        sure = np.abs(gr) > max(1e-3 * scale, 1e-7)
        np.testing.assert_allclose(upd[sure], z[f"train_upd_{k}"][sure], atol=2e-6, rtol=1e-3, err_msg=k)


def _oracle_check(tm, dev, g, rows, ev, pool, N, E, B, seed, n_batches_enc, ex):
    """Pipeline on E events vs the C oracle (every sampled field and count) and the torch-fp32 encoder
    oracle on ``n_batches_enc`` reference batches per side."""
    from tempme_amd.pipeline import ExplainPipeline
    src, dst, ts, eidx = ev
    f = tm.NeighborFinder.from_edges(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"],
                                     device=dev, seed=seed, split=px.SPLIT_TEST)
    pipe = ExplainPipeline(ex, f.graph, torch.from_numpy(pool), N, 3, B, seed=seed, split=px.SPLIT_TEST)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:E], dtype=dt)).to(dev)  # noqa: E731
    imp, h1, h2 = pipe.run(t(src, np.int32), t(dst, np.int32), t(ts, np.float64), t(eidx, np.int32),
                           torch.arange(E, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    pipe.check_errors()
    og = orc.OracleGraph(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"])
    o = orc.event_pipeline(og, seed, px.SPLIT_TEST, N, 3, src[:E], dst[:E], ts[:E], eidx[:E], np.arange(E), pool, 16)
    b = pipe.buf
    h = lambda x: x.cpu().numpy()  # noqa: E731
    assert np.array_equal(h(b.dst_fake[:E]), o["dst_fake"])
    for name in ("node6", "eid3", "ts3", "cat", "sub1_node", "sub1_eid", "sub1_ts", "sub2_node", "sub2_eid",
                 "sub2_ts"):
        assert np.array_equal(h(getattr(b, name)).swapaxes(0, 1), o[name]), name
    assert np.array_equal(h(b.cnt).swapaxes(0, 1).astype(np.int32), o["cnt"])
    assert np.array_equal(h(b.hist).astype(np.uint64), o["hist"])
    sd = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    nf, ef = torch.from_numpy(g["n_feat"]), torch.from_numpy(g["e_feat"])
    for bi in range(n_batches_enc):
        sl = slice(bi * B, (bi + 1) * B)
        for s in range(3):
            ref = er.forward(sd, nf, ef, o["node6"][sl, s], o["eid3"][sl, s], o["ts3"][sl, s], o["cat"][sl, s],
                             ts[sl], o["cnt"][sl, s].astype(np.float64))
            np.testing.assert_allclose(h(imp[s, sl]), ref.numpy()[..., 0], rtol=RTOL, atol=ATOL)
            e0, e1 = er.edge_importance(sd, ef, ref, o["eid3"][sl, s], o["ts3"][sl, s],
                                        [o["sub1_node"][sl, s], o["sub2_node"][sl, s]],
                                        [o["sub1_eid"][sl, s], o["sub2_eid"][sl, s]])
            np.testing.assert_allclose(h(h1[s, sl]), e0.numpy(), rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(h(h2[s, sl]), e1.numpy(), rtol=RTOL, atol=ATOL)


def test_full_enron_400_events_vs_oracle(dev, g):
    """configs[2]/[3] bench shape: 400 events (4 reference batches) of the full-Enron graph at N=20, zero
    node features as the bench runs it, encoder + explanation on two batches per side."""
    import tempme_amd as tm
    from tempme_amd.workload import enron_like, split
    gz = enron_like(n_nodes=184, n_edges=125235, alpha=1.2, seed=0)            # bench.py's graph
    ev, rows, pool = split(gz)
    torch.manual_seed(0)
    ex = tm.TempME(_Base(gz["n_feat"], gz["e_feat"], dev), "tgn", "enron", 40, 64, device=dev,
                   null_model={k: 1 / 12 for k in range(1, 13)}).to(dev).eval()
    _oracle_check(tm, dev, gz, rows, ev, pool, 20, 400, 100, 0, 2, ex)


def test_1m_edge_200_events_vs_oracle(dev):
    """configs[4] bench shape: the synthetic 1M-edge graph (V=100,000, Pareto 1.5, de=dn=172 U(0,1)
    features) at N=30, 200 events; encoder + explanation on one reference batch per side."""
    import tempme_amd as tm
    from tempme_amd.workload import enron_like, split
    gz = enron_like(n_nodes=100000, n_edges=1000000, alpha=1.5, de=172, dn=172, seed=0, node_feat="uniform")
    ev, rows, pool = split(gz)
    torch.manual_seed(0)
    ex = tm.TempME(_Base(gz["n_feat"], gz["e_feat"], dev), "tgn", "synth", 40, 64, device=dev,
                   null_model={k: 1 / 12 for k in range(1, 13)}).to(dev).eval()
    _oracle_check(tm, dev, gz, rows, ev, pool, 30, 200, 100, 0, 1, ex)


def test_dropin_equals_pipeline(dev, finder, g, z):
    """The drop-in surface (eval_one_epoch's calls from the host pack the pipeline sampled: TempME.forward x3
    in table mode, retrieve_explanation per-walk gate) returns exactly what the fused pipeline returns for the
    same events (bench.py reports both throughputs)."""
    from tempme_amd import pack as P
    from tempme_amd.pipeline import ExplainPipeline
    N, E = 20, EI.SETS[20]
    ex = _explainer(dev, g, z, "N20_base")
    pipe = ExplainPipeline(ex, finder.graph, torch.from_numpy(z["test_sampler_dst"]), N, 3, E, seed=0,
                           split=px.SPLIT_TEST)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:E], dtype=dt)).to(dev)  # noqa: E731
    imp, h1, h2 = [x.clone() for x in pipe.run(t(z["test_src"], np.int32), t(z["test_dst"], np.int32),
                                                t(z["test_ts"], np.float64), t(z["test_eidx"], np.int32),
                                                torch.arange(E, dtype=torch.int32, device=dev))]
    _, cat_d, edge = P.buffers_to_arrays(pipe.buf, E)

    class A:
        n_degree = N
    sg_s, sg_t, sg_b, w_s, w_t, w_b, _ = P.get_item(P.load_subgraph_margin(A(), cat_d), np.arange(E))
    e_s, e_t, e_b = P.get_item_edge(edge, np.arange(E))
    cut = z["test_ts"][:E].astype(np.float64)
    assert ex.dropin_edge_table() is not None
    # twice: the second pass reads every dependency-gate factor from the drop-in's per-edge-id cache
    # (tm_dropin_gate_cache), the first computes (and fills) them
    for _ in range(2):
        with torch.no_grad():
            i_s, i_t, i_b = ex(w_s, cut, e_s), ex(w_t, cut, e_t), ex(w_b, cut, e_b)
            expl = ex.retrieve_explanation(sg_s, i_s, w_s, sg_t, i_t, w_t, sg_b, i_b, w_b, training=False)
        for k, x in enumerate((i_s, i_t, i_b)):
            assert torch.equal(x[..., 0], imp[k]), k
        assert torch.equal(expl[0], h1.reshape(3 * E, N))
        assert torch.equal(expl[1], h2.reshape(3 * E, N * N))


@pytest.mark.parametrize("where", ["device_pack", "host_pack_grad"])
def test_dropin_device_pack_and_grad_equal_pipeline(dev, finder, g, z, where):
    """The same drop-in calls (a) through a device-resident pack (load_subgraph_margin(..., device=),
    load_edge: get_item hands out device views and the three forward calls overlap on side streams) and
    (b) from the host pack with gradients enabled (eval_one_epoch calls the explainer outside no_grad:
    the eval kernel's output, backward on demand) are bit-identical to the fused pipeline."""
    from tempme_amd import pack as P
    from tempme_amd.pipeline import ExplainPipeline
    N, E = 20, EI.SETS[20]
    ex = _explainer(dev, g, z, "N20_base")
    # the pipeline in reference batches of 25 events (the attention's time std is per batch = per call)
    pipe = ExplainPipeline(ex, finder.graph, torch.from_numpy(z["test_sampler_dst"]), N, 3, 25, seed=0,
                           split=px.SPLIT_TEST)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:E], dtype=dt)).to(dev)  # noqa: E731
    imp, h1, h2 = [x.clone() for x in pipe.run(t(z["test_src"], np.int32), t(z["test_dst"], np.int32),
                                                t(z["test_ts"], np.float64), t(z["test_eidx"], np.int32),
                                                torch.arange(E, dtype=torch.int32, device=dev))]
    _, cat_d, edge = P.buffers_to_arrays(pipe.buf, E)

    class A:
        n_degree = N
    if where == "device_pack":
        pk, ed = P.load_subgraph_margin(A(), cat_d, device=dev), P.load_edge(edge, dev)
    else:
        pk, ed = P.load_subgraph_margin(A(), cat_d), edge
    cut = z["test_ts"][:E].astype(np.float64)
    outs = []
    for b0 in range(0, E, 25):                           # four reference batches, back to back
        idx = np.arange(b0, b0 + 25)
        sg_s, sg_t, sg_b, w_s, w_t, w_b, fake = P.get_item(pk, idx)
        e_s, e_t, e_b = P.get_item_edge(ed, idx)
        i_s, i_t, i_b = ex(w_s, cut[idx], e_s), ex(w_t, cut[idx], e_t), ex(w_b, cut[idx], e_b)
        assert i_s.requires_grad                         # the reference calls the explainer with grad enabled
        with torch.no_grad():
            expl = ex.retrieve_explanation(sg_s, i_s, w_s, sg_t, i_t, w_t, sg_b, i_b, w_b, training=False)
        outs.append((i_s.detach(), i_t.detach(), i_b.detach(), expl))
        if where == "device_pack":
            assert isinstance(fake, torch.Tensor) and fake.device == dev and w_s[0].dtype == torch.int32
    for k in range(3):
        got = torch.cat([o[k] for o in outs])[..., 0]
        assert torch.equal(got, imp[k][:E]), k
    # explanation rows are per side: [src batch | tgt batch | bgd batch] per reference batch
    e1 = torch.cat([o[3][0].view(3, 25, N) for o in outs], 1).reshape(3 * E, N)
    e2 = torch.cat([o[3][1].view(3, 25, N * N) for o in outs], 1).reshape(3 * E, N * N)
    assert torch.equal(e1, h1.reshape(3 * E, N))
    assert torch.equal(e2, h2.reshape(3 * E, N * N))


def _general_inputs(dev, item, edges):
    """get_item / get_item_edge outputs as plain (non-resident) device tensors: the drop-in's general path (per-side
    calls, every parameter an input of its node), the fast paths' reference."""
    def t(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    sgs = [([t(x, torch.int32) for x in sg[0]], [t(x, torch.int32) for x in sg[1]], sg[2]) for sg in item[:3]]
    ws = [(t(w[0], torch.int32), t(w[1], torch.int32), t(w[2], torch.float32), t(w[3], torch.int32), w[4])
          for w in item[3:6]]
    return sgs, ws, [t(e, torch.float32) for e in edges]


def test_dropin_fast_path_gradients_match_general_path(dev, finder, g, z):
    """The drop-in fast path (tm_dropin_forward + tm_edge_importance_gf, parameters behind bundle tensors in the
    autograd nodes) on a device pack and on the reference's host pack (its numpy views staged on the side stream)
    against the general path (plain device tensors: per-side calls, every parameter an input of its node): same
    outputs bit for bit, and the same gradients of a loss over the explanation and the three graphlet
    importances, for every explainer parameter and the importances."""
    from tempme_amd import explainer as X
    from tempme_amd import pack as P
    from tempme_amd.pipeline import ExplainPipeline
    N, E = 20, 50
    ex = _explainer(dev, g, z, "N20_base")
    pipe = ExplainPipeline(ex, finder.graph, torch.from_numpy(z["test_sampler_dst"]), N, 3, 25, seed=0,
                           split=px.SPLIT_TEST)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:E], dtype=dt)).to(dev)  # noqa: E731
    pipe.run(t(z["test_src"], np.int32), t(z["test_dst"], np.int32), t(z["test_ts"], np.float64),
             t(z["test_eidx"], np.int32), torch.arange(E, dtype=torch.int32, device=dev))
    _, cat_d, edge = P.buffers_to_arrays(pipe.buf, E)

    class A:
        n_degree = N
    cut = z["test_ts"][:E].astype(np.float64)
    res = {}
    for where in ("device", "host", "general"):
        pk, ed = ((P.load_subgraph_margin(A(), cat_d, device=dev), P.load_edge(edge, dev)) if where == "device"
                  else (P.load_subgraph_margin(A(), cat_d), edge))
        ex.zero_grad()
        ex.__dict__.pop("_gf_cache", None)
        ex.__dict__.pop("_fastx", None)
        idx = np.arange(25, 50)
        item = P.get_item(pk, idx)
        edges = P.get_item_edge(ed, idx)
        if where == "general":
            (sg_s, sg_t, sg_b), (w_s, w_t, w_b), (e_s, e_t, e_b) = _general_inputs(dev, item, edges)
        else:
            sg_s, sg_t, sg_b, w_s, w_t, w_b, _ = item
            e_s, e_t, e_b = edges
        imps = [ex(w_s, cut[idx], e_s), ex(w_t, cut[idx], e_t), ex(w_b, cut[idx], e_b)]
        for i in imps:
            i.retain_grad()
        expl = ex.retrieve_explanation(sg_s, imps[0], w_s, sg_t, imps[1], w_t, sg_b, imps[2], w_b, training=False)
        assert (where != "general") == bool(ex.__dict__.get("_gf_cache")), "fast path on device / host pack views"
        if where == "device" and X._dropin_ext() is not None:
            # the first forward built the C++ host side; the other calls went through it
            assert ex.__dict__["_fastx"][0].hits == 3
        loss = expl[0].pow(2).sum() + 0.5 * expl[1].sum() + (imps[0] * imps[1]).sum() + imps[2].pow(2).sum()
        loss.backward()
        res[where] = ([x.detach().clone() for x in expl], [i.grad.clone() for i in imps],
                      {n: p.grad.detach().clone() for n, p in ex.named_parameters() if p.grad is not None})
    xg, gg, pg = res["general"]
    for fast in ("device", "host"):
        xf, gf_, pf = res[fast]
        for a_, b_ in zip(xf, xg):
            assert torch.equal(a_, b_), fast
        for a_, b_ in zip(gf_, gg):
            torch.testing.assert_close(a_, b_, rtol=1e-5, atol=1e-7, msg=fast)
        assert pf.keys() == pg.keys() and len(pf) >= 26
        for n in pf:
            torch.testing.assert_close(pf[n], pg[n], rtol=1e-5, atol=1e-7, msg=f"{fast} {n}")


def test_eval_forward_grad_matches_torch(dev, finder, g, z):
    """Eval mode with gradients enabled: the eval kernel's output with the on-demand backward (recompute
    through the training kernels) gives the torch formulation's weight gradients within 2e-4 rel-norm."""
    from tests.encoder_inputs import SIDES  # noqa: F401  (same walk layout)
    ex = _explainer(dev, g, z, "N20_base")
    d = EI.walks(z, 20, 25)
    x = d["src"]
    w = (x["node"], x["eid"], x["ts"], x["cat"], x["marg"])
    ex.zero_grad()
    ex(w, d["ts_cut"], x["cnt"]).pow(2).sum().backward()
    got = {n: p.grad.detach().clone() for n, p in ex.named_parameters() if p.grad is not None}
    ex.zero_grad()
    ex._forward_torch(w, d["ts_cut"], x["cnt"]).pow(2).sum().backward()
    want = {n: p.grad.detach().clone() for n, p in ex.named_parameters() if p.grad is not None}
    assert got.keys() == want.keys() and len(got) == 22
    for n in want:
        err = (got[n] - want[n]).norm() / max(want[n].norm(), 1e-12)
        assert err < 2e-4, (n, float(err))


def _bern_setup(dev, finder, g, z, E=50):
    from tempme_amd import pack as P
    from tempme_amd.pipeline import ExplainPipeline
    N = 20
    ex = _explainer(dev, g, z, "N20_base")
    pipe = ExplainPipeline(ex, finder.graph, torch.from_numpy(z["test_sampler_dst"]), N, 3, 25, seed=0,
                           split=px.SPLIT_TEST)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:E], dtype=dt)).to(dev)  # noqa: E731
    pipe.run(t(z["test_src"], np.int32), t(z["test_dst"], np.int32), t(z["test_ts"], np.float64),
             t(z["test_eidx"], np.int32), torch.arange(E, dtype=torch.int32, device=dev))
    _, cat_d, edge = P.buffers_to_arrays(pipe.buf, E)

    class A:
        n_degree = N
    return ex, P, A, cat_d, edge, z["test_ts"][:E].astype(np.float64)


def test_dropin_bern_fast_path_matches_general_path(dev, finder, g, z):
    """retrieve_explanation(training=True) on the eval-mode module (eval_one_epoch under --if_bern,
    temp_exp_main.py:46, :450-453) through the device-pack fast path (tm_edge_importance_gf3_bern: the
    gathered maxima and the padding mask of the three sides in one launch, one rsample over all of them)
    against the general path (per side: HIP training kernels, rsample, masked_fill).  With beta_sample's
    draw replaced by the identity (the draw is random; everything around it is deterministic): outputs
    bit-identical and the gradients of a loss over them equal for every parameter and importance."""
    from tempme_amd import explainer as X
    ex, P, A, cat_d, edge, cut = _bern_setup(dev, finder, g, z)
    ex.beta_sample = lambda prob, training: prob     # instance attribute: both paths call self.beta_sample
    res = {}
    for where in ("device", "host", "general"):
        pk, ed = ((P.load_subgraph_margin(A(), cat_d, device=dev), P.load_edge(edge, dev)) if where == "device"
                  else (P.load_subgraph_margin(A(), cat_d), edge))
        ex.zero_grad()
        ex.__dict__.pop("_gf_cache", None)
        ex.__dict__.pop("_fastx", None)
        idx = np.arange(25, 50)
        item = P.get_item(pk, idx)
        edges = P.get_item_edge(ed, idx)
        if where == "general":
            (sg_s, sg_t, sg_b), (w_s, w_t, w_b), (e_s, e_t, e_b) = _general_inputs(dev, item, edges)
        else:
            sg_s, sg_t, sg_b, w_s, w_t, w_b, _ = item
            e_s, e_t, e_b = edges
        imps = [ex(w_s, cut[idx], e_s), ex(w_t, cut[idx], e_t), ex(w_b, cut[idx], e_b)]
        for i in imps:
            i.retain_grad()
        expl = ex.retrieve_explanation(sg_s, imps[0], w_s, sg_t, imps[1], w_t, sg_b, imps[2], w_b, training=True)
        assert (where != "general") == bool(ex.__dict__.get("_gf_cache"))
        if where == "device" and X._dropin_ext() is not None:
            assert ex.__dict__["_fastx"][0].hits == 3
        loss = expl[0].pow(2).sum() + 0.5 * expl[1].sum() + (imps[0] * imps[1]).sum()
        loss.backward()
        res[where] = ([x.detach().clone() for x in expl], [i.grad.clone() for i in imps],
                      {n: p.grad.detach().clone() for n, p in ex.named_parameters() if p.grad is not None})
    xg, gg, pg = res["general"]
    for fast in ("device", "host"):
        xf, gf_, pf = res[fast]
        for a_, b_ in zip(xf, xg):
            assert torch.equal(a_, b_), fast
        for a_, b_ in zip(gf_, gg):
            torch.testing.assert_close(a_, b_, rtol=1e-5, atol=1e-7, msg=fast)
        assert pf.keys() == pg.keys() and len(pf) >= 26
        for n in pf:
            torch.testing.assert_close(pf[n], pg[n], rtol=1e-5, atol=1e-7, msg=f"{fast} {n}")


def test_dropin_bern_draws_are_beta(dev, finder, g, z):
    """The fast path's real draws: zero on padding entries, in (0, 1) elsewhere, and over 400 calls their
    per-entry mean and variance match Beta(max(10p,1), max(10(1-p),1)) (explainer_new.py:420-430) with p
    the eval path's maxima (parity for the rsample branch is statistical)."""
    ex, P, A, cat_d, edge, cut = _bern_setup(dev, finder, g, z, E=25)
    pk, ed = P.load_subgraph_margin(A(), cat_d, device=dev), P.load_edge(edge, dev)
    idx = np.arange(25)
    sg_s, sg_t, sg_b, w_s, w_t, w_b, _ = P.get_item(pk, idx)
    e_s, e_t, e_b = P.get_item_edge(ed, idx)
    torch.manual_seed(0)
    with torch.no_grad():
        imps = [ex(w_s, cut[idx], e_s), ex(w_t, cut[idx], e_t), ex(w_b, cut[idx], e_b)]
        draws = [torch.cat([x.reshape(-1) for x in
                            ex.retrieve_explanation(sg_s, imps[0], w_s, sg_t, imps[1], w_t, sg_b, imps[2], w_b,
                                                    training=True)]) for _ in range(400)]
        mean_eval = torch.cat([x.reshape(-1) for x in ex.retrieve_explanation(
            sg_s, imps[0], w_s, sg_t, imps[1], w_t, sg_b, imps[2], w_b, training=False)])
    d = torch.stack(draws).double()
    pad = mean_eval == 0
    assert bool((d[:, pad] == 0).all())
    live = d[:, ~pad]
    assert bool((live > 0).all() and (live < 1).all())
    m = mean_eval[~pad].double()                      # = a / (a + b), the eval branch
    # a + b = max(10p,1) + max(10(1-p),1) >= 10, so var = m(1-m)/(a+b+1) <= 1/44; the 400-draw mean's
    # standard error is <= 0.0075 per entry: check the average deviation and the worst entry loosely
    dev_mean = (live.mean(0) - m).abs()
    assert float(dev_mean.mean()) < 0.004 and float(dev_mean.max()) < 0.05
    # Beta variance m(1-m)/(a+b+1) with a+b+1 in [11, 12]: the pooled ratio lies in [1/12, 1/11] up to noise
    ratio = float(live.var(0).sum() / (m * (1 - m)).sum())
    assert 1 / 12.6 < ratio < 1 / 10.5, ratio


def test_dropin_cpp_host_side_equals_python_host_side(dev, finder, g, z):
    """The C++ host side of the drop-in fast path (csrc/dropin_ext.cpp) against its Python host side (the
    same library calls): four reference batches each way, retrieve_explanation eval and bern (identity
    draw), outputs bit-identical; a weight update between batches sends the next call back through
    Python (new version key) and the results follow the new weights."""
    from tempme_amd import explainer as X
    ex, P, A, cat_d, edge, cut = _bern_setup(dev, finder, g, z, E=100)
    assert X._dropin_ext() is not None, "tempme_amd/lib/_dropin_ext*.so missing (python tempme_amd/_build_ext.py)"
    ex.beta_sample = lambda prob, training: prob
    pk, ed = P.load_subgraph_margin(A(), cat_d, device=dev), P.load_edge(edge, dev)

    def run(force_python):
        outs = []
        for b0 in range(0, 100, 25):
            idx = np.arange(b0, b0 + 25)
            sg_s, sg_t, sg_b, w_s, w_t, w_b, _ = P.get_item(pk, idx)
            e_s, e_t, e_b = P.get_item_edge(ed, idx)
            imps = []
            for w, e in ((w_s, e_s), (w_t, e_t), (w_b, e_b)):
                if force_python:
                    ex.__dict__.pop("_fastx", None)
                imps.append(ex(w, cut[idx], e))
            if force_python:
                ex.__dict__.pop("_fastx", None)
            with torch.no_grad():
                a = ex.retrieve_explanation(sg_s, imps[0], w_s, sg_t, imps[1], w_t, sg_b, imps[2], w_b, training=False)
                b = ex.retrieve_explanation(sg_s, imps[0], w_s, sg_t, imps[1], w_t, sg_b, imps[2], w_b, training=True)
            outs.append([x.detach().clone() for x in imps + a + b])
        return outs

    cpp = run(False)
    assert ex.__dict__["_fastx"][0].hits >= 4 * 4
    py_ = run(True)
    for u, v in zip(cpp, py_):
        for x, y in zip(u, v):
            assert torch.equal(x, y)
    # a weight update: the C++ state's key no longer matches, the call goes through Python and rebuilds it
    with torch.no_grad():
        ex.MLP[0].weight.mul_(1.5)
    upd = run(False)
    assert not torch.equal(upd[0][0], cpp[0][0])
    ex.__dict__.pop("_fastx", None)
    ref = run(True)
    for u, v in zip(upd, ref):
        for x, y in zip(u, v):
            assert torch.equal(x, y)
