"""The explainer's training and evaluation drivers (tempme_amd/train.py, evaluate.py) over a TGAT base.

Yardstick: the eager per-side composition of tests/test_gpu_tgat.py::test_explainer_trains_through_tgat -- three
``TempME.forward`` calls, three ``retrieve_edge_imp_node`` calls, ``TGAT.contrast(test=True, if_explain=True,
exp_weights=[[s, t], [s, b]])``, three ``kl_loss`` calls -- whose parts the TGAT and encoder tests hold to the
reference (the reference's own TGAT explainer class is broken upstream, so the whole step has no golden).

Bounds (the project's own): losses rtol 1e-5 / atol 1e-6 and gradients ||got - want|| <= 2e-4 ||want|| + 1e-9 per
parameter (tests/test_gpu_train.py), logits ``tgat_inputs.logit_atol`` (never below 2e-5).  Where two calls run the
same kernels on the same values (the stacked entry against ``exp_weights`` of its views, ``prepared`` against none,
a reseeded second call) the results are compared bit for bit.
"""
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rank_metrics_ref as RR
import tgat_inputs as TA
import tgn_inputs as TI
from tests.encoder_inputs import SIDES, load as load_enc

pytestmark = pytest.mark.gpu

EX_SEEDS = {"uslegis": 0, "synth": 1}
RATIOS = [0.01, 0.05, 0.1, 0.2, 0.3]
BETA, PRIOR_P = 0.5, 0.3
LOSS_TOL = dict(rtol=1e-5, atol=1e-6)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gold():
    return TA.golden()


def _explainer(base, case, dev, base_type="tgat"):
    from tempme_amd import TempME
    enc = load_enc(case)
    torch.manual_seed(EX_SEEDS[case])
    ex = TempME(base, base_type, "uslegis_sampled", out_dim=40, hid_dim=64, temp=0.07, if_cat_feature=True,
                dropout_p=0.1, device=dev, null_model={k + 1: float(v) for k, v in enumerate(enc["null"])})
    missing, unexpected = ex.load_state_dict(enc["sd"], strict=False)
    assert not unexpected
    return ex.to(dev)


def _batch(case, B=None):
    """The committed 32-event N = 20 batch (its first B events) as a train.Batch of host arrays."""
    from tempme_amd.train import Batch
    enc, d = load_enc(case), TI.load_batch()
    B = d["B"] if B is None else B
    walks = [tuple(enc[s][k][:B] for k in ("node", "eid", "ts", "cat", "marg")) for s in SIDES]
    sgs = [tuple([x[:B] for x in d["sg_" + s][i]] for i in range(3)) for s in SIDES]
    return Batch(d["src"][:B], d["dst"][:B], d["ts_cut"][:B], d["e_idx"][:B], d["fake"][:B], sgs, walks,
                 [enc[s]["cnt"][:B] for s in SIDES])


def _setup(case, dev, B=None):
    base = TA.build_model(case).to(dev)
    ex = _explainer(base, case, dev)
    opt = torch.optim.Adam(ex.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    return base, ex, _batch(case, B), opt


def _contrast_args(b):
    return (b.src, b.dst, b.fake, b.ts, b.e_idx, *b.subgraphs)


def _composition(ex, base, b, training=False):
    """One step's tensors by the eager per-side composition (calls that exist without the drivers)."""
    a = _contrast_args(b)
    with torch.no_grad():
        po, no = base.contrast(*a, test=True, if_explain=False)
        y_ori = torch.where(torch.cat([po, no]).sigmoid() > 0.5, 1., 0.).view(-1, 1)
    gl = [ex(w, b.ts, e) for w, e in zip(b.walks, b.edges)]
    imps = [tuple(ex.retrieve_edge_imp_node(sg, g, w, training=training)) for sg, g, w in zip(b.subgraphs, gl, b.walks)]
    pos, neg = base.contrast(*a, test=True, if_explain=True, exp_weights=[[imps[0], imps[1]], [imps[0], imps[2]]])
    pred_loss = torch.nn.BCEWithLogitsLoss()(torch.cat([pos, neg]), y_ori)
    kl_loss = sum(ex.kl_loss(g, w, target=PRIOR_P) for g, w in zip(gl, b.walks))
    return dict(loss=pred_loss + BETA * kl_loss, pred_loss=pred_loss, kl_loss=kl_loss, pos_logit=pos, neg_logit=neg,
                pos_out_ori=po, neg_out_ori=no, y_ori=y_ori, imps=imps)


def _grads(ex):
    return {k: v.grad.detach().clone() for k, v in ex.named_parameters() if v.grad is not None}


def _assert_grads_close(got, want):
    assert got.keys() == want.keys() and len(want) > 0
    for k in want:
        assert torch.isfinite(got[k]).all() and torch.isfinite(want[k]).all(), k
        d, n = float((got[k].double() - want[k].double()).norm()), float(want[k].double().norm())
        assert d <= 2e-4 * n + 1e-9, (k, d, n)


# ------------------------------------------------------------------ 1. train_step = the composition
@pytest.mark.parametrize("case", TA.CASES)
def test_train_step_equals_composition(dev, gold, case):
    """train_step over a TGAT base (stacked encoder launch, one explain_groups call, the stacked contrast entry,
    the fused KL) = the eager per-side composition: losses, logits, the explainer's gradients; the step moves the
    parameters; the HIP launches are the expected ones (the library's own launch counters)."""
    from tempme_amd import _lib as L
    from tempme_amd.train import train_step
    base, ex, batch, opt = _setup(case, dev)
    base_w, ex_w, batch_w, _ = _setup(case, dev)
    ex.eval(), ex_w.eval()
    p0 = {k: v.detach().clone() for k, v in ex.named_parameters()}
    want = _composition(ex_w, base_w, batch_w)
    want["loss"].backward()
    assert ex._hip_ok()
    L.profile_enable(True)
    try:
        out = train_step(ex, base, opt, batch, beta=BETA, prior_p=PRIOR_P, if_bern=False)
        prof = L.profile_read()
    finally:
        L.profile_enable(False)
    print({k: v[1] for k, v in sorted(prof.items())})
    # the original and the explained contrast: three passes each, one backward per pass; the three sides'
    # explanation as one launch
    assert prof["tgat_attn_fwd_kernel"][1] == 6 and prof["tgat_attn_bwd_kernel"][1] == 3
    assert prof["explain_train_kernel"][1] == 1 and prof["kl_loss_kernel"][1] >= 1 and "gcn_kernel" in prof
    assert base._pack_cache is not None
    for k in ("loss", "pred_loss", "kl_loss"):
        print(case, k, float(out[k]), float(want[k].detach()))
        np.testing.assert_allclose(float(out[k]), float(want[k].detach()), err_msg=k, **LOSS_TOL)
    atol = TA.logit_atol(gold, case)
    for k in ("pos_logit", "neg_logit", "pos_out_ori", "neg_out_ori"):
        d = float((out[k] - want[k].detach()).abs().max())
        print(case, k, "max |diff|", d, "atol", atol)
        assert out[k].shape == (len(batch), 1) and d <= atol, (k, d)
    assert torch.equal(out["y_ori"], want["y_ori"])
    _assert_grads_close(_grads(ex), _grads(ex_w))
    changed = [k for k, v in ex.named_parameters() if v.grad is not None and not torch.equal(v.detach(), p0[k])]
    assert changed
    assert all(p.grad is None for p in base.parameters())
    base.check_errors()


# ------------------------------------------------------------------ 2. the stacked entry = exp_weights
@pytest.mark.parametrize("B", [32, 1])
def test_stacked_entry_equals_exp_weights(dev, B):
    """contrast(stacked_weights=(ew1, ew2)) = contrast(exp_weights=[[s, t], [s, b]]) of the per-side views of the
    same two tensors, bit for bit in the logits and in the gradients reaching the two tensors; contrast(prepared=)
    = contrast without it.  B = 1: one row per segment (seg_rows = 1)."""
    from tempme_amd.train import split_stacked_weights
    case = "uslegis"
    base = TA.build_model(case).to(dev)
    b = _batch(case, B)
    a = _contrast_args(b)
    ew = [w[[r for s in range(3) for r in range(s * 32, s * 32 + B)]].to(dev) for w in TI.explanation(case)]
    res = {}
    for how in ("stacked", "views", "views_prepared"):
        e1, e2 = (w.clone().requires_grad_(True) for w in ew)
        if how == "stacked":
            pos, neg = base.contrast(*a, test=True, if_explain=True, stacked_weights=(e1, e2))
        else:
            kw = {}
            if how == "views_prepared":
                kw["prepared"] = base.prepare_contrast(b.src, b.dst, b.fake, b.ts, *b.subgraphs)
            pos, neg = base.contrast(*a, test=True, if_explain=True, exp_weights=split_stacked_weights(e1, e2), **kw)
        assert pos.shape == neg.shape == (B, 1)
        (pos.sum() + 2.0 * neg.sum()).backward()
        res[how] = (pos.detach(), neg.detach(), e1.grad, e2.grad)
    for how in ("views", "views_prepared"):
        for x, y, what in zip(res["stacked"], res[how], ("pos", "neg", "d hop-1", "d hop-2")):
            assert torch.equal(x, y), (how, what)
    assert float(res["stacked"][2].abs().sum()) > 0 and float(res["stacked"][3].abs().sum()) > 0
    # prepared inputs, shared by the contrast without weights and the one with them
    prep = base.prepare_contrast(b.src, b.dst, b.fake, b.ts, *b.subgraphs)
    with torch.no_grad():
        want_o = base.contrast(*a, test=True, if_explain=False)
        got_o = base.contrast(*a, test=True, if_explain=False, prepared=prep)
        assert prep["cache"].get("pack") is base._pack_cache        # the first two passes' queries are kept
        want_e = base.contrast(*a, test=True, if_explain=True, exp_weights=split_stacked_weights(*ew))
        got_e = base.contrast(*a, test=True, if_explain=True, stacked_weights=tuple(ew), prepared=prep)
    for x, y in zip(want_o + want_e, got_o + got_e):
        assert torch.equal(x, y)
    assert not torch.equal(got_o[0], got_e[0])
    with pytest.raises(ValueError, match="rows"):
        base.contrast(*a, test=True, if_explain=True, stacked_weights=(ew[0][:2 * B], ew[1][:2 * B]))
    base.check_errors()


# ------------------------------------------------------------------ 3. different src weights keep their path
def test_different_src_weights_run_four_segments(dev, gold, monkeypatch):
    case, B = "uslegis", 32
    base = TA.build_model(case).to(dev)
    b = _batch(case)
    a = _contrast_args(b)
    s, t, bg = TA.side_weights(TI.explanation(case), B, dev)
    s2 = tuple(torch.flip(x, dims=(0,)).contiguous() for x in s)          # another src pair
    segs = []
    orig = base.node_embeddings

    def rec(*args, **kw):
        segs.append(kw.get("n_segments"))
        return orig(*args, **kw)
    monkeypatch.setattr(base, "node_embeddings", rec)
    with torch.no_grad():
        pos, neg = base.contrast(*a, test=True, if_explain=True, exp_weights=[[s, t], [s2, bg]])
        assert segs == [4]
        pos_pair, _ = base.contrast(*a, test=True, if_explain=True, exp_weights=[[s, t], [s, bg]])
        _, neg_pair = base.contrast(*a, test=True, if_explain=True, exp_weights=[[s2, t], [s2, bg]])
    assert segs == [4, 3, 3]
    atol = TA.logit_atol(gold, case)
    assert float((pos - pos_pair).abs().max()) <= atol and float((neg - neg_pair).abs().max()) <= atol
    _, neg_same = base.contrast(*a, test=True, if_explain=True, exp_weights=[[s, t], [s, bg]])
    assert float((neg - neg_same).abs().max()) > 10 * atol                 # the second src pair was read


# ------------------------------------------------------------------ 4. if_bern
def test_if_bern_is_reproducible_and_reads_hop2(dev):
    from tempme_amd.evaluate import eval_batch
    from tempme_amd.train import encode_sides, explain_sides, train_step
    case = "uslegis"
    args = SimpleNamespace(test_bs=32, if_bern=True, beta=BETA, prior_p=PRIOR_P, test_threshold=False,
                           base_type="tgat", n_degree=20, ratios=list(RATIOS))
    base, ex, batch, _ = _setup(case, dev)
    ex.eval()
    rows = []
    for _ in range(2):
        torch.manual_seed(77)
        rows.append(eval_batch(args, base, ex, batch, device_metrics=True).cpu().numpy())
    assert rows[0][:8].tobytes() == rows[1][:8].tobytes() and np.isfinite(rows[0][:8]).all()
    torch.manual_seed(78)
    other = eval_batch(args, base, ex, batch, device_metrics=True).cpu().numpy()
    assert other[5] != rows[0][5]                                           # the draws do reach the loss
    # the stochastic training step: two twins from one seed take the same forward
    losses = []
    for _ in range(2):
        base, ex, batch, opt = _setup(case, dev)
        ex.train()
        torch.manual_seed(79)
        out = train_step(ex, base, opt, batch, beta=BETA, prior_p=PRIOR_P, if_bern=True)
        assert all(torch.isfinite(out[k]).all() for k in ("loss", "pos_logit", "neg_logit"))
        g = _grads(ex)
        assert g and all(torch.isfinite(x).all() for x in g.values())
        losses.append(out["loss"].clone())
    assert torch.equal(losses[0], losses[1])
    # hop-2 reaches the base
    ex.eval()
    with torch.no_grad():
        torch.manual_seed(80)
        e1, e2 = explain_sides(ex, batch, encode_sides(ex, batch), True)
        assert e1.shape == (96, 20) and e2.shape == (96, 400) and float(e2.abs().sum()) > 0
        a = _contrast_args(batch)
        pos, neg = base.contrast(*a, test=True, if_explain=True, stacked_weights=(e1, e2))
        pos0, neg0 = base.contrast(*a, test=True, if_explain=True, stacked_weights=(e1, torch.zeros_like(e2)))
    assert torch.isfinite(pos).all() and torch.isfinite(neg).all()
    assert not torch.equal(pos, pos0) and not torch.equal(neg, neg0)


# ------------------------------------------------------------------ a small sampled pack with a TGAT base
def _pack_setup(dev, mode="train", n_head=2):
    import tempme_amd as tm
    from tempme_amd.preprocess import sample_events
    from tempme_amd.tgat import TGAT
    from tempme_amd.workload import enron_like, split
    g = enron_like(n_nodes=80, n_edges=3000, seed=4, node_feat="uniform")
    train = mode == "train"
    (src, dst, ts, eidx), rows, pool = split(g, mode="train") if train else split(g)
    sp = tm.SPLIT_TRAIN if train else tm.SPLIT_TEST
    f = tm.NeighborFinder.from_edges(g["src"][rows], g["dst"][rows], g["eidx"][rows], g["ts"][rows], g["n_nodes"],
                                     device=dev, seed=2, split=sp)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    ev = (to(src, np.int32), to(dst, np.int32), to(ts, np.float64), to(eidx, np.int32))
    buf = sample_events(f.graph, 2, sp, 10, 3, *ev, torch.arange(len(src), dtype=torch.int32, device=dev),
                        to(pool, np.int32))
    torch.manual_seed(3)
    base = TGAT(g["n_feat"], g["e_feat"], 10, num_layers=2, n_head=n_head).to(dev).eval()

    def explainer(dropout_p=0.1):
        torch.manual_seed(5)
        return tm.TempME(base, "tgat", "enron", out_dim=40, hid_dim=64, dropout_p=dropout_p, device=dev,
                         null_model={k: 1.0 / 12 for k in range(1, 13)}).to(dev).eval()
    return buf, ev, base, explainer


def _copy_state(ex_to, opt_to, ex_from, opt_from):
    """Parameters and Adam state of one (explainer, optimizer) pair into its twin."""
    with torch.no_grad():
        for p, q in zip(ex_to.parameters(), ex_from.parameters()):
            p.copy_(q)
    for p, q in zip(ex_to.parameters(), ex_from.parameters()):
        st = opt_from.state.get(q)
        if st:
            opt_to.state[p] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()}


# ------------------------------------------------------------------ 5. the captured step
@pytest.mark.parametrize("overlap_prepare", [False, True])
def test_graphed_step_equals_eager(dev, overlap_prepare):
    """GraphedTrainStep over a TGAT base: two eager warm-up batches, the capture, three replays.  Every replay is
    compared with an eager train_step of a twin that starts from the replay's own initial state (parameters and
    Adam state), so each comparison is one step from identical values: losses and logits within the bounds of the
    module docstring, gradients within 2e-4 relative, and the updated parameters within 5e-3
    (tests/test_gpu_train.py::test_graphed_step_equals_eager's bound: Adam's early steps move a parameter by
    ~lr sign(g), and a near-zero gradient's sign is decided by the summation order of torch's atomic backward)."""
    from tempme_amd.train import GraphedTrainStep, batch_from_pack, train_step
    buf, ev, base, explainer = _pack_setup(dev)
    B = 40
    rows = [torch.arange(k * B, (k + 1) * B, device=dev) for k in range(5)]
    ex, twin = explainer(), explainer()
    opt = torch.optim.Adam(ex.parameters(), lr=1e-3, capturable=True)
    opt_t = torch.optim.Adam(twin.parameters(), lr=1e-3, capturable=True)
    step = GraphedTrainStep(ex, base, opt, buf, *ev, rows[:2], if_bern=False, overlap_prepare=overlap_prepare)
    assert ex._packed_key is None
    for r in rows[2:]:
        _copy_state(twin, opt_t, ex, opt)
        torch.cuda.synchronize()
        out = step(r)
        torch.cuda.synchronize()
        want = train_step(twin, base, opt_t, batch_from_pack(buf, *ev, r), if_bern=False)
        for k in ("loss", "pred_loss", "kl_loss"):
            np.testing.assert_allclose(float(out[k]), float(want[k].detach()), err_msg=k, **LOSS_TOL)
        for k in ("pos_logit", "neg_logit", "pos_out_ori", "neg_out_ori"):
            assert float((out[k] - want[k]).abs().max()) <= 2e-5, k
        assert torch.equal(out["y_ori"], want["y_ori"])
        _assert_grads_close(_grads(ex), _grads(twin))
        for (k, p), q in zip(ex.named_parameters(), twin.parameters()):
            assert float((p.detach() - q.detach()).abs().max()) <= 5e-3, k
    base.check_errors()
    assert int(buf.err.item()) == 0


# ------------------------------------------------------------------ 6. run_steps(overlap=True) = the serial loop
def test_run_steps_overlap_equals_serial(dev, monkeypatch):
    """tests/test_gpu_train.py::test_run_steps_overlap_equals_serial's well-posed form over a TGAT base: every
    prepare_step output is bitwise the serial loop's, and every overlapped step is taken from the serial run's
    parameters, gradients and Adam state (loaded right before the optimizer step)."""
    import tempme_amd.train as T
    buf, ev, base, explainer = _pack_setup(dev)
    B, K = 40, 4
    orig_prep = T.prepare_step

    class Rec:
        def __init__(self, ex, opt, serial=None):
            self.ex, self.opt, self.serial, self.steps = ex, opt, serial, []

        def start(self):
            ps = list(self.ex.parameters())
            cp = lambda v: v.detach().clone() if torch.is_tensor(v) else v  # noqa: E731
            state = [{k: cp(v) for k, v in self.opt.state.get(p, {}).items()} for p in ps]
            self.steps.append(dict(grads=[p.grad.detach().clone() if p.grad is not None else None for p in ps],
                                   params=[p.detach().clone() for p in ps], state=state))

        def finish(self):
            if self.serial is None:
                return
            ref = self.serial[len(self.steps) - 1]
            with torch.no_grad():
                for p, w, gr, st in zip(self.ex.parameters(), ref["params"], ref["grads"], ref["state"]):
                    p.copy_(w)
                    if gr is not None:
                        p.grad.copy_(gr)
                    for k, v in st.items():
                        if torch.is_tensor(v):
                            self.opt.state[p][k].copy_(v)

    runs = []
    for overlap in (False, True):
        preps = []

        def rec_prep(bm, b):
            out = orig_prep(bm, b)
            assert "prepared" in out[0]                         # TGAT's prepared inputs travel with the step
            preps.append(tuple(x.clone() for x in out[1:]))
            return out
        monkeypatch.setattr(T, "prepare_step", rec_prep)
        ex = explainer()
        opt = torch.optim.Adam(ex.parameters(), lr=1e-3)
        rec = Rec(ex, opt, runs[0]["steps"] if overlap else None)
        batches = [T.batch_from_pack(buf, *ev, torch.arange(k * B, (k + 1) * B, device=dev)) for k in range(K)]
        if overlap:
            outs = T.run_steps(ex, base, opt, batches, overlap=True, if_bern=False, grad_sync=rec)
        else:
            outs = [T.train_step(ex, base, opt, b, if_bern=False, grad_sync=rec) for b in batches]
        torch.cuda.synchronize()
        runs.append(dict(losses=[float(o["loss"]) for o in outs], steps=rec.steps, preps=preps))
        monkeypatch.setattr(T, "prepare_step", orig_prep)
    ser, ovl = runs
    assert len(ser["preps"]) == len(ovl["preps"]) == K and len(ser["steps"]) == len(ovl["steps"]) == K
    for k in range(K):
        for a, b in zip(ser["preps"][k], ovl["preps"][k]):
            assert torch.equal(a, b), k
        for a, b in zip(ser["steps"][k]["params"], ovl["steps"][k]["params"]):
            assert torch.equal(a, b), k
        np.testing.assert_allclose(ovl["losses"][k], ser["losses"][k], err_msg=str(k), **LOSS_TOL)
        ga = torch.cat([x.reshape(-1) for x in ser["steps"][k]["grads"] if x is not None])
        gb = torch.cat([x.reshape(-1) for x in ovl["steps"][k]["grads"] if x is not None])
        assert float((ga - gb).norm()) <= 2e-4 * float(ga.norm()) + 1e-9, k


# ------------------------------------------------------------------ 7. eval_batch
def _args(**kw):
    a = dict(test_bs=32, if_bern=False, beta=BETA, prior_p=PRIOR_P, test_threshold=False, base_type="tgat",
             n_degree=20, ratios=list(RATIOS))
    a.update(kw)
    return SimpleNamespace(**a)


def test_eval_batch_equals_composition(dev, gold):
    """eval_batch on the full 32-event uslegis batch (its original logits have both classes, one of 64 above zero,
    the smallest |logit| 0.0094): host and device rows agree, both agree with the figures of the composition's
    logits, and the ratio figures are threshold_test's on the 6-list."""
    from sklearn.metrics import average_precision_score, roc_auc_score

    from tempme_amd import fidelity
    from tempme_amd.evaluate import FIGURES, THRESHOLD_RAN, eval_batch
    from tempme_amd.train import encode_sides, explain_sides, split_stacked_weights
    case = "uslegis"
    base, ex, batch, _ = _setup(case, dev)
    ex.eval()
    host = eval_batch(_args(), base, ex, batch)
    devr = eval_batch(_args(), base, ex, batch, device_metrics=True)
    assert torch.is_tensor(devr) and devr.is_cuda and devr.dtype == torch.float64
    devr = devr.cpu().numpy()
    tol_rank = (2 * 32 + 2 + len(RATIOS)) * RR.EPS          # rank_metrics' bound for 64 scores (test_gpu_rank_metrics)
    for j, k in enumerate(FIGURES[:8]):
        print(k, "host", host[j], "device", devr[j])
        assert np.isfinite(host[j]) and abs(host[j] - devr[j]) <= (tol_rank if j < 2 else 1e-6), k
    assert host[THRESHOLD_RAN] == devr[THRESHOLD_RAN] == 0.0 and np.isnan(host[8:THRESHOLD_RAN]).all()
    # the same figures from the composition's logits
    with torch.no_grad():
        c = _composition(ex, base, batch)
    y = c["y_ori"].cpu().numpy().reshape(-1)
    assert 0 < y.sum() < len(y)
    pos, neg, po, no = (c[k].double().cpu() for k in ("pos_logit", "neg_logit", "pos_out_ori", "neg_out_ori"))
    logit = torch.cat([pos, neg]).numpy().reshape(-1)
    atol = TA.logit_atol(gold, case)
    # AP and AUC are rank statistics of (positive, negative) pairs: they are the same for two sets of logits within
    # atol of each other when no such pair of the yardstick is closer than 2 atol; acc likewise needs |logit| > atol
    gap = np.abs(logit[y > 0.5][:, None] - logit[y < 0.5][None, :]).min()
    print("closest positive/negative logits", gap, "smallest |logit|", np.abs(logit).min(), "atol", atol)
    assert gap > 2 * atol and np.abs(logit).min() > atol
    prob = torch.cat([pos, neg]).float().sigmoid().numpy().reshape(-1)
    want = dict(aps=average_precision_score(y, prob), auc=roc_auc_score(y, prob),
                acc=float(((logit > 0) == (y > 0.5)).mean()),
                fid_prob=float(torch.cat([pos.sigmoid() - po.sigmoid(), no.sigmoid() - neg.sigmoid()]).mean()),
                fid_logit=float(torch.cat([pos - po, no - neg]).mean()), loss=float(c["loss"]),
                pred_loss=float(c["pred_loss"]), kl_loss=float(c["kl_loss"]))
    for row in (host, devr):
        got = dict(zip(FIGURES, row))
        for k in ("aps", "auc"):
            assert abs(got[k] - want[k]) <= tol_rank, (k, got[k], want[k])
        assert got["acc"] == np.float32(want["acc"])
        assert abs(got["fid_logit"] - want["fid_logit"]) <= atol and abs(got["fid_prob"] - want["fid_prob"]) <= atol
        for k in ("loss", "pred_loss", "kl_loss"):
            np.testing.assert_allclose(got[k], want[k], err_msg=k, **LOSS_TOL)
    # threshold_test through eval_batch = threshold_test on the 6-list of views
    args = _args(test_threshold=True)
    host_t = eval_batch(args, base, ex, batch)
    dev_t = eval_batch(args, base, ex, batch, device_metrics=True).cpu().numpy()
    assert host_t[THRESHOLD_RAN] == dev_t[THRESHOLD_RAN] == 1.0
    with torch.no_grad():
        e1, e2 = explain_sides(ex, batch, encode_sides(ex, batch), False)
        six = split_stacked_weights(e1, e2, flat=True)
        ratio = fidelity.threshold_test(args, six, base, *_contrast_args(batch)[:5], c["pos_out_ori"],
                                        c["neg_out_ori"], c["y_ori"], *batch.subgraphs)
    print("ratio figures", host_t[8:THRESHOLD_RAN], dev_t[8:THRESHOLD_RAN], ratio)
    assert np.isfinite(ratio).all()
    for j in range(5):
        tol = tol_rank if j < 2 else 1e-6
        assert abs(host_t[8 + j] - ratio[j]) <= (0.0 if j >= 2 else tol_rank), j
        assert abs(dev_t[8 + j] - ratio[j]) <= tol, j
    base.check_errors()


# ------------------------------------------------------------------ 8. eval_one_epoch
def test_eval_one_epoch_equals_batch_rows(dev):
    from tempme_amd.evaluate import FIGURES, eval_batch, eval_one_epoch, eval_spans
    from tempme_amd.train import batch_from_pack, prepare_step
    buf, ev, base, explainer = _pack_setup(dev, mode="test")
    ex = explainer()
    ev = tuple(x[:161] for x in ev)                                  # three batches of 40
    args = _args(test_bs=40, n_degree=10, test_threshold=True)
    spans = eval_spans(160, 40)
    assert len(spans) == 3
    batch = lambda s, e: batch_from_pack(buf, *ev, torch.arange(s, e, dtype=torch.int64, device=dev))  # noqa: E731
    ori = torch.cat([torch.cat(prepare_step(base, batch(s, e))[1:3]) for _, s, e in spans])
    with torch.no_grad():                                            # both classes in every batch
        base.affinity_score.fc2.bias -= ori.median()
    for _, s, e in spans:
        y = prepare_step(base, batch(s, e))[3]
        assert 0 < float(y.sum()) < y.numel()
    for device_metrics in (False, True):
        rows = []
        for _, s, e in spans:
            r = eval_batch(args, base, ex, batch(s, e), device_metrics=device_metrics)
            rows.append(r.cpu().numpy() if torch.is_tensor(r) else r)
        rows = np.stack(rows)
        got = eval_one_epoch(args, base, ex, buf, *ev, device_metrics=device_metrics)
        assert got["n_batches"] == 3
        want = rows[:, :len(FIGURES)].mean(axis=0)
        assert np.isfinite(want).all()
        np.testing.assert_allclose([got[k] for k in FIGURES], want, rtol=0, atol=1e-6, equal_nan=False)
    base.check_errors()


# ------------------------------------------------------------------ 9. two ranks
WORLD = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _train_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        from tempme_amd.train import GradAllReduce, batch_from_pack, train_epoch, train_step
        buf, ev, base, explainer = _pack_setup(dev)
        B = 40
        batch = lambda k: batch_from_pack(buf, *ev, torch.arange(k * B, (k + 1) * B, device=dev))  # noqa: E731

        def grads(ex):
            return [p.grad.detach().clone() if p.grad is not None else None for p in ex.parameters()]

        class Rec(GradAllReduce):
            def finish(self):
                super().finish()
                self.synced = grads(self.module)

        # one deterministic step per rank on its own batch: the all-reduced gradients
        ex = explainer()
        opt = torch.optim.Adam(ex.parameters(), lr=1e-3)
        sync = Rec(ex)
        train_step(ex, base, opt, batch(rank), if_bern=False, grad_sync=sync)
        synced = sync.synced
        # then one epoch over 161 events (four whole batches of 40, two per rank), stochastic as train_epoch runs it
        short = tuple(x[:161] for x in ev)
        outs = train_epoch(ex, base, opt, buf, *short, B, generator=torch.Generator().manual_seed(9), if_bern=True,
                           grad_sync=GradAllReduce(ex), rank=rank, world=world)
        assert len(outs) == 2 and all(torch.isfinite(o["loss"]).item() for o in outs)
        params = [None] * world
        dist.all_gather_object(params, [p.detach().cpu() for p in ex.parameters()])
        if rank == 0:
            for a, b in zip(params[0], params[1]):
                assert torch.equal(a, b)                    # replicas identical after the all-reduced steps
            # the first step = one process's average of the two batches' gradients from the same parameters
            ex1 = explainer()

            class NoStep:
                def zero_grad(self):
                    ex1.zero_grad()

                def step(self):
                    pass
            ref = []
            for k in range(world):
                train_step(ex1, base, NoStep(), batch(k), if_bern=False)
                ref.append(grads(ex1))
            n = 0
            for i, s in enumerate(synced):
                if s is None:
                    continue
                avg = sum(r[i] for r in ref) / world
                assert float((s - avg).norm()) <= 2e-4 * float(avg.norm()) + 1e-9, i
                n += 1
            assert n > 0
            base.check_errors()
            q.put("ok")
        dist.barrier()
    except Exception as exc:
        q.put(repr(exc))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_train_epoch_keeps_replicas_identical():
    """Two spawned ranks on cuda:0 (gloo, as tests/test_gpu_multi_rank.py): GradAllReduce over a TGAT base's step
    gives one process's average of the two batches' gradients, and train_epoch leaves both ranks with identical
    parameters."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_train_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        res = q.get(timeout=240)
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    assert res == "ok", res
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


# ------------------------------------------------------------------ 10. mismatch
def test_base_type_mismatch_raises(dev):
    from tempme_amd.evaluate import eval_batch
    from tempme_amd.train import train_step
    case = "uslegis"
    batch = _batch(case, 4)
    tgat = TA.build_model(case).to(dev)
    tgn = TI.build_model(case).to(dev)
    for base, base_type in ((tgat, "tgn"), (tgn, "tgat"), (tgat, "graphmixer")):
        ex = _explainer(base, case, dev, base_type).eval()
        opt = torch.optim.Adam(ex.parameters(), lr=1e-3)
        with pytest.raises(ValueError, match=f"(?s){base_type}.*{type(base).__name__}"):
            train_step(ex, base, opt, batch, if_bern=False)
        with pytest.raises(ValueError, match=f"(?s){base_type}.*{type(base).__name__}"):
            eval_batch(_args(base_type=base_type), base, ex, batch)
