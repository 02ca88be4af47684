"""GPU parity of the base-TGAT consumer: TGAT.contrast with per-side explanation weights, its
explanation-weight gradient, threshold_test's tgat branch and the composition with TempME, through the C
ABI (tm_tgat_attn_fwd / _bwd, tm_tgat_merge_fwd, tm_mask_least_important), against the reference's outputs
(tests/golden/tgat_uslegis.npz) and an fp64 restatement of the kernels (tests/tgat_ref.py).

Logit tolerance: the TGN test's rule, atol 10 x the reference's own fp32-vs-fp64 envelope + rtol 1e-5.  The
committed envelope is 2.2e-6 for uslegis (above the 2e-6 behind TGN's 2e-5), so its atol scales to 2.2e-5;
synth (1.5e-6) keeps 2e-5 (tgat_inputs.logit_atol, test_tgat_cpu.test_reference_fp32_envelope).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tgat_inputs as TA
import tgat_ref as R
import tgn_inputs as TI

pytestmark = pytest.mark.gpu

RTOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gold():
    return TA.golden()


@pytest.fixture(scope="module")
def batch():
    return TI.load_batch()


def _logits(m, d, w=None):
    p, n = TA.contrast(m, d, w)
    assert p.shape == n.shape == (d["B"], 1)
    return torch.cat([p, n]).detach().cpu().numpy()


# ------------------------------------------------------------------ 1. contrast parity
@pytest.mark.parametrize("case", TA.CASES)
def test_contrast_matches_reference(dev, gold, batch, case):
    m = TA.build_model(case)
    if case == "uslegis":
        m = m.to(dev)                                   # synth: host-resident parameters work too
    B = batch["B"]
    atol = TA.logit_atol(gold, case)
    with torch.no_grad():
        for tag, w in (("ori", None), ("expl", TI.explanation(case)), ("rand", TI.rand_weights(case))):
            out = _logits(m, batch, None if w is None else TA.side_weights(w, B, dev))
            err = np.abs(out - gold[f"{case}_{tag}"]).max()
            print(case, tag, "max |logit - reference|", err, "atol", atol)
            np.testing.assert_allclose(out, gold[f"{case}_{tag}"], atol=atol, rtol=RTOL, err_msg=tag)
    m.check_errors()


def test_src_weights_given_twice_run_twice(dev, gold, batch):
    """Pairs with different src weight objects compute the src side per pair, as the reference does; equal
    values then give the single-src result."""
    m = TA.build_model("synth").to(dev)
    B = batch["B"]
    w = TA.side_weights(TI.rand_weights("synth"), B, dev)
    a = (batch["src"], batch["dst"], batch["fake"], batch["ts_cut"], batch["e_idx"], batch["sg_src"], batch["sg_tgt"],
         batch["sg_bgd"])
    with torch.no_grad():
        one = torch.cat(m.contrast(*a, test=True, if_explain=True, exp_weights=[[w[0], w[1]], [w[0], w[2]]]))
        w0b = tuple(x.clone() for x in w[0])
        two = torch.cat(m.contrast(*a, test=True, if_explain=True, exp_weights=[[w[0], w[1]], [w0b, w[2]]]))
        ones = tuple(torch.ones_like(x) for x in w[0])
        other = torch.cat(m.contrast(*a, test=True, if_explain=True, exp_weights=[[w[0], w[1]], [ones, w[2]]]))
    assert torch.equal(one, two)
    assert torch.equal(one[:B], other[:B]) and (one[B:] - other[B:]).abs().max() > 1e-3


# ------------------------------------------------------------------ 2. explanation-weight gradient
@pytest.mark.parametrize("case", TA.CASES)
def test_explanation_weight_gradient(dev, gold, batch, case):
    """d (pos.sum() + neg.sum()) / d the six explanation tensors against the reference model evaluated in
    fp64.  Tolerance per hop: 10 x the reference's own fp32-vs-fp64 gradient distance at that hop (max over
    the three sides) from the fixture: uslegis hop-1 1.1e-5 -> 1.1e-4, hop-2 9.2e-7 -> 9.2e-6; synth hop-1
    3.0e-7 -> 3.0e-6, hop-2 7.9e-9 -> 7.9e-8 (gradient scales: 2.3 / 0.59 and 0.65 / 0.0098).
    The hop-1 gradient carries pass 1 and pass 3: detaching pass 3's weights changes it."""
    m = TA.build_model(case).to(dev)
    B = batch["B"]
    w = TA.side_weights(TI.explanation(case), B, dev, grad=True)
    pos, neg = TA.contrast(m, batch, w)
    (pos.sum() + neg.sum()).backward()
    assert all(p.grad is None for p in m.parameters())                # the base model is frozen
    for h in (0, 1):
        tol = 10 * max(float(np.abs(gold[f"{case}_grad32_{s}{h}"] - gold[f"{case}_grad64_{s}{h}"]).max())
                       for s in TA.SIDES)
        for si, s in enumerate(TA.SIDES):
            got, ref = w[si][h].grad.cpu().numpy(), gold[f"{case}_grad64_{s}{h}"]
            print(case, s, "hop", h + 1, "max |grad - fp64 reference|", np.abs(got - ref).max(), "tol", tol)
        for si, s in enumerate(TA.SIDES):
            np.testing.assert_allclose(w[si][h].grad.cpu().numpy(), gold[f"{case}_grad64_{s}{h}"], atol=tol, rtol=0,
                                       err_msg=f"{s}{h}")
    # pass 3's weights detached: hop-1 loses its second contribution
    w2 = TA.side_weights(TI.explanation(case), B, dev, grad=True)
    orig = m._attn_pass

    def detached(pk, mi, *a):
        a = list(a)
        if mi == 1:
            a[9] = a[9].detach()            # ew of _attn_pass(pk, mi, src, src_t, R, N, node_idx, ngh_dense, ...)
        return orig(pk, mi, *a)
    m._attn_pass = detached
    pos, neg = TA.contrast(m, batch, w2)
    (pos.sum() + neg.sum()).backward()
    m._attn_pass = orig
    for si in range(3):
        assert (w2[si][0].grad - w[si][0].grad).abs().max() > 1e-3 * w[si][0].grad.abs().max()


# ------------------------------------------------------------------ 3. attention kernels through the C ABI
def _attn_case(dev, dims, N, H, seed):
    from tempme_amd import _lib as L
    dn, de, dtm = dims
    dk, Rr = dn + de + dtm, 7
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen, dtype=torch.float64) * scale).float()
    x = SimpleNamespace(R=Rr, N=N, H=H, dk=dk, dims=dims, T=float(np.sqrt(dk / 1.0)))
    x.node, x.edge = rnd(Rr, N, dn), rnd(Rr, N, de)
    x.dt = torch.rand(Rr, N, generator=gen).float() * 50.0
    x.tw = (1.0 / 10 ** torch.linspace(0, 4, dtm)).float()
    x.tb = rnd(dtm, scale=0.5)
    x.qf = rnd(Rr, H, dk)
    x.mask = torch.randint(1, 9, (Rr, N), generator=gen, dtype=torch.int32)
    x.mask[0, 0] = 0
    x.mask[3] = 0                                               # one fully masked row
    x.mask[5, N - 1] = 0
    x.ew = torch.rand(Rr, N, generator=gen).float()
    x.ew[2, 1] = 0.0
    x.gz = rnd(Rr, H, dk)
    x.L = L
    return x


def _desc(x, dev, t, node_idx=None, node_tab=None, node_rows=0, err=None):
    a = x.L.TgatAttn()
    a.rows, a.n_ngh, a.n_head = x.R, x.N, x.H
    a.d_node, a.d_edge, a.d_time = x.dims
    a.node_rows, a.edge_rows, a.head_major_rows, a.seg_rows = node_rows, 0, 1, 0
    a.temperature = x.T
    a.node_tab = (node_tab if node_tab is not None else t["node"]).data_ptr()
    a.node_idx = node_idx.data_ptr() if node_idx is not None else None
    a.edge_tab, a.edge_idx = t["edge"].data_ptr(), None
    a.dt, a.time_w, a.time_b = t["dt"].data_ptr(), t["tw"].data_ptr(), t["tb"].data_ptr()
    a.mask_node, a.ew, a.qf = t["mask"].data_ptr(), t["ew"].data_ptr(), t["qf"].data_ptr()
    a.err_flag = err.data_ptr() if err is not None else None
    return a


def _tol(ref):
    """fp32 unit roundoff 6e-8 times the longest chain of a result (d_key <= 65 products and a 64-lane
    butterfly per score, <= 5 softmax terms, the hardware cosine's 1.8e-7 per time feature) stays below
    1e-5 of the largest element of the tensor compared (at least 1)."""
    return 1e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("dims", [(5, 3, 5), (30, 5, 30)])
def test_attention_kernels_match_fp64(dev, dims, N, H):
    x = _attn_case(dev, dims, N, H, seed=100 * N + H + dims[0])
    L = x.L
    t = {k: getattr(x, k).to(dev).contiguous() for k in ("node", "edge", "dt", "tw", "tb", "qf", "mask", "ew", "gz")}
    st = L.stream_ptr(dev)
    # fp64 restatement, with autograd for the three gradients
    node64 = x.node.double().requires_grad_(True)
    ew64 = x.ew.double().requires_grad_(True)
    qf64 = x.qf.double().requires_grad_(True)
    key = R.keys(node64, x.edge, x.dt, x.tw, x.tb)
    z_ref = R.attn(qf64, key, x.mask, ew64, x.T)
    (z_ref * x.gz.double()).sum().backward()
    # dense node table: forward and backward
    z = torch.empty(x.R, x.H * x.dk, device=dev)
    stats = torch.empty(x.R, x.H, 2, device=dev)
    a = _desc(x, dev, t)
    L.check(L.lib().tm_tgat_attn_fwd(C.byref(a), L.ptr(z), L.ptr(stats), st))
    parts = torch.full((x.R * x.H, x.N), float("nan"), device=dev)
    d_node = torch.full((x.R * x.N, dims[0]), float("nan"), device=dev)
    d_qf = torch.full((x.R, x.H * x.dk), float("nan"), device=dev)
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(stats), L.ptr(t["gz"]), L.ptr(parts), L.ptr(d_node),
                                     L.ptr(d_qf), st))
    d_ew = parts.view(x.H, x.R, x.N).sum(0)                     # pair q = r H + h -> weight row q % rows
    for name, got, ref in (("z", z.view(x.R, x.H, x.dk), z_ref.detach()), ("d_ew", d_ew, ew64.grad),
                           ("d_node", d_node.view(x.R, x.N, -1), node64.grad),
                           ("d_qf", d_qf.view(x.R, x.H, x.dk), qf64.grad)):
        err = (got.cpu().double() - ref).abs().max().item()
        print(dims, N, H, name, "max err", err, "tol", _tol(ref))
        assert torch.isfinite(got).all(), name
        assert err <= _tol(ref), name
    # the masked row's scores are constants: no gradient reaches its query through them
    m_rows = R.pair_rows(x.R, x.H, True)
    full = (x.mask[m_rows] == 0).all(-1)                        # [R, H] pairs whose mask row is all padding
    assert full.any() and d_qf.view(x.R, x.H, x.dk).cpu()[full].abs().max() == 0
    # each nullable output alone gives the same values
    p2 = torch.empty_like(parts)
    q2 = torch.empty_like(d_qf)
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(stats), L.ptr(t["gz"]), L.ptr(p2), None, L.ptr(q2), st))
    assert torch.equal(p2, parts) and torch.equal(q2, d_qf)
    n2 = torch.empty_like(d_node)
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(stats), L.ptr(t["gz"]), L.ptr(p2), L.ptr(n2), None, st))
    assert torch.equal(n2, d_node)
    # gathered node table with one out-of-range id: the flag is set, the slot reads row 0, nothing faults
    rows_tab = x.R * x.N
    idx = torch.arange(rows_tab, dtype=torch.int32)
    idx[4] = rows_tab + 3
    tab = x.node.reshape(rows_tab, -1).clone()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    b = _desc(x, dev, t, node_idx=idx.to(dev), node_tab=tab.to(dev), node_rows=rows_tab, err=err)
    z2 = torch.empty_like(z)
    L.check(L.lib().tm_tgat_attn_fwd(C.byref(b), L.ptr(z2), L.ptr(stats), st))
    assert int(err.item()) == L.TM_E_ARG
    node_fix = x.node.clone().reshape(rows_tab, -1)
    node_fix[4] = node_fix[0]
    z_fix = R.attn(x.qf.double(), R.keys(node_fix.view(x.R, x.N, -1), x.edge, x.dt, x.tw, x.tb), x.mask,
                   x.ew.double(), x.T)
    assert (z2.view(x.R, x.H, x.dk).cpu().double() - z_fix).abs().max().item() <= _tol(z_fix)


def test_attention_limits_are_refused(dev):
    from tempme_amd import _lib as L
    x = _attn_case(dev, (5, 3, 5), 3, 1, seed=1)
    t = {k: getattr(x, k).to(dev).contiguous() for k in ("node", "edge", "dt", "tw", "tb", "qf", "mask", "ew", "gz")}
    z = torch.empty(8, device=dev)
    for change in (dict(n_head=5), dict(d_node=300, d_time=300)):
        a = _desc(x, dev, t)
        for k, v in change.items():
            setattr(a, k, v)
        assert L.lib().tm_tgat_attn_fwd(C.byref(a), L.ptr(z), L.ptr(z), L.stream_ptr(dev)) == L.TM_E_UNSUPPORTED
        assert L.lib().tm_last_error()


# ------------------------------------------------------------------ 4. the fused tail
def _tail_weights(dk, feat, H, gen):
    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen, dtype=torch.float64) * scale
    K1 = H * dk
    return dict(G=rnd(dk, K1, scale=K1 ** -0.5), fcb=rnd(dk, scale=0.1), lnw=1 + rnd(dk, scale=0.1),
                lnb=rnd(dk, scale=0.1), w11=rnd(feat, dk, scale=dk ** -0.5), b11=rnd(feat, scale=0.1),
                w12=rnd(feat, feat, scale=feat ** -0.5), b12=rnd(feat, scale=0.1),
                w21=rnd(feat, feat, scale=feat ** -0.5), b21=rnd(feat, scale=0.1),
                w22=rnd(feat, feat, scale=feat ** -0.5), b22=rnd(feat, scale=0.1))


# feat is the leading block of d_key (src = query[:, :feat]), so feat <= d_key: (13, 172) and (65, 172) do not exist
TAIL_DIMS = [(13, 5, 2), (65, 5, 2), (345, 5, 3), (345, 172, 3)]


@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("dk,feat,H", TAIL_DIMS)
def test_fused_tail_matches_fp64(dev, rows, dk, feat, H):
    """tm_tgat_merge_fwd against the torch tail in fp64.  Tolerance: 10 x the distance of the same tail in
    torch fp32 on the CPU from that fp64 result (the rule of the logit tests), at least 1e-6."""
    from tempme_amd import tgat as T
    gen = torch.Generator().manual_seed(rows * 1000 + dk + feat)
    w = _tail_weights(dk, feat, H, gen)
    z = torch.randn(rows, H * dk, generator=gen, dtype=torch.float64).float()
    query = torch.randn(rows, dk, generator=gen, dtype=torch.float64).float()
    w32 = {k: v.float() for k, v in w.items()}
    ref = R.tail(z.double(), query.double(), {k: v.double() for k, v in w32.items()}, feat)
    cpu32 = R.tail(z, query, w32, feat)
    tol = max(10 * (cpu32.double() - ref).abs().max().item(), 1e-6)
    lw = dict(H=H, Gt=w32["G"].t().contiguous().to(dev), fcb=w32["fcb"].to(dev), lnw=w32["lnw"].to(dev),
              lnb=w32["lnb"].to(dev))
    for k in ("11", "12", "21", "22"):
        lw[f"w{k}t"] = w32[f"w{k}"].t().contiguous().to(dev)
        lw[f"b{k}"] = w32[f"b{k}"].to(dev)
    out = T.merge_fwd(z.to(dev), query.to(dev), lw, feat)
    torch_tail = T.merge_torch(z.to(dev), query.to(dev), lw, feat)
    err = (out.cpu().double() - ref).abs().max().item()
    print(rows, dk, feat, "fused max err", err, "tol", tol, "torch-op tail err",
          (torch_tail.cpu().double() - ref).abs().max().item())
    assert out.shape == (rows, feat) and torch.isfinite(out).all()
    assert err <= tol


def test_fused_tail_refuses_what_it_cannot_hold(dev):
    from tempme_amd import _lib as L
    m = L.TgatMerge()
    m.rows, m.n_head, m.d_key, m.feat = 4, 2, 600, 5
    assert L.lib().tm_tgat_merge_fwd(C.byref(m), None, L.stream_ptr(dev)) == L.TM_E_UNSUPPORTED
    m.d_key, m.feat = 512, 512
    assert L.lib().tm_tgat_merge_fwd(C.byref(m), None, L.stream_ptr(dev)) == L.TM_E_UNSUPPORTED


def test_fused_tail_equals_torch_tail_in_contrast(dev, gold, batch):
    """With fused_tail on, the no-grad contrast (fused tail) equals the grad-enabled contrast (torch tail)
    within the logit tolerance, and the fused kernel really ran."""
    from tempme_amd import _lib as L
    case = "uslegis"
    m = TA.build_model(case).to(dev)
    assert m.fused_tail is False                     # the torch-op tail is the default (it measured faster)
    m.fused_tail = True
    B = batch["B"]
    ew = TI.explanation(case)
    L.profile_enable(True)
    with torch.no_grad():
        fused = _logits(m, batch, TA.side_weights(ew, B, dev))
    names = L.profile_read()
    L.profile_enable(False)
    assert names["tgat_merge_fwd_kernel"][1] == 3 and names["tgat_attn_fwd_kernel"][1] == 3
    w = TA.side_weights(ew, B, dev, grad=True)
    pos, neg = TA.contrast(m, batch, w)
    assert pos.requires_grad
    torch_tail = torch.cat([pos, neg]).detach().cpu().numpy()
    np.testing.assert_allclose(fused, torch_tail, atol=TA.logit_atol(gold, case), rtol=RTOL)
    m.fused_tail = False
    with torch.no_grad():
        off = _logits(m, batch, TA.side_weights(ew, B, dev))
    np.testing.assert_array_equal(off, torch_tail)


# ------------------------------------------------------------------ 5. pairing
def test_head_major_pairing_matters(dev, batch):
    m = TA.build_model("synth").to(dev)
    w = TA.side_weights(TI.rand_weights("synth"), batch["B"], dev)
    with torch.no_grad():
        a = _logits(m, batch, w)
        m.head_major_rows = False
        b = _logits(m, batch, w)
    assert np.abs(a - b).max() > 1e-3


# ------------------------------------------------------------------ 6. fidelity
@pytest.mark.parametrize("case", TA.CASES)
def test_threshold_test_matches_reference(dev, gold, batch, case):
    from tempme_amd import fidelity
    g, d = gold, batch
    B, N = d["B"], d["N"]
    ne = N + N * N
    ratios = list(g["ratios"])
    G = len(ratios)
    m = TA.build_model(case).to(dev)
    expl = TI.explanation(case)
    six = [w.to(dev) for s in range(3) for w in (expl[0][s * B:(s + 1) * B], expl[1][s * B:(s + 1) * B])]
    sgs = (d["sg_src"], d["sg_tgt"], d["sg_bgd"])
    stacked = [torch.cat(six[0::2]), torch.cat(six[1::2])]
    masked = fidelity._masked_nodes(stacked, sgs, N, ratios, dev).cpu().numpy()
    bits = np.unpackbits(g[f"{case}_thr_zero_bits"])[:G * 3 * B * ne].reshape(G, 3 * B, ne).astype(bool)
    assert np.array_equal(masked == 0, bits)                  # bit-exact, tie order included
    pos, neg = fidelity.masked_contrast_tgat(m, six, d["src"], d["dst"], d["fake"], d["ts_cut"], *sgs, N, ratios)
    got = torch.cat([pos, neg], dim=1).detach().cpu().numpy()
    np.testing.assert_allclose(got, g[f"{case}_thr_logits"].reshape(G, 2 * B), atol=TA.logit_atol(g, case), rtol=RTOL)
    ori = torch.from_numpy(g[f"{case}_ori"]).to(dev)
    pos_o, neg_o = ori[:B], ori[B:]
    y_ori = torch.where(ori.sigmoid() > 0.5, 1., 0.).view(-1, 1)
    args = SimpleNamespace(ratios=ratios, base_type="tgat", n_degree=N, bs=B)
    metrics = fidelity.threshold_test(args, six, m, d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], pos_o,
                                      neg_o, y_ori, *sgs)
    np.testing.assert_allclose(metrics, g[f"{case}_thr_metrics"], atol=2e-5, rtol=0)
    m.check_errors()


# ------------------------------------------------------------------ 7. composition with the explainer
def test_explainer_trains_through_tgat(dev, batch):
    """TempME(base=TGAT, "tgat") -> retrieve_edge_imp_node per side -> contrast(if_explain=True) -> backward:
    finite, non-zero gradients on the explainer's parameters; the logits equal those of the same weights
    fed in detached."""
    from tempme_amd import TempME
    from tests.encoder_inputs import load as load_enc
    case, B = "uslegis", 8
    base = TA.build_model(case).to(dev)
    enc = load_enc(case)
    torch.manual_seed(0)
    ex = TempME(base, "tgat", "uslegis_sampled", out_dim=40, hid_dim=64, device=dev,
                null_model={k + 1: float(v) for k, v in enumerate(enc["null"])})
    ex.load_state_dict(enc["sd"], strict=False)
    ex = ex.to(dev).eval()
    d = batch
    cut = d["ts_cut"][:B]
    imps = []
    for s in TA.SIDES:
        e = enc[s]
        walks = tuple(e[k][:B] for k in ("node", "eid", "ts", "cat", "marg"))
        sub = tuple([x[:B] for x in d["sg_" + s][i]] for i in range(3))
        graphlet = ex(walks, cut, e["cnt"][:B])
        imps.append(tuple(ex.retrieve_edge_imp_node(sub, graphlet, walks, training=False)))
    assert all(t.requires_grad for pair in imps for t in pair)
    sgs = [tuple([x[:B] for x in d["sg_" + s][i]] for i in range(3)) for s in TA.SIDES]
    a = (d["src"][:B], d["dst"][:B], d["fake"][:B], cut, d["e_idx"][:B], *sgs)
    pos, neg = base.contrast(*a, test=True, if_explain=True, exp_weights=[[imps[0], imps[1]], [imps[0], imps[2]]])
    assert pos.shape == neg.shape == (B, 1)
    (pos.sum() + neg.sum()).backward()
    grads = [p.grad for p in ex.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)
    assert sum(float(x.abs().sum()) for x in grads) > 0
    det = [tuple(t.detach() for t in pair) for pair in imps]
    with torch.no_grad():
        pos_d, neg_d = base.contrast(*a, test=True, if_explain=True, exp_weights=[[det[0], det[1]], [det[0], det[2]]])
    np.testing.assert_allclose(torch.cat([pos, neg]).detach().cpu().numpy(), torch.cat([pos_d, neg_d]).cpu().numpy(),
                               atol=2e-5, rtol=RTOL)
    base.check_errors()
