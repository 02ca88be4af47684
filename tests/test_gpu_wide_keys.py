"""Attention keys wider than 512 floats (Wikipedia / Reddit: 172 + 172 + 172 = 516): the ninth key register of
the TGN and TGAT attention kernels and the 9-tile instance of the fused TGAT tail, through the C ABI and through the
models.  d_key <= 576 = 9 x 64; TGN base *training* stays at 512 (tests/test_gpu_tgn_train.py pins 516 as refused).

Register 8 of a lane carries key columns 512..575.  The key layouts put each kind of column there:
  (172, 172, 172) = 516  four live lanes, the time segment alone in the register
  (171, 171, 171) = 513  one live lane
  (192, 192, 192) = 576  every lane live
  (520, 3, 5)     = 528  node columns in register 8: d_node is written from it
  (300, 215, 5)   = 520  the edge-to-time boundary inside register 8
with N in {3, 5} (one wave per row / the split forward) and H in {2, 3} (the 2-head and the 4-head instances).
Every kernel output lies between guard floats, so a store past d_key shows as a failed assertion.

Tolerances are the existing files' own.  Kernel outputs: 1e-5 max(1, max |ref|) (test_gpu_tgat._tol, applied there
at d_key = 512; a 516- or 576-long dot product adds at most 12 % to the chain it was derived for).  Fused tail:
10 x the CPU fp32 tail's distance from fp64, at least 1e-6 (test_fused_tail_matches_fp64).  TGN logits: atol 2e-5,
rtol 1e-5 against the fp64 oracle (test_gpu_tgn; the oracle's own fp32 run sits 9.1e-7, 1.07e-6 and 5.7e-7 from
fp64 on the three cases, seeds 3, 4, 5, so the bound is about 19 x the reference's envelope).  TGAT logits and
parameter gradients: test_gpu_tgat_train's rules on each case's own fp32 / fp64 pair.
"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_tgat as TG
import test_gpu_tgat_train as TGT
import test_gpu_tgn as TN
import test_gpu_tgn_train as TNT
import tgat_ref as R
import tgn_inputs as TI
import tgn_train_inputs as TT
import tgn_train_ref as TR
from oracle import tgn_ref as O

pytestmark = pytest.mark.gpu

LAYOUTS = [(172, 172, 172), (171, 171, 171), (192, 192, 192), (520, 3, 5), (300, 215, 5)]
ROWS = 7
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


def lid(d):
    return "x".join(str(v) for v in d)


def _guarded_set(dev, shapes):
    bufs, views = {}, SimpleNamespace()
    for name, shape in shapes:
        bufs[name], view = TGT.guarded(dev, *shape)
        setattr(views, name, view)
    return bufs, views


def _close(tag, name, got, ref):
    err = (got.cpu().double() - ref).abs().max().item()
    tol = TG._tol(ref)
    print(tag, name, "max err", err, "tol", tol)
    assert torch.isfinite(got).all(), name
    assert err <= tol, name


# ------------------------------------------------------------------ 1. TGAT plain pair
@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("dims", LAYOUTS, ids=lid)
def test_tgat_plain_pair_matches_fp64(dev, dims, N, H):
    x = TG._attn_case(dev, dims, N, H, seed=100 * N + H + dims[0])
    assert x.R == ROWS and x.dk > 512
    L = x.L
    t = {k: getattr(x, k).to(dev).contiguous() for k in ("node", "edge", "dt", "tw", "tb", "qf", "mask", "ew", "gz")}
    st = L.stream_ptr(dev)
    node64 = x.node.double().requires_grad_(True)
    ew64 = x.ew.double().requires_grad_(True)
    qf64 = x.qf.double().requires_grad_(True)
    z_ref = R.attn(qf64, R.keys(node64, x.edge, x.dt, x.tw, x.tb), x.mask, ew64, x.T)
    (z_ref * x.gz.double()).sum().backward()
    bufs, o = _guarded_set(dev, [("z", (x.R, x.H * x.dk)), ("stats", (x.R, x.H, 2)), ("parts", (x.R * x.H, x.N)),
                                 ("d_node", (x.R * x.N, dims[0])), ("d_qf", (x.R, x.H * x.dk))])
    a = TG._desc(x, dev, t)
    L.check(L.lib().tm_tgat_attn_fwd(C.byref(a), L.ptr(o.z), L.ptr(o.stats), st))
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(o.stats), L.ptr(t["gz"]), L.ptr(o.parts), L.ptr(o.d_node),
                                     L.ptr(o.d_qf), st))
    torch.cuda.synchronize()
    assert all(TGT.guards_intact(b) for b in bufs.values()), "a store outside an output"
    d_ew = o.parts.view(x.H, x.R, x.N).sum(0)                   # pair q = r H + h -> weight row q % rows
    tag = (dims, N, H)
    _close(tag, "z", o.z.view(x.R, x.H, x.dk), z_ref.detach())
    _close(tag, "d_ew", d_ew, ew64.grad)
    _close(tag, "d_node", o.d_node.view(x.R, x.N, -1), node64.grad)
    _close(tag, "d_qf", o.d_qf.view(x.R, x.H, x.dk), qf64.grad)
    # the nullable outputs alone: the other instances of the backward give the same bits
    b2, o2 = _guarded_set(dev, [("parts", (x.R * x.H, x.N)), ("d_node", (x.R * x.N, dims[0])),
                                ("d_qf", (x.R, x.H * x.dk)), ("parts_only", (x.R * x.H, x.N))])
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(o.stats), L.ptr(t["gz"]), L.ptr(o2.parts), None, L.ptr(o2.d_qf),
                                     st))
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(o.stats), L.ptr(t["gz"]), L.ptr(o2.parts), L.ptr(o2.d_node), None,
                                     st))
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(o.stats), L.ptr(t["gz"]), L.ptr(o2.parts_only), None, None, st))
    torch.cuda.synchronize()
    assert all(TGT.guards_intact(b) for b in b2.values())
    assert torch.equal(o2.parts, o.parts) and torch.equal(o2.parts_only, o.parts)
    assert torch.equal(o2.d_qf, o.d_qf) and torch.equal(o2.d_node, o.d_node)


# ------------------------------------------------------------------ 2. TGAT training pair
@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("dims", LAYOUTS, ids=lid)
def test_tgat_training_pair(dev, dims, N, H):
    from tempme_amd import _lib as L
    case = (ROWS, N, *dims, H, 0, True, True)                   # dense node table: d_node is written
    x = TGT.kernel_inputs(case, seed=sum(int(v) for v in case))
    t = TGT.device_inputs(dev, x)
    st = L.stream_ptr(dev)
    dn = dims[0]
    # keep = NULL: the plain pair's bits
    o0 = TGT.run_train_pair(L, dev, x, t, None, 1.0)
    a = TGT.describe(L, x, t)
    bufs, p = _guarded_set(dev, [("z", (x.R, x.H * x.dk)), ("stats", (x.R, x.H, 2)), ("parts", (x.R * x.H, x.N)),
                                 ("d_node", (x.R * x.N, dn)), ("d_qf", (x.R, x.H * x.dk))])
    L.check(L.lib().tm_tgat_attn_fwd(C.byref(a), L.ptr(p.z), L.ptr(p.stats), st))
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(p.stats), L.ptr(t["gz"]), L.ptr(p.parts), L.ptr(p.d_node),
                                     L.ptr(p.d_qf), st))
    torch.cuda.synchronize()
    assert o0.guards and all(TGT.guards_intact(b) for b in bufs.values())
    for name in ("z", "stats", "parts", "d_node", "d_qf"):
        assert torch.equal(getattr(o0, name), getattr(p, name)), name
    # an injected keep mask: the fp64 restatement
    ref = TGT.train_attn_ref(x, x.keep, x.scale)
    o = TGT.run_train_pair(L, dev, x, t, t["keep"], x.scale)
    assert o.guards and int(t["err"].item()) == 0
    assert torch.equal(o.stats, p.stats), "stats hold the plain softmax's max and sum"
    tag = (dims, N, H)
    _close(tag, "z", o.z.view(x.R, x.H, x.dk), ref.z)
    _close(tag, "d_ew_parts", o.parts.view(x.R, x.H, x.N), ref.d_ew)
    _close(tag, "d_qf", o.d_qf.view(x.R, x.H, x.dk), ref.d_qf)
    _close(tag, "d_node", o.d_node.view(x.R, x.N, dn), ref.d_node)
    err = (o.d_time.cpu().double() - ref.d_time).abs()
    bound = 1e-6 * ref.mag_time                                 # test_gpu_tgat_train's bound on the time gradient
    print(tag, "d_time worst err / bound", float((err / bound).max()), "|d_time| max", float(ref.d_time.abs().max()))
    assert torch.isfinite(o.d_time).all() and bool((err <= bound).all())
    # a second launch: the same bits
    o2 = TGT.run_train_pair(L, dev, x, t, t["keep"], x.scale)
    assert o2.guards
    for name in ("z", "stats", "parts", "d_node", "d_qf", "d_time"):
        assert torch.equal(getattr(o, name), getattr(o2, name)), name


# ------------------------------------------------------------------ 3. TGN plain pair
@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("dims", LAYOUTS, ids=lid)
def test_tgn_plain_pair_matches_fp64(dev, dims, N, H):
    """tm_tgn_attn_fwd / _bwd against the closed form of tests/tgn_train_ref.py without a keep mask (TGN's
    single-rounded time argument)."""
    from tempme_amd import _lib as L
    case = (ROWS, N, *dims, H, 0, 0, True)                      # node table rows 0 = dense
    x = TT.kernel_inputs(case, seed=sum(int(v) for v in case))
    t = TNT.device_inputs(dev, x)
    st = L.stream_ptr(dev)
    a = TNT.describe(L, x, t)
    bufs, o = _guarded_set(dev, [("z", (x.R, x.H * x.dk)), ("stats", (x.R, x.H, 2)), ("parts", (x.R * x.H, x.N)),
                                 ("d_node", (x.R * x.N, dims[0])), ("parts_only", (x.R * x.H, x.N))])
    L.check(L.lib().tm_tgn_attn_fwd(C.byref(a), L.ptr(o.z), L.ptr(o.stats), st))
    L.check(L.lib().tm_tgn_attn_bwd(C.byref(a), L.ptr(o.stats), L.ptr(t["gz"]), L.ptr(o.parts), L.ptr(o.d_node), st))
    L.check(L.lib().tm_tgn_attn_bwd(C.byref(a), L.ptr(o.stats), L.ptr(t["gz"]), L.ptr(o.parts_only), None, st))
    torch.cuda.synchronize()
    assert all(TGT.guards_intact(b) for b in bufs.values()) and int(t["err"].item()) == 0
    ref = TR.attn_closed_form(x, None, 1.0)
    tag = (dims, N, H)
    _close(tag, "z", o.z.view(x.R, x.H, x.dk), ref.z)
    _close(tag, "d_ew (per pair)", o.parts.view(x.R, x.H, x.N), ref.d_ew)
    _close(tag, "d_node", o.d_node.view(x.R, x.N, -1), ref.d_node)
    assert torch.equal(o.parts_only, o.parts)


# ------------------------------------------------------------------ 4. the fused tail
def _tail(dev, rows, dk, feat, H):
    from tempme_amd import _lib as L
    gen = torch.Generator().manual_seed(rows * 1000 + dk + feat)
    w = TG._tail_weights(dk, feat, H, gen)
    z = torch.randn(rows, H * dk, generator=gen, dtype=torch.float64).float()
    query = torch.randn(rows, dk, generator=gen, dtype=torch.float64).float()
    w32 = {k: v.float() for k, v in w.items()}
    ref = R.tail(z.double(), query.double(), {k: v.double() for k, v in w32.items()}, feat)
    cpu32 = R.tail(z, query, w32, feat)
    tol = max(10 * (cpu32.double() - ref).abs().max().item(), 1e-6)
    lw = dict(Gt=w32["G"].t().contiguous().to(dev), fcb=w32["fcb"].to(dev), lnw=w32["lnw"].to(dev),
              lnb=w32["lnb"].to(dev))
    for k in ("11", "12", "21", "22"):
        lw[f"w{k}t"] = w32[f"w{k}"].t().contiguous().to(dev)
        lw[f"b{k}"] = w32[f"b{k}"].to(dev)
    zd, qd = z.to(dev), query.to(dev)
    m = L.TgatMerge()
    m.rows, m.n_head, m.d_key, m.feat = rows, H, dk, feat
    m.z, m.query = zd.data_ptr(), qd.data_ptr()
    for f, k in (("gt", "Gt"), ("fc_b", "fcb"), ("ln_w", "lnw"), ("ln_b", "lnb"), ("w11t", "w11t"), ("b11", "b11"),
                 ("w12t", "w12t"), ("b12", "b12"), ("w21t", "w21t"), ("b21", "b21"), ("w22t", "w22t"), ("b22", "b22")):
        setattr(m, f, lw[k].data_ptr())
    outs = []
    for _ in range(2):
        buf, out = TGT.guarded(dev, rows, feat)
        L.check(L.lib().tm_tgat_merge_fwd(C.byref(m), L.ptr(out), L.stream_ptr(dev)), "TGAT layer tail")
        torch.cuda.synchronize()
        assert TGT.guards_intact(buf)
        outs.append(out)
    err = (outs[0].cpu().double() - ref).abs().max().item()
    print(rows, dk, feat, H, "fused max err", err, "tol", tol)
    assert torch.isfinite(outs[0]).all()
    assert err <= tol
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("dk,feat,H", [(516, 172, 2), (516, 5, 3), (576, 172, 4), (513, 172, 3)])
def test_fused_tail_nine_tiles_matches_fp64(dev, rows, dk, feat, H):
    _tail(dev, rows, dk, feat, H)


def test_fused_tail_eight_tiles_at_512(dev):
    """d_key = 512 still takes the 8-tile instance: within the same rule, and the same bits twice."""
    _tail(dev, 33, 512, 172, 2)


# ------------------------------------------------------------------ 5. limits
def test_d_key_577_is_refused(dev):
    from tempme_amd import _lib as L
    lib = L.lib()
    st = L.stream_ptr(dev)
    buf = torch.empty(1 << 16, device=dev)
    wide = dict(d_node=300, d_edge=200, d_time=77)              # 577

    def refused(rc, who):
        assert rc == L.TM_E_UNSUPPORTED, who
        msg = lib.tm_last_error().decode()
        assert "576" in msg and who in msg, msg

    x = TGT.kernel_inputs(TGT.KERNEL_CASES[0], seed=1)
    t = TGT.device_inputs(dev, x)
    a = TGT.describe(L, x, t)
    for k, v in wide.items():
        setattr(a, k, v)
    refused(lib.tm_tgat_attn_fwd(C.byref(a), L.ptr(buf), L.ptr(buf), st), "tm_tgat_attn_fwd")
    refused(lib.tm_tgat_attn_bwd(C.byref(a), L.ptr(buf), L.ptr(buf), L.ptr(buf), None, L.ptr(buf), st),
            "tm_tgat_attn_bwd")
    refused(lib.tm_tgat_attn_train_fwd(C.byref(a), None, 1.0, L.ptr(buf), L.ptr(buf), st), "tm_tgat_attn_train_fwd")
    refused(lib.tm_tgat_attn_train_bwd(C.byref(a), None, 1.0, L.ptr(buf), L.ptr(buf), None, None, L.ptr(buf),
                                       L.ptr(buf), L.ptr(buf), st), "tm_tgat_attn_train_bwd")
    xn = TT.kernel_inputs(TT.KERNEL_CASES[0], seed=1)
    tn = TNT.device_inputs(dev, xn)
    b = TNT.describe(L, xn, tn)
    for k, v in wide.items():
        setattr(b, k, v)
    refused(lib.tm_tgn_attn_fwd(C.byref(b), L.ptr(buf), L.ptr(buf), st), "tm_tgn_attn_fwd")
    refused(lib.tm_tgn_attn_bwd(C.byref(b), L.ptr(buf), L.ptr(buf), L.ptr(buf), None, st), "tm_tgn_attn_bwd")
    m = L.TgatMerge()
    m.rows, m.n_head, m.d_key, m.feat = 4, 2, 577, 5
    refused(lib.tm_tgat_merge_fwd(C.byref(m), None, st), "tm_tgat_merge_fwd")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6. the TGN model
TGN_CASES = [(3, 172, 172), (4, 171, 171), (5, 192, 192)]       # seed, d_node, d_edge
TGN_N, TGN_B = 5, 4


def _tgn_case(seed, dn, de):
    key = ("tgn", seed, dn, de)
    if key in _cache:
        return _cache[key]
    from tempme_amd.tgn import TGN
    nf, ef, src, dst, fake, cut, sgs, ew = TN._random_case(seed, V=50, E=300, N=TGN_N, B=TGN_B, dn=dn, de=de)
    torch.manual_seed(seed)
    m = TGN(nf, ef, n_neighbors=TGN_N, device=torch.device("cpu"), n_layers=2, n_heads=2, dropout=0.1)
    m.forbidden_memory_update = True
    with torch.no_grad():
        m.memory.memory.normal_(0, 0.5)
        m.time_encoder.w.bias.normal_(0, 0.5)
    m.eval()
    c = SimpleNamespace(m=m, nf=nf, ef=ef, src=src, dst=dst, fake=fake, cut=cut, sgs=sgs, ew=ew,
                        sd={k: v.detach() for k, v in m.state_dict().items()})
    _cache[key] = c
    return c


def _oracle(c, ew, sgs=None, dtype=torch.float64):
    sgs = c.sgs if sgs is None else sgs
    return O.contrast(c.sd, c.m.memory.messages, c.nf, c.ef, c.src, c.dst, c.fake, c.cut, *sgs, TGN_N, 2, ew, None,
                      dtype=dtype)


@pytest.mark.parametrize("seed,dn,de", TGN_CASES)
def test_tgn_contrast_matches_oracle(dev, seed, dn, de):
    c = _tgn_case(seed, dn, de)
    p, n = c.m.contrast(c.src, c.dst, c.fake, c.cut, None, *c.sgs, explain_weights=[x.to(dev) for x in c.ew])
    c.m.check_errors()
    got = torch.cat([p, n]).detach().cpu().double().numpy()
    p64, n64 = _oracle(c, c.ew)
    want = torch.cat([p64, n64]).numpy()
    print(dn, de, "max |logit - fp64 oracle|", float(np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("seed,dn,de", TGN_CASES)
def test_tgn_explanation_weight_gradient_matches_oracle(dev, seed, dn, de):
    """test_gpu_tgn.test_explanation_weight_gradient_vs_oracle's bounds at the wide keys."""
    c = _tgn_case(seed, dn, de)
    y = torch.cat([torch.ones(TGN_B, 1), torch.zeros(TGN_B, 1)])
    ew = [x.clone().to(dev).requires_grad_(True) for x in c.ew]
    p, n = c.m.contrast(c.src, c.dst, c.fake, c.cut, None, *c.sgs, explain_weights=ew)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(torch.cat([p, n]), y.to(dev))
    loss.backward()
    ew64 = [x.clone().double().requires_grad_(True) for x in c.ew]
    p64, n64 = _oracle(c, ew64)
    loss64 = torch.nn.functional.binary_cross_entropy_with_logits(torch.cat([p64, n64]), y.double())
    loss64.backward()
    assert abs(loss.item() - loss64.item()) < 1e-5
    for a, b in zip(ew, ew64):
        ga, gb = a.grad.double().cpu(), b.grad
        print(dn, de, "grad err", float(torch.linalg.norm(ga - gb)), "|g64|", float(torch.linalg.norm(gb)))
        assert torch.linalg.norm(ga - gb) <= 1e-4 * torch.linalg.norm(gb)
        assert (ga - gb).abs().max() <= 1e-6 + 1e-4 * gb.abs().max()
    assert all(q.grad is None for q in c.m.parameters())           # frozen base model


def test_tgn_threshold_test_at_516(dev):
    """threshold_test's masks are the oracle's top-k bit for bit, the masked contrast of every ratio follows the
    fp64 oracle on the oracle's masked subgraphs, and threshold_test itself runs."""
    from tempme_amd import fidelity
    c = _tgn_case(*TGN_CASES[0])
    N, B = TGN_N, TGN_B
    ne = N + N * N
    ratios = [0.1, 0.3, 0.5, 0.9]
    expl = [x.to(dev) for x in c.ew]
    masked = fidelity._masked_nodes(expl, c.sgs, N, ratios, dev).cpu().numpy()
    imp = torch.cat(c.ew, dim=1).numpy()
    pos, neg = fidelity.masked_contrast(c.m, expl, c.src, c.dst, c.fake, c.cut, *c.sgs, N, ratios)
    got = torch.cat([pos, neg], dim=1).detach().cpu().double().numpy()
    for gi, r in enumerate(ratios):
        k = ne - min(max(int(np.ceil(r * ne)), 1), ne)
        sel = O.select_k_smallest(imp, k)
        msg = [O.masked_subgraph(sg, sel[s * B:(s + 1) * B], N) for s, sg in enumerate(c.sgs)]
        want_nodes = np.concatenate([np.concatenate(m[0], axis=1) for m in msg], axis=0)
        assert np.array_equal(masked[gi], want_nodes.astype(np.int32)), r
        p64, n64 = _oracle(c, None, sgs=msg)
        want = torch.cat([p64, n64]).numpy().reshape(-1)
        np.testing.assert_allclose(got[gi], want, atol=2e-5, rtol=1e-5, err_msg=str(r))
    with torch.no_grad():
        p, n = c.m.contrast(c.src, c.dst, c.fake, c.cut, None, *c.sgs)
    ori = torch.cat([p, n])
    y_ori = torch.where(ori.sigmoid() > 0.5, 1., 0.).view(-1, 1)
    y_ori[0], y_ori[-1] = 1.0, 0.0                                # both classes present for the ranking metrics
    args = SimpleNamespace(ratios=ratios, base_type="tgn", n_degree=N, bs=B)
    metrics = fidelity.threshold_test(args, expl, c.m, c.src, c.dst, c.fake, c.cut, None, p, n, y_ori, *c.sgs)
    assert len(metrics) == 5 and np.isfinite(metrics).all()


def test_tgn_training_at_516_is_still_refused(dev):
    """TGN base training stays at d_key <= 512: the first step's refusal names d_key."""
    from tempme_amd.tgn import TGN
    nf, ef, src, dst, fake, cut, sgs, _ = TN._random_case(3, V=50, E=300, N=TGN_N, B=TGN_B, dn=172, de=172)
    torch.manual_seed(3)
    m = TGN(nf, ef, n_neighbors=TGN_N, device=torch.device("cpu"), n_layers=2, n_heads=2, dropout=0.1).to(dev)
    m.train()
    m.train_on_hip()
    e_idx = np.arange(1, TGN_B + 1)
    with pytest.raises(NotImplementedError, match="d_key"):
        m.contrast(src, dst, fake, cut, e_idx, *sgs)


# ------------------------------------------------------------------ 7. the TGAT model
TGAT_SHAPES = [(4, 5, 172, 172, 2, 0.1), (3, 3, 171, 171, 3, 0.5), (3, 4, 192, 192, 4, 0.0)]


@pytest.mark.parametrize("shape", TGAT_SHAPES, ids=TGT.ids)
def test_tgat_training_step_matches_fp64_formulation(dev, shape):
    c = TGT.make_case(dev, *shape)
    assert c.marker == (3 * c.B, c.N, c.p > 0), "the HIP training path did not run"
    l64 = torch.cat([c.ref64[1], c.ref64[2]]).numpy()
    l32 = torch.cat([c.ref32[1], c.ref32[2]]).double().numpy()
    atol = 10.0 * max(float(np.abs(l32 - l64).max()), 2e-6)
    got = torch.cat([c.pos, c.neg]).double().cpu().numpy()
    print("max |logit - fp64|", float(np.abs(got - l64).max()), "atol", atol)
    np.testing.assert_allclose(got, l64, atol=atol, rtol=TGT.RTOL)
    np.testing.assert_allclose(float(c.loss), float(c.ref64[0]), atol=atol, rtol=TGT.RTOL)
    assert len(c.grads) == 36
    worst = TGT.check_grads(c.grads, c.ref64[3], c.ref32[3])
    print("worst err / bound per tensor kind:", {k: round(v, 4) for k, v in sorted(worst.items())})
    # the second step: the same bits
    assert torch.equal(c.loss, c.loss2) and torch.equal(c.pos, c.pos2) and torch.equal(c.neg, c.neg2)
    for k, g in c.grads.items():
        assert torch.equal(g, c.grads2[k]), k
    assert torch.equal(c.eval_before, c.eval_after), "eval-mode contrast changed after train_on_hip()"


@pytest.mark.parametrize("shape", TGAT_SHAPES, ids=TGT.ids)
def test_tgat_frozen_contrast_fused_tail(dev, shape):
    """The frozen contrast with explanation weights: the fused tail (no gradient needed) equals the torch tail (the
    weights require a gradient) within the case's logit tolerance, the 9-tile kernel ran, and the gradient reaches
    all six weight tensors."""
    from tempme_amd import _lib as L
    c = TGT.make_case(dev, *shape)
    m, b = c.model, c.batch
    l64 = torch.cat([c.ref64[1], c.ref64[2]]).numpy()
    l32 = torch.cat([c.ref32[1], c.ref32[2]]).double().numpy()
    atol = 10.0 * max(float(np.abs(l32 - l64).max()), 2e-6)
    gen = torch.Generator().manual_seed(c.B + c.N)
    base = [(torch.rand(c.B, c.N, generator=gen), torch.rand(c.B, c.N * c.N, generator=gen)) for _ in range(3)]

    def run(grad):
        w = [tuple(x.to(dev).requires_grad_(grad) for x in side) for side in base]
        pos, neg = m.contrast(b[0], b[1], b[2], b[3], None, *b[4:], if_explain=True,
                              exp_weights=[[w[0], w[1]], [w[0], w[2]]])
        return torch.cat([pos, neg]), w
    was_training, was_fused = m.training, m.fused_tail
    m.eval()
    try:
        m.fused_tail = True
        L.profile_enable(True)
        with torch.no_grad():
            fused, _ = run(False)
        names = L.profile_read()
        L.profile_enable(False)
        assert names["tgat_merge_fwd_kernel"][1] == 3 and names["tgat_attn_fwd_kernel"][1] == 3
        out, w = run(True)
        assert out.requires_grad
        np.testing.assert_allclose(fused.cpu().numpy(), out.detach().cpu().numpy(), atol=atol, rtol=TGT.RTOL)
        m.fused_tail = False
        with torch.no_grad():
            off, _ = run(False)
        assert torch.equal(off, out.detach())
        out.sum().backward()
        for side in w:
            for x in side:
                assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
        assert all(q.grad is None for q in m.parameters())          # frozen on this path
        m.check_errors()
    finally:
        m.fused_tail = was_fused
        m.train(was_training)


def test_tgat_threshold_test_at_516(dev):
    from tempme_amd import fidelity
    c = TGT.make_case(dev, *TGAT_SHAPES[0])
    m, b = c.model, c.batch
    gen = torch.Generator().manual_seed(11)
    expl = [torch.rand(c.B, c.N if h == 0 else c.N * c.N, generator=gen).to(dev) for _ in range(3) for h in (0, 1)]
    was_training = m.training
    m.eval()
    try:
        with torch.no_grad():
            p, n = m.contrast(b[0], b[1], b[2], b[3], None, *b[4:])
        y_ori = torch.where(torch.cat([p, n]).sigmoid() > 0.5, 1., 0.).view(-1, 1)
        y_ori[0], y_ori[-1] = 1.0, 0.0
        args = SimpleNamespace(ratios=[0.2, 0.6], base_type="tgat", n_degree=c.N, bs=c.B)
        metrics = fidelity.threshold_test(args, expl, m, b[0], b[1], b[2], b[3], None, p, n, y_ori, *b[4:])
    finally:
        m.train(was_training)
    assert len(metrics) == 5 and np.isfinite(metrics).all()


def test_learn_base_tgat_epoch_at_172_172(dev):
    """learn_base.train_epoch with a TGAT at Wikipedia's widths (172 node and 172 edge features, model width 516):
    two steps at bs = 16, N = 5, p = 0.1 on the uslegis fixture's events with 172 random edge-feature columns."""
    import pandas as pd

    from tempme_amd import learn_base
    from tempme_amd.tgat import TGAT
    G = os.path.join(TI.G, "data")
    g_df = pd.read_csv(os.path.join(G, "ml_uslegis_sampled.csv"))
    rows = np.load(os.path.join(G, "ml_uslegis_sampled.npy")).shape[0]
    nf = np.load(os.path.join(G, "ml_uslegis_sampled_node.npy"))
    assert nf.shape[1] == 172
    ef = np.random.default_rng(1).uniform(-1, 1, (rows, 172)).astype(np.float32)
    ef[0] = 0
    sp = learn_base.split_data(g_df, device=dev)
    idx = np.random.default_rng(0).permutation(len(sp.train_src_l))
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        m = TGAT(nf, ef, 5, num_layers=2, n_head=2, drop_out=0.1).to(dev)
        assert m.model_dim == 516
        m.train_on_hip()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        out = learn_base.train_epoch(m, opt, sp.train_ngh_finder, sp.train_rand_sampler, sp.train_src_l, sp.train_dst_l,
                                     sp.train_ts_l, sp.train_e_idx_l, 16, idx_list=idx, max_steps=2, metrics=False)
        assert m._tgat_train_key == (3 * 16, 5, True)
        m.check_errors()
        runs.append(out["loss"])
    print("losses", runs[0])
    assert len(runs[0]) == 2 and np.isfinite(runs[0]).all()
    assert runs[0] == runs[1]
