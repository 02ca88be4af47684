"""Base-TGN training on the HIP path: the training pair of the attention kernels through the C ABI
(tm_tgn_attn_train_fwd / tm_tgn_attn_train_bwd / tm_tgn_attn_train_dtab / tm_tgn_rows_reduce, csrc/tgn_train.hip)
against the plain kernels and an fp64 closed form; the stateful training step of TGN.train_on_hip against the
reference's own four steps (tests/golden/tgn_train.npz) and against the reference-shaped torch formulation with the
same dropout masks (tests/tgn_train_ref.py); the memory state it leaves; and, end to end, learn_base.train_epoch.

Tolerances.  Kernel outputs: 1e-5 of the tensor's largest element (at least 1) for z, d_ew_parts, d_qf, d_node and
d_tab; d_time within 1e-6 of the summed magnitudes of its terms (the derivation is in test_gpu_tgat_train's
docstring; the kernels differ in the rounding of the cosine's argument only).  Logits: atol 2e-5.  Parameter
gradients: per tensor ||g_hip - g_64|| <= max(1e-4 ||g_64||, 10 ||g_32 - g_64||) with g_32 / g_64 the reference's
(or the formulation's) two runs; where g_64 is identically zero the HIP gradient must be exactly zero.  Memory and
stored raw messages: max(1e-5, 10 x the reference's own fp32-vs-fp64 distance); last_update, the timestamps and the
set of nodes with a pending message: equal.
"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tgn_inputs as TI
import tgn_train_inputs as TT
import tgn_train_ref as TR
from tests.test_gpu_tgat_train import check_grads, grads_of, guarded, guards_intact

pytestmark = pytest.mark.gpu

RTOL = 1e-5
LOGIT_ATOL = 2e-5
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


def _tol(ref):
    return 1e-5 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ 1. the kernels through the C ABI
def device_inputs(dev, x):
    t = {k: getattr(x, k).to(dev).contiguous() for k in ("node", "edge", "dt", "tw", "tb", "qf", "gz", "mask", "keep")}
    if x.ew is not None:
        t["ew"] = x.ew.to(dev).contiguous()
    if not x.dense:
        t["tab"], t["node_idx"] = x.tab.to(dev).contiguous(), x.node_idx.to(dev).contiguous()
    t["err"] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def describe(L, x, t):
    dn, de, dtm = x.dims
    a = L.TgnAttn()
    a.rows, a.n_ngh, a.n_head = x.R, x.N, x.H
    a.d_node, a.d_edge, a.d_time = dn, de, dtm
    a.head_major_rows, a.seg_rows = 1, x.seg
    a.temperature = x.T
    if x.dense:
        a.node_tab, a.node_idx, a.node_rows = t["node"].data_ptr(), None, 0
    else:
        a.node_tab, a.node_idx, a.node_rows = t["tab"].data_ptr(), t["node_idx"].data_ptr(), x.node_rows
    a.edge_tab, a.edge_idx, a.edge_rows = t["edge"].data_ptr(), None, 0
    a.dt, a.time_w, a.time_b = t["dt"].data_ptr(), t["tw"].data_ptr(), t["tb"].data_ptr()
    a.mask_node, a.qf = t["mask"].data_ptr(), t["qf"].data_ptr()
    a.ew = t["ew"].data_ptr() if x.ew is not None else None
    a.err_flag = t["err"].data_ptr()
    return a


def run_train_pair(L, dev, x, t, keep, scale, gz=None, with_parts=True, row_begin=0):
    """tm_tgn_attn_train_fwd + _bwd (+ _dtab for a gathered table) on guarded outputs -> the payload views."""
    from tempme_amd.tgn import _rows_by_table_row
    dn, de, dtm = x.dims
    a = describe(L, x, t)
    st = L.stream_ptr(dev)
    lib = L.lib()
    o = SimpleNamespace()
    bufs = {}
    shapes = [("z", (x.R, x.H * x.dk)), ("stats", (x.R, x.H, 2)), ("parts", (x.R * x.H, x.N)),
              ("d_qf", (x.R, x.H * x.dk)), ("d_time", (2, dtm))]
    shapes += [("d_node", (x.R * x.N, dn))] if x.dense else [("ab", (x.R, x.N, x.H, 2)), ("d_tab", (x.node_rows, dn))]
    for name, shape in shapes:
        bufs[name], view = guarded(dev, *shape)
        setattr(o, name, view)
    ws_bytes = int(lib.tm_tgn_attn_train_workspace_bytes(x.R, dtm))
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    bufs["ws"], ws = guarded(dev, ws_bytes // 4)
    gz = t["gz"] if gz is None else gz
    L.check(lib.tm_tgn_attn_train_fwd(C.byref(a), L.ptr(keep), scale, L.ptr(o.z), L.ptr(o.stats), st))
    L.check(lib.tm_tgn_attn_train_bwd(C.byref(a), L.ptr(keep), scale, L.ptr(o.stats), L.ptr(gz),
                                      L.ptr(o.parts) if with_parts else None, L.ptr(o.d_node) if x.dense else None,
                                      L.ptr(o.d_qf), L.ptr(o.d_time), None if x.dense else L.ptr(o.ab), L.ptr(ws), st))
    if not x.dense:
        order, seg = _rows_by_table_row(t["node_idx"].reshape(-1), x.node_rows)
        L.check(lib.tm_tgn_attn_train_dtab(C.byref(a), L.ptr(o.ab), L.ptr(gz), L.ptr(order), order.shape[0], L.ptr(seg),
                                           row_begin, L.ptr(o.d_tab), st))
    torch.cuda.synchronize()
    o.guards = all(guards_intact(b) for b in bufs.values())
    return o


@pytest.mark.parametrize("case", TT.KERNEL_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_train_kernels(dev, case):
    from tempme_amd import _lib as L
    x = TT.kernel_inputs(case, seed=sum(int(v) for v in case))
    t = device_inputs(dev, x)
    st = L.stream_ptr(dev)
    dn = x.dims[0]
    # keep = NULL: the plain pair's bits
    o0 = run_train_pair(L, dev, x, t, None, 1.0)
    a = describe(L, x, t)
    z = torch.empty(x.R, x.H * x.dk, device=dev)
    stats = torch.empty(x.R, x.H, 2, device=dev)
    parts = torch.empty(x.R * x.H, x.N, device=dev)
    d_node = torch.empty(x.R * x.N, dn, device=dev) if x.dense else None
    L.check(L.lib().tm_tgn_attn_fwd(C.byref(a), L.ptr(z), L.ptr(stats), st))
    L.check(L.lib().tm_tgn_attn_bwd(C.byref(a), L.ptr(stats), L.ptr(t["gz"]), L.ptr(parts), L.ptr(d_node), st))
    assert o0.guards
    assert torch.equal(o0.z, z) and torch.equal(o0.stats, stats) and torch.equal(o0.parts, parts)
    if x.dense:
        assert torch.equal(o0.d_node, d_node)
    # with the mask: the fp64 closed form
    ref = TR.attn_closed_form(x, x.keep, x.scale)
    o = run_train_pair(L, dev, x, t, t["keep"], x.scale)
    assert o.guards and int(t["err"].item()) == 0
    assert torch.equal(o.stats, stats), "stats hold the plain softmax's max and sum"
    checks = [("z", o.z.view(x.R, x.H, x.dk), ref.z), ("d_ew_parts", o.parts.view(x.R, x.H, x.N), ref.d_ew),
              ("d_qf", o.d_qf.view(x.R, x.H, x.dk), ref.d_qf)]
    if x.dense:
        checks.append(("d_node", o.d_node.view(x.R, x.N, dn), ref.d_node))
    else:
        checks += [("d_tab", o.d_tab, ref.d_tab), ("slot a", o.ab[..., 0], ref.a), ("slot b", o.ab[..., 1], ref.b)]
    for name, got, want in checks:
        err = (got.cpu().double() - want).abs().max().item()
        print(case, name, "max err", err, "tol", _tol(want))
        assert torch.isfinite(got).all(), name
        assert err <= _tol(want), name
    err = (o.d_time.cpu().double() - ref.d_time).abs()
    bound = 1e-6 * ref.mag_time
    print(case, "d_time worst err / bound", float((err / bound).max()), "|d_time| max", float(ref.d_time.abs().max()))
    assert torch.isfinite(o.d_time).all() and bool((err <= bound).all())
    # a second launch: the same bits, the time and the table gradient included
    o2 = run_train_pair(L, dev, x, t, t["keep"], x.scale)
    names = ("z", "parts", "d_qf", "d_time") + (("d_node",) if x.dense else ("ab", "d_tab"))
    for name in names:
        assert torch.equal(getattr(o, name), getattr(o2, name)), name
    # d_ew_parts is nullable: the other outputs do not change
    o3 = run_train_pair(L, dev, x, t, t["keep"], x.scale, with_parts=False)
    assert torch.equal(o3.d_qf, o.d_qf) and torch.equal(o3.d_time, o.d_time) and bool(torch.isnan(o3.parts).all())
    # the (row, head) pair whose keep bytes are all zero: z, d_qf and d ew of the pair are exactly 0, and nothing
    # of its gz reaches any other output
    r0, h0 = 2, x.H - 1
    assert float(o.z.view(x.R, x.H, x.dk)[r0, h0].abs().max()) == 0.0
    assert float(o.d_qf.view(x.R, x.H, x.dk)[r0, h0].abs().max()) == 0.0
    assert float(o.parts.view(x.R, x.H, x.N)[r0, h0].abs().max()) == 0.0
    gz2 = t["gz"].clone()
    gz2[r0, h0] = torch.randn(x.dk, generator=torch.Generator().manual_seed(3)).to(dev) * 5.0
    o4 = run_train_pair(L, dev, x, t, t["keep"], x.scale, gz=gz2)
    assert torch.equal(o4.d_time, o.d_time) and torch.equal(o4.d_qf, o.d_qf) and torch.equal(o4.parts, o.parts)
    if x.dense:
        assert torch.equal(o4.d_node, o.d_node)
        return
    assert torch.equal(o4.d_tab, o.d_tab)
    # table rows no slot names are exactly zero (written, not accumulated into the NaN-filled buffer)
    used = torch.zeros(x.node_rows, dtype=torch.bool)
    used[x.node_idx.reshape(-1).long()] = True
    if x.R * x.N < 3 * x.node_rows:
        assert int((~used).sum()) > 0
    assert float(o.d_tab[(~used).to(dev)].abs().sum()) == 0.0
    assert bool(used[0]), "a quarter of the slots name the padding row"
    # row_begin = 1 leaves the padding row zero without reading its list; the other rows keep their bits
    o5 = run_train_pair(L, dev, x, t, t["keep"], x.scale, row_begin=1)
    assert o5.guards and float(o5.d_tab[0].abs().max()) == 0.0 and torch.equal(o5.d_tab[1:], o.d_tab[1:])
    assert float(o.d_tab[0].abs().max()) > 0.0


def test_rows_reduce_is_the_gather_backward(dev):
    """tm_tgn_rows_reduce: out[v] = sum of the gradient rows whose index is v, against index_add in fp64; the same
    bits twice; rows nobody names are zero."""
    from tempme_amd import _lib as L
    from tempme_amd.tgn import _GatherRowsFn, _rows_by_table_row
    gen = torch.Generator().manual_seed(5)
    for n, d, V in ((4101, 24, 50), (37, 172, 300), (9, 70, 4)):
        idx = torch.randint(0, V, (n,), generator=gen)
        idx[torch.rand(n, generator=gen) < 0.25] = 0
        g = torch.randn(n, d, generator=gen)
        want = torch.zeros(V, d, dtype=torch.float64).index_add_(0, idx, g.double())
        gd, idd = g.to(dev), idx.to(dev)
        order, seg = _rows_by_table_row(idd, V)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        outs = []
        for _ in range(2):
            buf, out = guarded(dev, V, d)
            L.check(L.lib().tm_tgn_rows_reduce(L.ptr(gd), n, d, L.ptr(order), n, L.ptr(seg), V, 0, L.ptr(out), L.ptr(err),
                                               L.stream_ptr(dev)))
            torch.cuda.synchronize()
            assert guards_intact(buf) and int(err.item()) == 0
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        assert float((outs[0].cpu().double() - want).abs().max()) <= _tol(want)
        used = torch.zeros(V, dtype=torch.bool)
        used[idx] = True
        assert float(outs[0][(~used).to(dev)].abs().sum()) == 0.0
        # the autograd function built on it: tab[idx] forward, the reduction backward (the padding row takes none)
        tab = torch.randn(V, d, generator=gen).to(dev).requires_grad_(True)
        y = _GatherRowsFn.apply(tab, idd, err)
        assert torch.equal(y, tab.detach()[idd])
        y.backward(gd)
        assert float(tab.grad[0].abs().max()) == 0.0 and torch.equal(tab.grad[1:], outs[0][1:])


def test_train_kernel_limits_are_refused(dev):
    from tempme_amd import _lib as L
    x = TT.kernel_inputs(TT.KERNEL_CASES[0], seed=1)
    t = device_inputs(dev, x)
    buf = torch.empty(1 << 16, device=dev)
    idx = torch.zeros(64, dtype=torch.long, device=dev)
    st = L.stream_ptr(dev)
    lib = L.lib()
    # d_key = 172 + 172 + 172 = 516 (wikipedia) stays unsupported
    for change, code in ((dict(d_node=172, d_edge=172, d_time=172), L.TM_E_UNSUPPORTED), (dict(n_head=5), L.TM_E_UNSUPPORTED),
                         (dict(n_ngh=400), L.TM_E_UNSUPPORTED), (dict(n_ngh=0), L.TM_E_ARG)):
        a = describe(L, x, t)
        for k, v in change.items():
            setattr(a, k, v)
        assert lib.tm_tgn_attn_train_fwd(C.byref(a), None, 1.0, L.ptr(buf), L.ptr(buf), st) == code
        assert lib.tm_tgn_attn_train_bwd(C.byref(a), None, 1.0, L.ptr(buf), L.ptr(buf), None, None, L.ptr(buf),
                                         L.ptr(buf), None, L.ptr(buf), st) == code
        assert lib.tm_tgn_attn_train_dtab(C.byref(a), L.ptr(buf), L.ptr(buf), L.ptr(idx), 0, L.ptr(idx), 0, L.ptr(buf),
                                          st) == code
        assert lib.tm_last_error()
    # d_node wants a dense table, the table gradient a gathered one
    a = describe(L, x, t)
    assert lib.tm_tgn_attn_train_bwd(C.byref(a), None, 1.0, L.ptr(buf), L.ptr(buf), None, L.ptr(buf), L.ptr(buf),
                                     L.ptr(buf), None, L.ptr(buf), st) == L.TM_E_ARG
    a.node_idx = None
    assert lib.tm_tgn_attn_train_dtab(C.byref(a), L.ptr(buf), L.ptr(buf), L.ptr(idx), 4, L.ptr(idx), 0, L.ptr(buf),
                                      st) == L.TM_E_ARG
    assert lib.tm_tgn_rows_reduce(L.ptr(buf), 4, 600, L.ptr(idx), 4, L.ptr(idx), 4, 0, L.ptr(buf), None,
                                  st) == L.TM_E_UNSUPPORTED
    assert lib.tm_tgn_attn_train_workspace_bytes(-1, 8) == -1


# ------------------------------------------------------------------ 2. the reference's own four steps
def bce_step(model, batch):
    p, n = model.contrast(*batch)
    crit = torch.nn.functional.binary_cross_entropy_with_logits
    loss = crit(p, torch.ones_like(p)) + crit(n, torch.zeros_like(n))
    loss.backward()
    model.memory.detach_memory()
    return loss.detach(), p.detach(), n.detach()


def live_grads(model):
    return {k: v for k, v in grads_of(model).items() if v is not None}


def golden_run(dev, case):
    """The golden run on the device, once per case: four training steps (no optimizer step), the state they leave,
    the frozen model's logits on that state."""
    if ("golden", case) in _cache:
        return _cache["golden", case]
    m = TT.build_model(case).to(dev)
    m.train_on_hip()
    c = SimpleNamespace(model=m, steps=[], shapes=TT.shapes_of(m))
    for batch in TT.step_batches():
        m.zero_grad(set_to_none=True)
        loss, pos, neg = bce_step(m, batch)
        c.steps.append((loss, pos, neg, live_grads(m)))
    m.zero_grad(set_to_none=True)
    m.check_errors()
    c.marker = m._tgn_train_key
    c.memory, c.last_update = m.memory.memory.detach().cpu().clone(), m.memory.last_update.detach().cpu().clone()
    c.pending = {k: v.cpu() for k, v in m.pending_messages().items()}
    c.other_grads = [m.memory.memory.grad, m.memory.last_update.grad, m.n_feat_th.grad, m.e_feat_th.grad]
    m.forbidden_memory_update = True
    m.eval()
    with torch.no_grad():
        c.frozen = torch.cat(m.contrast(*TT.full_batch())).cpu()
    m.forbidden_memory_update = False
    m.train()
    _cache["golden", case] = c
    return c


@pytest.mark.parametrize("case", list(TT.CASES))
def test_reference_training_steps_on_the_device(dev, case):
    g = TT.golden()
    c = golden_run(dev, case)
    assert c.marker == (3 * TT.STEP_B, TI.N_DEG, False), "the HIP training path did not run"
    for k, (loss, pos, neg, grads) in enumerate(c.steps):
        l64, logits64, names, g64, n64 = TT.stored(g, case, k, "64", c.shapes)
        _, _, _, g32, n32 = TT.stored(g, case, k, "32", c.shapes)
        got = torch.cat([pos, neg]).double().cpu().numpy().reshape(-1)
        print(case, "step", k, "max |logit - reference fp64|", float(np.abs(got - logits64).max()))
        np.testing.assert_allclose(got, logits64, atol=LOGIT_ATOL, rtol=RTOL)
        np.testing.assert_allclose(float(loss), l64, atol=LOGIT_ATOL, rtol=RTOL)
        # every tensor the reference's step fills gets a .grad, and no other
        assert set(grads) == set(names), (k, set(grads) ^ set(names))
        worst = check_grads(grads, g64, g32, tag=f"{case} s{k} ")
        for n, ref in n64.items():
            got_n = float(torch.linalg.norm(grads[n].double()))
            bound = max(1e-4 * ref, 10 * abs(n32[n] - ref))
            print(f"{case} s{k} {n}: norm {got_n:.6e} stored {ref:.6e} bound {bound:.3e}")
            assert abs(got_n - ref) <= bound, (k, n, got_n, ref, bound)
        print("worst err / bound per tensor kind:", {k2: round(v, 4) for k2, v in sorted(worst.items())})
    assert all(x is None for x in c.other_grads), "memory, last_update and the feature tables take no gradient"
    names3 = [n for n in c.shapes if ".attention_models.2." in n or n.startswith("memory_updater.layer_norm")]
    assert names3 and not any(n in c.steps[-1][3] for n in names3)


@pytest.mark.parametrize("case", list(TT.CASES))
def test_state_after_four_steps(dev, case):
    g = TT.golden()
    c = golden_run(dev, case)
    pre = f"{case}_end_"
    assert np.array_equal(c.last_update.numpy(), g[pre + "last_update"])
    assert np.array_equal(c.pending["nodes"].numpy(), g[pre + "msg_nodes"])
    assert np.array_equal(c.pending["ts"].numpy(), g[pre + "msg_ts"])
    rows = g[pre + "mem_rows"]
    assert np.array_equal(np.nonzero(c.memory.abs().sum(1).numpy())[0], rows)
    mem_tol = max(1e-5, 10 * float(g[pre + "mem_env"]))
    raw_tol = max(1e-5, 10 * float(g[pre + "msg_raw_env"]))
    mem_err = float(np.abs(c.memory.numpy()[rows] - g[pre + "mem32"]).max())
    raw_err = float(np.abs(c.pending["raw"].numpy() - g[pre + "msg_raw32"]).max())
    print(case, "memory err", mem_err, "tol", mem_tol, "raw message err", raw_err, "tol", raw_tol)
    assert mem_err <= mem_tol and raw_err <= raw_tol
    # the frozen path (forbidden_memory_update=True, eval()) sees exactly that memory and those messages
    err = float(np.abs(c.frozen.numpy() - g[pre + "frozen64"]).max())
    print(case, "frozen logits err", err)
    np.testing.assert_allclose(c.frozen.numpy(), g[pre + "frozen64"], atol=LOGIT_ATOL, rtol=RTOL)


@pytest.mark.parametrize("case", list(TT.CASES))
def test_stateful_eval_pass(dev, case):
    """eval() / no_grad with forbidden_memory_update=False: no flag needed, no dropout, the memory moves on batch by
    batch as in the reference's eval_one_epoch."""
    g = TT.golden()
    m = TT.build_model(case, dropout=0.5).to(dev).eval()
    with torch.no_grad():
        for k, batch in enumerate(TT.step_batches()):
            pos, neg = m.contrast(*batch)
            assert not pos.requires_grad
            np.testing.assert_allclose(pos.cpu().numpy(), g[f"{case}_eval_s{k}_pos"], atol=LOGIT_ATOL, rtol=RTOL)
            np.testing.assert_allclose(neg.cpu().numpy(), g[f"{case}_eval_s{k}_neg"], atol=LOGIT_ATOL, rtol=RTOL)
    m.check_errors()
    # train() with gradients and without the flag is refused, not run on some other path
    m.train()
    with pytest.raises(NotImplementedError, match="train_on_hip"):
        m.contrast(*TT.step_batches()[0])


# ------------------------------------------------------------------ 3. dropout: the formulation with the same masks
@pytest.mark.parametrize("case,p", [("small8", 0.5), ("small10", 0.1)])
def test_steps_with_dropout_match_formulation(dev, case, p):
    """Three stateful steps with supplied keep masks against tests/tgn_train_ref.py (fp64 and fp32) with the same
    masks: from step 1 on the keys and queries read memory rows the message MLP and the GRU cell produced."""
    m = TT.build_model(case, dropout=p).to(dev)
    m.train_on_hip()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    batches = TT.step_batches()[:3]
    gen = torch.Generator(device=dev).manual_seed(17)
    keeps = [m.draw_keep_masks(3 * TT.STEP_B, TI.N_DEG, generator=gen) for _ in batches]
    frac = float(torch.cat([k.reshape(-1) for k in keeps[0]]).float().mean())
    assert abs(frac - (1 - p)) < 0.01
    scale = 1.0 / (1.0 - p)
    got = []
    for batch, keep in zip(batches, keeps):
        m.tgn_keep_masks = keep
        m.zero_grad(set_to_none=True)
        loss, pos, neg = bce_step(m, batch)
        assert m._tgn_train_key == (3 * TT.STEP_B, TI.N_DEG, True)
        got.append((loss, pos, neg, live_grads(m)))
    m.check_errors()
    kc = [[k.cpu() for k in keep] for keep in keeps]
    ref64 = TR.train_steps(TR.RefTGN(sd, TT.heads(case), torch.float64), batches, kc, scale)
    ref32 = TR.train_steps(TR.RefTGN(sd, TT.heads(case), torch.float32), batches, kc, scale)
    for k, (loss, pos, neg, grads) in enumerate(got):
        l64 = torch.cat([ref64[k][1], ref64[k][2]]).numpy().reshape(-1)
        mine = torch.cat([pos, neg]).double().cpu().numpy().reshape(-1)
        print(case, p, "step", k, "max |logit - fp64|", float(np.abs(mine - l64).max()))
        np.testing.assert_allclose(mine, l64, atol=LOGIT_ATOL, rtol=RTOL)
        g64 = {n: v for n, v in ref64[k][3].items() if v is not None and n in grads}
        assert set(g64) == set(grads)
        check_grads(grads, g64, ref32[k][3], tag=f"{case} p={p} s{k} ")


# ------------------------------------------------------------------ 4. the memory's methods and the dict
def test_backup_restore_reproduces_the_steps(dev):
    c = golden_run(dev, "small10")
    m = TT.build_model("small10").to(dev)
    m.train_on_hip()
    batches = TT.step_batches()
    for batch in batches[:2]:
        m.zero_grad(set_to_none=True)
        bce_step(m, batch)
    backup = m.memory.backup_memory()
    runs = []
    for _ in range(2):
        out = []
        for batch in batches[2:]:
            m.zero_grad(set_to_none=True)
            out.append(bce_step(m, batch) + (live_grads(m),))
        runs.append(out)
        state = (m.memory.memory.detach().clone(), m.memory.last_update.detach().clone(), m.memory.msg_raw.clone(),
                 m.memory.msg_flag.clone())
        runs[-1].append(state)
        m.memory.restore_memory(backup)
    for a, b in zip(runs[0][:-1], runs[1][:-1]):
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
        assert set(a[3]) == set(b[3]) and all(torch.equal(a[3][k], b[3][k]) for k in a[3])
    assert all(torch.equal(x, y) for x, y in zip(runs[0][-1], runs[1][-1]))
    # and they are the golden run's steps 2 and 3 (the same model, the same four slices)
    for a, ref in zip(runs[0][:-1], c.steps[2:]):
        assert torch.equal(a[1], ref[1]) and torch.equal(a[2], ref[2])
    # restored: the state of after step 1, not of after step 3
    assert not torch.equal(m.memory.msg_flag, runs[0][-1][3])


def test_messages_round_trip_through_the_dict(dev):
    c = golden_run(dev, "small8")
    m = c.model
    m.messages_to_dict()
    msgs = m.memory.messages
    assert sorted(k for k, v in msgs.items() if v) == c.pending["nodes"].tolist()
    assert all(len(v) == 1 for v in msgs.values())
    m2 = TT.build_model("small8").to(dev)
    m2.load_state_dict(m.state_dict(), strict=True)
    m2.memory.messages = {k: [(x[0].clone(), x[1].clone()) for x in v] for k, v in msgs.items()}
    m2.messages_from_dict()
    p2 = m2.pending_messages()
    assert torch.equal(p2["nodes"].cpu(), c.pending["nodes"]) and torch.equal(p2["raw"].cpu(), c.pending["raw"])
    m2.forbidden_memory_update = True
    m2.eval()
    with torch.no_grad():
        frozen2 = torch.cat(m2.contrast(*TT.full_batch())).cpu()
    assert torch.equal(frozen2, c.frozen)
    # one more stateful step from the store of each model: the same bits
    m2.forbidden_memory_update = False
    m.eval()
    with torch.no_grad():
        a = m.contrast(*TT.step_batches()[0])
        b = m2.contrast(*TT.step_batches()[0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _cache.pop(("golden", "small8"))          # this model's state has moved on


# ------------------------------------------------------------------ 5. end to end
def test_ten_adam_steps_follow_the_formulation(dev):
    """The (8, 4, H = 2) golden model, p = 0, ten Adam(lr = 1e-3) steps over the four slices in turn, stateful, the
    memory detached after every step: the losses follow the CPU formulation's (fp32, torch.optim.Adam) to four
    digits."""
    m = TT.build_model("small8").to(dev)
    m.train_on_hip()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    batches = TT.step_batches()
    losses = []
    for i in range(10):
        opt.zero_grad()
        loss, _, _ = bce_step(m, batches[i % 4])
        opt.step()
        losses.append(loss)
    losses = np.array([float(x) for x in torch.stack(losses).cpu()])
    ref = TR.RefTGN(sd, TT.heads("small8"), torch.float32)
    ropt = torch.optim.Adam(list(ref.trainable().values()), lr=1e-3)
    want = []
    for i in range(10):
        ref.zero_grad()
        loss = TR.bce(*ref.step(batches[i % 4]))
        loss.backward()
        ropt.step()
        want.append(float(loss.detach()))
    print("losses", losses.tolist(), "formulation", want)
    assert np.isfinite(losses).all()
    np.testing.assert_allclose(losses, np.array(want), rtol=1e-4, atol=0)
    moved = max(float((v.detach().cpu() - sd[k]).abs().max()) for k, v in m.named_parameters() if v.grad is not None)
    assert moved > 1e-3, "the parameters did not move"


def test_train_epoch_runs_and_reproduces(dev):
    """learn_base.train_epoch with a TGN on the uslegis fixture, 3 steps at bs = 32, N = 20, p = 0.1: finite losses,
    and the same seeds give the same bits."""
    import pandas as pd

    from tempme_amd import learn_base
    from tempme_amd.tgn import TGN
    G = os.path.join(TI.G, "data")
    g_df = pd.read_csv(os.path.join(G, "ml_uslegis_sampled.csv"))
    ef = np.load(os.path.join(G, "ml_uslegis_sampled.npy"))
    nf = np.load(os.path.join(G, "ml_uslegis_sampled_node.npy"))
    sp = learn_base.split_data(g_df, device=dev)
    idx = np.random.default_rng(0).permutation(len(sp.train_src_l))
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        m = TGN(nf, ef, n_neighbors=20, device=dev, n_layers=2, n_heads=2, dropout=0.1).to(dev)
        m.train_on_hip()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        out = learn_base.train_epoch(m, opt, sp.train_ngh_finder, sp.train_rand_sampler, sp.train_src_l, sp.train_dst_l,
                                     sp.train_ts_l, sp.train_e_idx_l, 32, idx_list=idx, max_steps=3, metrics=False)
        assert m._tgn_train_key == (3 * 32, 20, True)
        m.check_errors()
        assert int(m.memory.msg_flag.sum()) > 0 and m.memory.memory.grad_fn is None
        runs.append(out["loss"])
    print("losses", runs[0])
    assert len(runs[0]) == 3 and np.isfinite(runs[0]).all()
    assert runs[0] == runs[1]
