"""GPU: what the encoder's training entry points refuse, and what they do with nothing to do.  tm_encoder_bwd,
tm_encoder_pool_bwd, tm_encoder_wgrad, tm_encoder_pool_wgrad, tm_explain_train_fwd, tm_explain_train_fwd_pad and
tm_explain_train_bwd through tempme_amd._lib at the 2x3x7 shape of test_gpu_enhance_train.py, on a workspace the
matching training forward filled: each refusal returns its code, names the entry point in tm_last_error() and
launches no kernel; a call over zero groups or zero events returns TM_OK and launches no kernel, and the three calls
that end in the weight-gradient driver then leave every gradient all zero.  No case passes a bad non-NULL pointer.

tm_explain_train_fwd_pad shares its checks with tm_explain_train_fwd and reports them under that name; its own name
stands on the NULL check of the four arguments only it takes."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
BWD = ("tm_encoder_bwd", "tm_encoder_pool_bwd")
WGRAD = ("tm_encoder_wgrad", "tm_encoder_pool_wgrad")
EXPL_FWD = ("tm_explain_train_fwd", "tm_explain_train_fwd_pad")
EXPL_BWD = "tm_explain_train_bwd"
POOLED = ("tm_encoder_pool_bwd", "tm_encoder_pool_wgrad")
CALLS = BWD + WGRAD + EXPL_FWD + (EXPL_BWD,)
SCORING_IO = ("imp", "dlogit", "M2", "dM2", "M1d", "dM1", "X")   # the pooled calls read none of these
N_HOP = 3


def r16(x):
    return -(-x // 16) * 16


class Call:
    """One entry point's argument list at the 2x3x7 shape, every pointer valid; run(**changes) replaces arguments
    by name (io_without: these fields of the io block NULL; grads_without: that entry of grads NULL) and returns
    (code, tm_last_error(), {profile name: launches})."""

    def __init__(self, name):
        from tempme_amd import _lib as L
        from tempme_amd import explainer as X
        from test_gpu_enhance_train import DEV, SHAPES, build
        self.L, self.name = L, name
        ex, d = build(shape=SHAPES["2x3x7"])
        self.ex = ex
        node6, eid3, ts3, cat, cut, cnt, G, B, W = d["args"]
        n, st = G * B * W, L.stream_ptr(DEV)
        nt, et = ex.feature_tables()
        w = ex.packed_weights()
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)  # noqa: E731
        g = torch.Generator().manual_seed(1)
        rnd = lambda *s: torch.rand(*s, generator=g).to(DEV)  # noqa: E731
        self.keep = [nt, et, node6, eid3, ts3, cat, cut, cnt]
        if name in BWD + WGRAD:
            pooled = name in POOLED
            wgt = torch.ones(n, dtype=torch.float32, device=DEV)
            _, ws = ex._pool_train_fwd(d["args"], wgt, None, 1.0) if pooled else ex._train_fwd(d["args"], None, 1.0)
            # tm_encoder_grad_io's buffers (include/tempme.h) at n walks, R = 3 n walk positions
            h, R, KM = ex.hid_dim, 3 * n, r16(ex.mlp_dim)
            KE, DN = r16(ex.edge_dim + 3 + ex.node_dim), r16(ex.node_dim)
            self.io = dict(imp=e(n), dlogit=e(n), M2=e(n, h), dM2=e(n, h), M1d=e(n, KM), dM1=e(n, KM), X=e(n, KM),
                           dY2=e(n, h), H1d=e(n, h), dH1=e(n, h), O=e(n, 2 * h), dP=e(n, 2 * h), dQ=e(2, n, 2 * h),
                           dF=e(n, 3, 2 * h), ev=e(R, KE), AB=e(R, 2, DN), H=e(R, 2, h), dZ=e(R, 2, h), dlev=e(R, DN),
                           g=e(R, DN), dt=e(R))
            assert tuple(self.io) == L.GRAD_IO_FIELDS
            self.io_type = L.EncoderGradIO
            up = rnd(G, B, ex.mlp_dim) if pooled else rnd(n)
            bwd = dict(w=w, n_feat=L.ptr(nt), e_feat=L.ptr(et), n_groups=G, B=B, W=W, node6=L.ptr(node6),
                       eid3=L.ptr(eid3), ts3=L.ptr(ts3), cat=L.ptr(cat), cut=L.ptr(cut), cnt=L.ptr(cnt))
            if pooled:
                bwd["wgt"] = L.ptr(wgt)
            bwd.update(drop=None, drop_scale=1.0, workspace=L.ptr(ws))
            bwd.update(dict(d_emb=L.ptr(up), ld_demb=ex.mlp_dim) if pooled else dict(d_imp=L.ptr(up)))
            bwd.update(io=True, stream=st)
            self.keep += [wgt, ws, up]
            self.args = bwd
            if name in WGRAD:   # the weight gradients read what the backward left in io
                rc, msg, _ = self.run(name=BWD[pooled])
                assert rc == L.TM_OK, msg
                self.grads = [e(*s) for s in ex._padded_shapes(X._POOL_IDX if pooled else X._ENC_IDX)]
                self.args = dict(w=w, n_groups=G, B=B, W=W, io=True, workspace=L.ptr(ws), grads=True, stream=st)
        else:
            N = N_HOP
            rows = G * B
            imp = 0.1 + rnd(n)
            s1e = torch.randint(0, 90, (rows, N), generator=g, dtype=torch.int32).to(DEV)
            s2e = torch.randint(0, 90, (rows, N * N), generator=g, dtype=torch.int32).to(DEV)
            s1n = torch.randint(0, 3, (rows, N), generator=g, dtype=torch.int32).to(DEV)
            s2n = torch.randint(0, 3, (rows, N * N), generator=g, dtype=torch.int32).to(DEV)
            self.io, _ = ex._expl_io(rows * 3 * W)
            assert tuple(self.io) == L.EXPL_IO_FIELDS
            self.io_type = L.ExplainGradIO
            self.out = [torch.full(s, SENTINEL, dtype=torch.float32, device=DEV)
                        for s in ((rows, N), (rows, N * N), (rows, N), (rows, N * N))]
            p1, p2, pad1, pad2 = self.out
            fwd = dict(w=w, e_feat=L.ptr(et), n_groups=G, B=B, W=W, N=N, eid3=L.ptr(eid3), ts3=L.ptr(ts3),
                       imp=L.ptr(imp), sub1_eid=L.ptr(s1e), sub2_eid=L.ptr(s2e), keep1=None, keep2=None, scale1=1.0,
                       scale2=1.0, io=True, p1=L.ptr(p1), p2=L.ptr(p2))
            if name != EXPL_FWD[0]:
                fwd.update(sub1_node=L.ptr(s1n), sub2_node=L.ptr(s2n), pad1=L.ptr(pad1), pad2=L.ptr(pad2))
            fwd["stream"] = st
            self.keep += [imp, s1e, s2e, s1n, s2n]
            self.args = fwd
            if name == EXPL_BWD:   # the backward reads the gate the forward left in io
                rc, msg, _ = self.run(name=EXPL_FWD[1])
                assert rc == L.TM_OK, msg
                dp1, dp2, self.d_imp = rnd(rows, N), rnd(rows, N * N), e(n)
                self.grads = [e(*s) for s in ex._padded_shapes(X._GATE_IDX)]
                self.keep += [dp1, dp2]
                self.args = dict(w=w, n_groups=G, B=B, W=W, N=N, eid3=L.ptr(eid3), ts3=L.ptr(ts3), imp=L.ptr(imp),
                                 sub1_eid=L.ptr(s1e), sub2_eid=L.ptr(s2e), keep1=None, keep2=None, scale1=1.0,
                                 scale2=1.0, dp1=L.ptr(dp1), dp2=L.ptr(dp2), io=True, d_imp=L.ptr(self.d_imp),
                                 grads=True, stream=st)

    def run(self, name=None, io_without=(), grads_without=None, **changes):
        L = self.L
        assert set(changes) <= set(self.args), changes
        a = dict(self.args, **changes)
        if a["io"] is True:
            io = self.io_type(*[None if k in io_without else self.io[k].data_ptr() for k in self.io])
            a["io"] = C.byref(io)
        if a.get("grads") is True:
            a["grads"] = (C.c_void_p * len(self.grads))(*[None if i == grads_without else t.data_ptr()
                                                          for i, t in enumerate(self.grads)])
        L.profile_enable(True)
        try:
            rc = getattr(L.lib(), name or self.name)(*a.values())
            prof = L.profile_read()
        finally:
            L.profile_enable(False)
        torch.cuda.synchronize()
        return rc, L.lib().tm_last_error().decode(), {k: v[1] for k, v in prof.items()}


def refused(call, who, what="", **changes):
    rc, msg, launches = call.run(**changes)
    assert rc == call.L.TM_E_ARG, (call.name, changes, rc, msg)
    assert msg.startswith(who + ": " + what), (call.name, changes, msg)
    assert not any(launches.values()), (call.name, changes, launches)


def good(call, **changes):
    rc, msg, launches = call.run(**changes)
    assert rc == call.L.TM_OK, (call.name, changes, msg)
    assert any(launches.values()), (call.name, changes)
    return launches


@pytest.mark.parametrize("name", BWD)
def test_backward_refuses_bad_arguments(name):
    call = Call(name)
    pooled = name in POOLED
    for p in ("w", "io"):
        refused(call, name, "bad arguments", **{p: None})
    refused(call, name, "bad arguments", B=-1)
    for p in ("n_feat", "node6", "ts3", "cut", "workspace") + (("wgt", "d_emb") if pooled else ("d_imp",)):
        refused(call, name, "NULL pointer", **{p: None})
    refused(call, name, "NULL output buffer", io_without=("dY2",))
    refused(call, name, "NULL output buffer", io_without=("dt",))
    if pooled:
        # ld_demb is tested before the NULL pointers
        refused(call, name, "ld_demb below hid_dim", ld_demb=call.ex.hid_dim - 1)
        refused(call, name, "ld_demb below hid_dim", ld_demb=call.ex.hid_dim - 1, n_feat=None)
        launches = good(call, io_without=SCORING_IO)     # the scoring MLP's buffers and imp take no part
        assert launches == {"head_pool_bwd_kernel": 1, "gcn_bwd_kernel": 1}
    else:
        refused(call, name, "NULL output buffer", io_without=("dlogit",))
        good(call, io_without=("imp",))                  # imp is optional
    launches = good(call)                                # and the unchanged list is a good call
    assert launches == {"head_pool_bwd_kernel" if pooled else "head_bwd_kernel": 1, "gcn_bwd_kernel": 1}


@pytest.mark.parametrize("name", WGRAD)
def test_weight_gradients_refuse_bad_arguments(name):
    call = Call(name)
    for p in ("w", "io", "workspace", "grads"):
        refused(call, name, "bad arguments", **{p: None})
    refused(call, name, "bad arguments", B=-1)
    refused(call, name, "NULL gradient 0", grads_without=0)
    last = len(call.grads) - 1
    refused(call, name, "NULL gradient %d" % last, grads_without=last)
    refused(call, name, "bad job 7", io_without=("dY2",))          # a NULL required io field: attention.MLP.3's job
    if name in POOLED:
        assert len(call.grads) == 16
        good(call, io_without=SCORING_IO)
    else:
        assert len(call.grads) == 22
        refused(call, name, "bad job 10", io_without=("dlogit",))
    assert good(call) == {"wgrad_partial_kernel": 1, "wgrad_reduce_kernel": 1}


@pytest.mark.parametrize("name", EXPL_FWD)
def test_explain_forward_refuses_bad_arguments(name):
    call = Call(name)
    who = EXPL_FWD[0]                                   # the shared checks carry the plain entry point's name
    for p in ("w", "io"):
        refused(call, who, "bad arguments", **{p: None})
    for ch in (dict(B=-1), dict(W=0), dict(N=0)):
        refused(call, who, "bad arguments", **ch)
    for p in ("e_feat", "eid3", "ts3", "imp", "sub2_eid", "p1"):
        refused(call, who, "NULL pointer", **{p: None})
    refused(call, who, "NULL pointer", io_without=("gate",))
    if name != who:
        for p in ("sub1_node", "sub2_node", "pad1", "pad2"):
            refused(call, name, "NULL pointer", **{p: None})
        refused(call, name, "NULL pointer", sub1_node=None, w=None)   # _pad's own check comes first
    assert all(bool((o == SENTINEL).all()) for o in call.out)
    assert good(call) == {"gate_train_fwd_kernel": 1, "explain_train_kernel": 1}
    filled = call.out if name != who else call.out[:2]
    assert not any(bool((o == SENTINEL).any()) for o in filled)


def test_explain_backward_refuses_bad_arguments():
    call = Call(EXPL_BWD)
    for p in ("w", "io", "grads"):
        refused(call, EXPL_BWD, "bad arguments", **{p: None})
    for ch in (dict(B=-1), dict(W=0), dict(N=0)):
        refused(call, EXPL_BWD, "bad arguments", **ch)
    assert len(call.grads) == 8
    refused(call, EXPL_BWD, "NULL gradient 7", grads_without=7)
    for p in ("eid3", "imp", "sub1_eid", "dp2", "d_imp"):
        refused(call, EXPL_BWD, "NULL pointer", **{p: None})
    refused(call, EXPL_BWD, "NULL pointer", io_without=("dG1",))
    assert good(call) == {"explain_train_bwd_kernel": 1, "gate_train_bwd_kernel": 1, "wgrad_partial_kernel": 1,
                          "wgrad_reduce_kernel": 1}


@pytest.mark.parametrize("name", CALLS)
def test_zero_sized_calls_launch_nothing(name):
    call = Call(name)
    grads = getattr(call, "grads", None)
    for zero in ("n_groups", "B"):
        for t in grads or ():
            t.fill_(SENTINEL)
        rc, msg, launches = call.run(**{zero: 0})
        assert rc == call.L.TM_OK, (name, zero, msg)
        assert not any(launches.values()), (name, zero, launches)
        for i, t in enumerate(grads or ()):             # no rows: every gradient is zero
            assert bool((t == 0).all()), (name, zero, i)
