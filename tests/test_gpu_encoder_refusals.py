"""GPU: what the four encoder forwards refuse, and what they do with nothing to do.  tm_encoder_fwd_tab,
tm_encoder_pool_fwd, tm_encoder_train_fwd and tm_encoder_pool_train_fwd through tempme_amd._lib at the 2x3x7 shape
of test_gpu_enhance_train.py: each refusal returns its code, names the entry point in tm_last_error() and leaves the
output buffer as it was; a call over zero groups or zero events returns TM_OK and launches no kernel.

tm_encoder_fwd_tab shares its argument checks with tm_encoder_fwd and reports them under that name; its own name
stands on the refusal only it can give (a table at dims without a table mode)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
FORWARDS = ("tm_encoder_fwd_tab", "tm_encoder_pool_fwd", "tm_encoder_train_fwd", "tm_encoder_pool_train_fwd")
TAKES_M = ("tm_encoder_fwd_tab", "tm_encoder_pool_fwd")
POOLED = ("tm_encoder_pool_fwd", "tm_encoder_pool_train_fwd")


class Call:
    """One forward's argument list at the 2x3x7 shape, every pointer valid; run(**changes) replaces arguments by
    name and returns (code, tm_last_error(), the output buffer, {profile name: launches})."""

    def __init__(self, name, de=32):
        from tempme_amd import _lib as L
        from test_gpu_enhance_train import DEV, SHAPES, build
        self.L, self.name = L, name
        self.ex, d = build(shape=SHAPES["2x3x7"], de=de)
        self.ex.eval()
        node6, eid3, ts3, cat, cut, cnt, G, B, W = d["args"]
        n = G * B * W
        nt, et = self.ex.feature_tables()
        w = self.ex.packed_weights()
        pooled = name in POOLED
        size = L.lib().tm_encoder_pool_workspace_bytes if pooled else L.lib().tm_encoder_workspace_bytes
        self.keep = (nt, et, torch.ones(n, dtype=torch.float32, device=DEV),
                     torch.empty(size(w, n), dtype=torch.uint8, device=DEV))
        self.out = torch.full((G * B, self.ex.mlp_dim) if pooled else (n,), SENTINEL, dtype=torch.float32, device=DEV)
        a = dict(w=w, n_feat=L.ptr(nt), e_feat=L.ptr(et))
        if name in TAKES_M:
            a["etab"] = None
        a.update(n_groups=G, B=B, W=W)
        if name in TAKES_M:
            a["M"] = 1
        a.update(node6=L.ptr(node6), eid3=L.ptr(eid3), ts3=L.ptr(ts3), cat=L.ptr(cat), cut=L.ptr(cut), cnt=L.ptr(cnt))
        if pooled:
            a["wgt"] = L.ptr(self.keep[2])
        if name not in TAKES_M:
            a.update(drop=None, drop_scale=1.0)
        a.update(workspace=L.ptr(self.keep[3]), out=L.ptr(self.out))
        if pooled:
            a["ld_out"] = self.ex.mlp_dim
        a["stream"] = L.stream_ptr(DEV)
        self.args = a
        self.keep += (node6, eid3, ts3, cat, cut, cnt)

    def run(self, **changes):
        L = self.L
        assert set(changes) <= set(self.args), changes
        L.profile_enable(True)
        try:
            rc = getattr(L.lib(), self.name)(*dict(self.args, **changes).values())
            prof = L.profile_read()
        finally:
            L.profile_enable(False)
        torch.cuda.synchronize()
        return rc, L.lib().tm_last_error().decode(), self.out, {k: v[1] for k, v in prof.items()}


def refused(call, code, who, **changes):
    rc, msg, out, _ = call.run(**changes)
    assert rc == code, (call.name, changes, rc, msg)
    assert msg.startswith(who + ": "), (call.name, changes, msg)
    assert bool((out == SENTINEL).all()), (call.name, changes)


@pytest.mark.parametrize("name", FORWARDS)
def test_bad_arguments_are_refused(name):
    call = Call(name)
    L = call.L
    who = "tm_encoder_fwd" if name == "tm_encoder_fwd_tab" else name
    for p in ("n_feat", "node6", "cut", "workspace", "out") + (("wgt",) if name in POOLED else ()):
        refused(call, L.TM_E_ARG, who, **{p: None})
    refused(call, L.TM_E_ARG, who, w=None)
    refused(call, L.TM_E_ARG, who, B=-1)
    if name in TAKES_M:
        refused(call, L.TM_E_ARG, who, M=0)
        assert call.args["W"] % 2
        refused(call, L.TM_E_SHAPE, who, M=2)
    if name in POOLED:
        refused(call, L.TM_E_ARG, who, ld_out=call.ex.mlp_dim - 1)
    rc, _, out, _ = call.run()                      # and the unchanged list is a good call
    assert rc == L.TM_OK and not bool((out == SENTINEL).any())


@pytest.mark.parametrize("name", TAKES_M)
def test_table_without_table_mode_is_refused(name):
    call = Call(name, de=50)
    L = call.L
    assert L.lib().tm_edge_table_cols(call.args["w"]) == 0
    refused(call, L.TM_E_UNSUPPORTED, name, etab=L.ptr(call.keep[2]))


@pytest.mark.parametrize("name", FORWARDS)
def test_zero_sized_calls_launch_nothing(name):
    call = Call(name)
    for zero in ("n_groups", "B"):
        rc, _, out, launches = call.run(**{zero: 0})
        assert rc == call.L.TM_OK, (name, zero)
        assert not any(launches.values()), (name, zero, launches)
        assert bool((out == SENTINEL).all()), (name, zero)
