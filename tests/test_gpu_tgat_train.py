"""Base-TGAT training on the HIP path: the training pair of the attention kernels through the C ABI
(tm_tgat_attn_train_fwd / tm_tgat_attn_train_bwd, csrc/tgat_train.hip) against the plain kernels and an fp64
restatement; one training step of TGAT.train_on_hip against the reference-shaped torch formulation with the same
dropout masks (tests/tgat_train_ref.py) and against the reference's own step (tests/golden/tgat_train.npz); and,
end to end, learn_base.train_epoch with a TGAT.

Tolerances.  Kernel outputs: test_gpu_tgat._tol's rule (1e-5 of the tensor's largest element, at least 1); the test
inputs keep the scores O(1) at every d_key (qf ~ N(0, 1), temperature sqrt(d_key / H)).  d_time sums
-sin(u) dt dk over every slot, with dt up to 1e6 and terms of both signs, so its bound is taken of the sum of the
terms' magnitudes, computed by the restatement: 1e-6 of it, 17 fp32 unit roundoffs -- a term carries the rounding of
a score (8 fma and 6 butterfly steps, of which the running error is a few roundoffs of the summed magnitudes), expf
(2), the division by the softmax sum, three products, the hardware sine (1.8e-7 absolute, 3 roundoffs of a term's
magnitude) and the fp32 sums over the wave's <= 2 N slots and the four waves; the partials add in fp64.  Logits:
tgat_inputs.logit_atol's rule on the case's own fp32 / fp64 pair.  Parameter gradients: test_gpu_gm_train.check_grads,
||g_hip - g_64|| <= max(1e-4 ||g_64||, 10 ||g_32 - g_64||); where g_64 is identically zero the HIP gradient must be
exactly zero.
"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tgat_ref as R
import tgat_train_inputs as TT
import tgat_train_ref as TR
import tgn_inputs as TI

pytestmark = pytest.mark.gpu

RTOL = 1e-5
GUARD = 64            # guard floats on each side of every kernel output
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ fp64 restatement of the training pair
def pair_rows(Rr, H, seg):
    """Mask / weight row of pair (r, h): base + ((r - base) H + h) % seg inside the row's segment."""
    seg = seg or Rr
    r = torch.arange(Rr).view(Rr, 1)
    h = torch.arange(H).view(1, H)
    base = r - r % seg
    return base + ((r - base) * H + h) % seg


def train_attn_ref(x, keep, scale):
    """tests/tgat_ref.attn with the keep mask, and the backward in closed form (the formulas of csrc/attn_train.h in
    fp64).  x: node [R, N, dn], edge [R, N, de], dt [R, N], tw / tb [dt], qf / gz [R, H, dk], mask [R, N], ew [R, N]
    or None, T, seg; keep uint8 [R H N] or None.  Returns z, d_ew_parts [R, H, N], d_node, d_qf, d_time [2, dt] and
    the magnitude sums d_time's bound is taken from."""
    Rr, N, dn = x.node.shape
    de, H = x.edge.shape[2], x.qf.shape[1]
    key = R.keys(x.node, x.edge, x.dt, x.tw, x.tb)                         # [R, N, dk] fp64, fp32 arguments
    u = ((x.dt.float().unsqueeze(-1) * x.tw.float()) + x.tb.float()).double()
    m = pair_rows(Rr, H, x.seg)
    qf, gz = x.qf.double(), x.gz.double()
    s = torch.einsum("rhc,rjc->rhj", qf, key) / x.T
    masked = x.mask[m] == 0
    p = torch.softmax(s.masked_fill(masked, -1e10), dim=-1)
    kf = torch.ones(Rr, H, N, dtype=torch.float64) if keep is None else keep.view(Rr, H, N).double() * scale
    e = kf if x.ew is None else x.ew.double()[m] * kf
    z = torch.einsum("rhj,rjc->rhc", p * e, key)
    c = torch.einsum("rhc,rjc->rhj", gz, key)
    S = (p * e * c).sum(-1, keepdim=True)
    live = (~masked).double()
    ds = p * (e * c - S) * live
    dk = torch.einsum("rhj,rhc->rjc", p * e, gz) + torch.einsum("rhj,rhc->rjc", ds / x.T, qf)
    d_qf = torch.einsum("rhj,rjc->rhc", ds, key) / x.T
    sin_u = -torch.sin(u)
    dkt = dk[..., dn + de:]
    d_time = torch.stack([(sin_u * x.dt.double().unsqueeze(-1) * dkt).sum((0, 1)), (sin_u * dkt).sum((0, 1))])
    # magnitudes: every product and sum above with absolute values
    cabs = torch.einsum("rhc,rjc->rhj", gz.abs(), key.abs())
    Sabs = (p * e.abs() * cabs).sum(-1, keepdim=True)
    mag = torch.einsum("rhj,rhc->rjc", p * e.abs(), gz.abs()) + \
        torch.einsum("rhj,rhc->rjc", p * (e.abs() * cabs + Sabs) * live / x.T, qf.abs())
    magt = mag[..., dn + de:]
    mag_time = torch.stack([(x.dt.double().abs().unsqueeze(-1) * magt).sum((0, 1)), magt.sum((0, 1))])
    return SimpleNamespace(z=z, d_ew=p * c * kf, d_node=dk[..., :dn], d_qf=d_qf, d_time=d_time, mag_time=mag_time)


def _tol(ref):
    return 1e-5 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ 1. the kernels through the C ABI
# (rows, N, d_node, d_edge, d_time, H, seg_rows, dense node table, explanation weights)
KERNEL_CASES = [
    (15, 3, 8, 4, 8, 2, 0, False, True),          # one wave per row; rows no multiple of 4
    (21, 5, 24, 18, 24, 3, 0, False, True),       # split kernel; KPL = 2 with a ragged last register
    (8, 4, 30, 4, 30, 4, 0, False, False),        # d_key = 64 exactly; 4 heads
    (8, 4, 170, 172, 170, 4, 0, False, True),     # d_key = 512; KPL = 8
    (60, 20, 172, 32, 172, 2, 20, False, False),  # the golden dims, head-major in segments
    (21, 5, 24, 18, 24, 3, 7, True, False),       # pass 3's form: dense node_tab with the d_node output
    # more than 4 * 1024 rows: the backward's waves walk two rows each (per-wave LDS reused across rows, the time
    # sums carried in registers over rows, 513 / 1,023 partials through the reducer) -- what any batch of 69 or
    # more events takes in pass 2
    (4101, 4, 8, 4, 8, 2, 0, False, True),        # split forward; the last workgroup's second quad holds one row
    (8184, 3, 8, 4, 8, 2, 1023, True, False),     # dense table, one wave per row forward, 2 row quads per workgroup
]


def kernel_inputs(case, seed):
    Rr, N, dn, de, dtm, H, seg, dense, with_ew = case
    dk = dn + de + dtm
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen, dtype=torch.float64) * scale).float()
    x = SimpleNamespace(R=Rr, N=N, H=H, dk=dk, dims=(dn, de, dtm), seg=seg, dense=dense,
                        T=float(np.sqrt(dk / H)))
    x.node, x.edge = rnd(Rr, N, dn), rnd(Rr, N, de)
    x.dt = torch.floor(torch.rand(Rr, N, generator=gen, dtype=torch.float64) * 1e6).float()
    x.tw = (1.0 / 10 ** torch.linspace(0, 9, dtm)).float()
    x.tb = rnd(dtm, scale=0.5)
    x.qf, x.gz = rnd(Rr, H, dk), rnd(Rr, H, dk)
    x.mask = torch.randint(1, 9, (Rr, N), generator=gen, dtype=torch.int32)
    x.mask[torch.rand(Rr, N, generator=gen) < 0.25] = 0
    x.mask[3] = 0                                               # one row with no valid neighbour
    x.ew = torch.rand(Rr, N, generator=gen).float() if with_ew else None
    x.keep = (torch.rand(Rr * H * N, generator=gen) < 0.6).to(torch.uint8)
    x.keep.view(Rr, H, N)[2, H - 1] = 0                         # one (row, head) with every byte dropped
    x.scale = float(1.0 / 0.6)
    return x


def guarded(dev, *shape):
    """A NaN-filled device buffer with GUARD floats on both sides -> (buffer, view of the payload)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def run_train_pair(L, dev, x, t, keep, scale, gz=None, with_parts=True):
    """tm_tgat_attn_train_fwd + _bwd on guarded outputs -> namespace of the payload views (and the guards' state)."""
    dn, de, dtm = x.dims
    a = describe(L, x, t)
    st = L.stream_ptr(dev)
    o = SimpleNamespace()
    bufs = {}
    for name, shape in (("z", (x.R, x.H * x.dk)), ("stats", (x.R, x.H, 2)), ("parts", (x.R * x.H, x.N)),
                        ("d_node", (x.R * x.N, dn)), ("d_qf", (x.R, x.H * x.dk)), ("d_time", (2, dtm))):
        bufs[name], view = guarded(dev, *shape)
        setattr(o, name, view)
    ws_bytes = int(L.lib().tm_tgat_attn_train_workspace_bytes(x.R, dtm))
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    bufs["ws"], ws = guarded(dev, ws_bytes // 4)
    L.check(L.lib().tm_tgat_attn_train_fwd(C.byref(a), L.ptr(keep), scale, L.ptr(o.z), L.ptr(o.stats), st))
    L.check(L.lib().tm_tgat_attn_train_bwd(C.byref(a), L.ptr(keep), scale, L.ptr(o.stats),
                                           L.ptr(t["gz"] if gz is None else gz), L.ptr(o.parts) if with_parts else None,
                                           L.ptr(o.d_node) if x.dense else None, L.ptr(o.d_qf), L.ptr(o.d_time),
                                           L.ptr(ws), st))
    torch.cuda.synchronize()
    o.guards = all(guards_intact(b) for b in bufs.values())
    return o


def describe(L, x, t):
    dn, de, dtm = x.dims
    a = L.TgatAttn()
    a.rows, a.n_ngh, a.n_head = x.R, x.N, x.H
    a.d_node, a.d_edge, a.d_time = dn, de, dtm
    a.head_major_rows, a.seg_rows = 1, x.seg
    a.temperature = x.T
    if x.dense:
        a.node_tab, a.node_idx, a.node_rows = t["node"].data_ptr(), None, 0
    else:
        a.node_tab, a.node_idx, a.node_rows = t["node"].data_ptr(), t["node_idx"].data_ptr(), x.R * x.N
    a.edge_tab, a.edge_idx, a.edge_rows = t["edge"].data_ptr(), None, 0
    a.dt, a.time_w, a.time_b = t["dt"].data_ptr(), t["tw"].data_ptr(), t["tb"].data_ptr()
    a.mask_node, a.qf = t["mask"].data_ptr(), t["qf"].data_ptr()
    a.ew = t["ew"].data_ptr() if x.ew is not None else None
    a.err_flag = t["err"].data_ptr()
    return a


def device_inputs(dev, x):
    t = {k: getattr(x, k).to(dev).contiguous() for k in ("node", "edge", "dt", "tw", "tb", "qf", "gz", "mask", "keep")}
    if x.ew is not None:
        t["ew"] = x.ew.to(dev).contiguous()
    # the gathered form reads the same rows through an index (a permutation of a permuted table)
    if not x.dense:
        perm = torch.randperm(x.R * x.N, generator=torch.Generator().manual_seed(7))
        tab = torch.empty(x.R * x.N, x.dims[0])
        tab[perm] = x.node.reshape(x.R * x.N, -1)
        t["node"], t["node_idx"] = tab.to(dev).contiguous(), perm.to(torch.int32).to(dev)
    t["err"] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_train_kernels(dev, case):
    from tempme_amd import _lib as L
    x = kernel_inputs(case, seed=sum(int(v) for v in case))
    t = device_inputs(dev, x)
    st = L.stream_ptr(dev)
    dn = x.dims[0]
    # keep = NULL: the plain kernels' bits
    o0 = run_train_pair(L, dev, x, t, None, 1.0)
    a = describe(L, x, t)
    z = torch.empty(x.R, x.H * x.dk, device=dev)
    stats = torch.empty(x.R, x.H, 2, device=dev)
    parts = torch.empty(x.R * x.H, x.N, device=dev)
    d_node = torch.empty(x.R * x.N, dn, device=dev) if x.dense else None
    d_qf = torch.empty(x.R, x.H * x.dk, device=dev)
    L.check(L.lib().tm_tgat_attn_fwd(C.byref(a), L.ptr(z), L.ptr(stats), st))
    L.check(L.lib().tm_tgat_attn_bwd(C.byref(a), L.ptr(stats), L.ptr(t["gz"]), L.ptr(parts), L.ptr(d_node),
                                     L.ptr(d_qf), st))
    assert o0.guards
    assert torch.equal(o0.z, z) and torch.equal(o0.stats, stats)
    assert torch.equal(o0.parts, parts) and torch.equal(o0.d_qf, d_qf)
    if x.dense:
        assert torch.equal(o0.d_node, d_node)
    # with the mask: the fp64 restatement
    ref = train_attn_ref(x, x.keep, x.scale)
    o = run_train_pair(L, dev, x, t, t["keep"], x.scale)
    assert o.guards and int(t["err"].item()) == 0
    assert torch.equal(o.stats, stats), "stats hold the plain softmax's max and sum"
    checks = [("z", o.z.view(x.R, x.H, x.dk), ref.z), ("d_ew_parts", o.parts.view(x.R, x.H, x.N), ref.d_ew),
              ("d_qf", o.d_qf.view(x.R, x.H, x.dk), ref.d_qf)]
    if x.dense:
        checks.append(("d_node", o.d_node.view(x.R, x.N, dn), ref.d_node))
    for name, got, want in checks:
        err = (got.cpu().double() - want).abs().max().item()
        print(case, name, "max err", err, "tol", _tol(want))
        assert torch.isfinite(got).all(), name
        assert err <= _tol(want), name
    err = (o.d_time.cpu().double() - ref.d_time).abs()
    bound = 1e-6 * ref.mag_time
    print(case, "d_time worst err / bound", float((err / bound).max()), "|d_time| max", float(ref.d_time.abs().max()))
    assert torch.isfinite(o.d_time).all() and bool((err <= bound).all())
    # a second launch: the same bits, the time gradient included
    o2 = run_train_pair(L, dev, x, t, t["keep"], x.scale)
    for name in ("z", "parts", "d_qf", "d_time"):
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


def test_train_kernel_limits_are_refused(dev):
    from tempme_amd import _lib as L
    x = kernel_inputs(KERNEL_CASES[0], seed=1)
    t = device_inputs(dev, x)
    buf = torch.empty(4096, device=dev)
    st = L.stream_ptr(dev)
    for change, code in ((dict(n_head=5), L.TM_E_UNSUPPORTED), (dict(d_node=300, d_time=300), L.TM_E_UNSUPPORTED),
                         (dict(n_ngh=400), L.TM_E_UNSUPPORTED), (dict(n_ngh=0), L.TM_E_ARG)):
        a = describe(L, x, t)
        for k, v in change.items():
            setattr(a, k, v)
        assert L.lib().tm_tgat_attn_train_fwd(C.byref(a), None, 1.0, L.ptr(buf), L.ptr(buf), st) == code
        assert L.lib().tm_tgat_attn_train_bwd(C.byref(a), None, 1.0, L.ptr(buf), L.ptr(buf), None, None, L.ptr(buf),
                                              L.ptr(buf), L.ptr(buf), st) == code
        assert L.lib().tm_last_error()
    assert L.lib().tm_tgat_attn_train_workspace_bytes(-1, 8) == -1


# ------------------------------------------------------------------ 2. one training step of the model
# B, N, d_node, d_edge, H, p
SHAPES = [(5, 3, 8, 4, 2, 0.5), (7, 5, 24, 18, 3, 0.1), (4, 20, 172, 32, 2, 0.1), (6, 4, 30, 4, 4, 0.0)]


def bce_step(model, batch):
    p, n = model.contrast(batch[0], batch[1], batch[2], batch[3], None, *batch[4:], if_explain=False)
    crit = torch.nn.functional.binary_cross_entropy_with_logits
    loss = crit(p, torch.ones_like(p)) + crit(n, torch.zeros_like(n))
    loss.backward()
    return loss.detach(), p.detach(), n.detach()


def grads_of(model):
    return {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in model.named_parameters()
            if v.requires_grad}


def synth_batch(rng, B, N, V, E):
    """test_gpu_gm_train's generator for 2-hop subgraphs: padding neighbours at rate 0.25 (a padding node's own
    neighbours are padding), row 1 with no valid neighbour, dt = floor(U[0, 1e6)) per hop, padding records 0."""
    cut = np.floor(rng.uniform(5e7, 1e8, B))
    sgs = []
    for _ in range(3):
        n1 = rng.integers(1, V, (B, N))
        n1[rng.uniform(size=n1.shape) < 0.25] = 0
        n1[1] = 0
        n2 = rng.integers(1, V, (B, N, N))
        n2[rng.uniform(size=n2.shape) < 0.25] = 0
        n2[n1 == 0] = 0
        e1 = np.where(n1 > 0, rng.integers(1, E + 1, n1.shape), 0)
        e2 = np.where(n2 > 0, rng.integers(1, E + 1, n2.shape), 0)
        t1 = np.where(n1 > 0, cut[:, None] - np.floor(rng.uniform(0, 1e6, n1.shape)), 0.0)
        t2 = np.where(n2 > 0, t1[:, :, None] - np.floor(rng.uniform(0, 1e6, n2.shape)), 0.0)
        f = np.float64
        sgs.append(([n1.astype(f), n2.reshape(B, N * N).astype(f)], [e1.astype(f), e2.reshape(B, N * N).astype(f)],
                    [t1, t2.reshape(B, N * N)]))
    src, dst, fake = (rng.integers(1, V, B) for _ in range(3))
    return (src, dst, fake, cut, *sgs)


def make_case(dev, B, N, dn, de, H, p):
    """One HIP training step with supplied masks, a second identical one, and the fp64 / fp32 reference-shaped
    formulation with the same masks on the CPU.  Computed once per shape."""
    key = (B, N, dn, de, H, p)
    if key in _cache:
        return _cache[key]
    from tempme_amd.tgat import TGAT
    rng = np.random.default_rng(B + N + dn + H)
    V, E = 300, 2000
    nf = rng.uniform(0, 1, (V, dn)).astype(np.float32)
    ef = rng.uniform(0, 1, (E + 1, de)).astype(np.float32)
    nf[0] = ef[0] = 0
    torch.manual_seed(N + H)
    m = TGAT(nf, ef, N, num_layers=2, n_head=H, drop_out=p)
    with torch.no_grad():
        m.time_encoder.phase.data.copy_(torch.from_numpy(rng.normal(0, 0.5, dn).astype(np.float32)))
    m = m.to(dev)
    batch = synth_batch(rng, B, N, V, E)
    c = SimpleNamespace(model=m, batch=batch, H=H, p=p, B=B, N=N)
    c.sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m.eval()
    with torch.no_grad():
        c.eval_before = torch.cat(m.contrast(batch[0], batch[1], batch[2], batch[3], None, *batch[4:]))
    # the flag off: training mode with dropout is refused as before; without dropout the frozen path runs
    m.train()
    c.off_error = None
    try:
        pos, _ = m.contrast(batch[0], batch[1], batch[2], batch[3], None, *batch[4:])
        c.off_requires_grad = pos.requires_grad
    except NotImplementedError as exc:
        c.off_error = exc
    c.off_marker = getattr(m, "_tgat_train_key", None)
    m.train_on_hip()
    c.keep = m.draw_keep_masks(3 * B, N, generator=torch.Generator(device=dev).manual_seed(N + dn)) if p > 0 else None
    c.scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    m.tgat_keep_masks = c.keep
    c.loss, c.pos, c.neg = bce_step(m, batch)
    c.marker = getattr(m, "_tgat_train_key", None)
    c.grads = grads_of(m)
    m.zero_grad(set_to_none=True)
    c.loss2, c.pos2, c.neg2 = bce_step(m, batch)
    c.grads2 = grads_of(m)
    m.zero_grad(set_to_none=True)
    m.check_errors()
    m.eval()
    with torch.no_grad():
        c.eval_after = torch.cat(m.contrast(batch[0], batch[1], batch[2], batch[3], None, *batch[4:]))
    m.train()
    kc = None if c.keep is None else [k.cpu() for k in c.keep]
    c.ref64 = TR.loss_and_grads(c.sd, H, batch, kc, c.scale, torch.float64)
    c.ref32 = TR.loss_and_grads(c.sd, H, batch, kc, c.scale, torch.float32)
    _cache[key] = c
    return c


def check_grads(grads, g64, g32, tag=""):
    """test_gpu_gm_train.check_grads: per parameter tensor ||g_hip - g_64|| <= max(1e-4 ||g_64||,
    10 ||g_32 - g_64||); an identically zero g_64 wants an exactly zero HIP gradient.  Returns the worst ratio to
    the bound per tensor kind."""
    worst = {}
    for k, ref in g64.items():
        assert grads.get(k) is not None, f"{tag}{k}: no gradient"
        got = grads[k].double().cpu()
        ref = ref.double()
        err = float(torch.linalg.norm(got - ref))
        nref = float(torch.linalg.norm(ref))
        kind = ".".join(x for x in k.split(".") if not x.isdigit())
        if nref == 0.0:
            print(f"{tag}{k}: identically zero, |g_hip| max {float(got.abs().max()):.3e}")
            assert float(got.abs().max()) == 0.0, (tag, k)
            continue
        bound = max(1e-4 * nref, 10 * float(torch.linalg.norm(g32[k].double() - ref)))
        worst[kind] = max(worst.get(kind, 0.0), err / bound)
        print(f"{tag}{k}: err {err:.3e} bound {bound:.3e} |g64| {nref:.3e}")
        assert err <= bound, (tag, k, err, bound)
    return worst


def ids(s):
    return "-".join(str(v) for v in s)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_logits_match_fp64_formulation(dev, shape):
    c = make_case(dev, *shape)
    l64 = torch.cat([c.ref64[1], c.ref64[2]]).numpy()
    l32 = torch.cat([c.ref32[1], c.ref32[2]]).double().numpy()
    atol = 10.0 * max(float(np.abs(l32 - l64).max()), 2e-6)
    got = torch.cat([c.pos, c.neg]).double().cpu().numpy()
    print("max |logit - fp64|", float(np.abs(got - l64).max()), "atol", atol)
    np.testing.assert_allclose(got, l64, atol=atol, rtol=RTOL)
    np.testing.assert_allclose(float(c.loss), float(c.ref64[0]), atol=atol, rtol=RTOL)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parameter_gradients_match_fp64_formulation(dev, shape):
    c = make_case(dev, *shape)
    worst = check_grads(c.grads, c.ref64[3], c.ref32[3])
    print("worst err / bound per tensor kind:", {k: round(v, 4) for k, v in sorted(worst.items())})


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_all_36_parameters_have_a_gradient(dev, shape):
    c = make_case(dev, *shape)
    # 2 x 15 in attn_model_list (w_qs, w_ks, w_vs, fc and layer_norm with their biases, the merger's four Linears),
    # 4 in affinity_score, basis_freq and phase: the 36 the reference's own step fills (tgat_train.npz)
    assert len(c.grads) == 36
    assert sum(k.startswith("attn_model_list.") for k in c.grads) == 30
    assert sum(k.startswith("affinity_score.") for k in c.grads) == 4
    assert {"time_encoder.basis_freq", "time_encoder.phase"} <= set(c.grads)
    for k, g in c.grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        assert g.shape == c.sd[k].shape
    assert c.model.n_feat_th.grad is None and c.model.e_feat_th.grad is None


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_second_step_is_bitwise_equal(dev, shape):
    c = make_case(dev, *shape)
    assert torch.equal(c.loss, c.loss2) and torch.equal(c.pos, c.pos2) and torch.equal(c.neg, c.neg2)
    for k, g in c.grads.items():
        assert torch.equal(g, c.grads2[k]), k


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_path_markers_and_untouched_paths(dev, shape):
    c = make_case(dev, *shape)
    assert c.off_marker is None, "train_on_hip is off by default"
    if c.p > 0:
        assert isinstance(c.off_error, NotImplementedError), "training with drop_out > 0 and the flag off must raise"
    else:
        assert c.off_error is None and not c.off_requires_grad      # the frozen path: no parameter gradient
    assert c.marker == (3 * c.B, c.N, c.p > 0), "the HIP training path did not run"
    assert torch.equal(c.eval_before, c.eval_after), "eval-mode contrast changed after train_on_hip()"
    # no_grad and explanation weights keep their paths
    m, b = c.model, c.batch
    before = m._tgat_train_key
    m._tgat_train_key = None
    if c.p == 0:
        with torch.no_grad():
            m.contrast(b[0], b[1], b[2], b[3], None, *b[4:])
        w = [(torch.rand(c.B, c.N, device=dev), torch.rand(c.B, c.N * c.N, device=dev)) for _ in range(3)]
        m.contrast(b[0], b[1], b[2], b[3], None, *b[4:], if_explain=True, exp_weights=[[w[0], w[1]], [w[0], w[2]]])
    else:
        with torch.no_grad(), pytest.raises(NotImplementedError):
            m.contrast(b[0], b[1], b[2], b[3], None, *b[4:])
    assert m._tgat_train_key is None
    m._tgat_train_key = before


# ------------------------------------------------------------------ 3. the reference's own step
@pytest.mark.parametrize("case", list(TT.CASES))
def test_reference_training_step_on_the_device(dev, case):
    """tests/golden/tgat_train.npz (.train(), drop_out 0, the golden batch): HIP loss and logits within the case's
    logit_atol, full gradients within max(1e-4 ||g_64||, 10 ||g_32 - g_64||) of the stored pair, and the
    Frobenius norms of the full-size matrices within the same bound of the stored norms."""
    g = TT.golden()
    m = TT.build_model(case).to(dev)
    m.train_on_hip()
    batch = TT.batch()
    loss, pos, neg = bce_step(m, batch)
    assert m._tgat_train_key == (3 * TI.BSZ, TI.N_DEG, False)
    l64, logits64, g64, n64 = TT.stored(g, case, "64")
    _, _, g32, n32 = TT.stored(g, case, "32")
    atol = TT.logit_atol(g, case)
    got = torch.cat([pos, neg]).double().cpu().numpy().reshape(-1)
    print(case, "max |logit - reference fp64|", float(np.abs(got - logits64).max()), "atol", atol)
    np.testing.assert_allclose(got, logits64, atol=atol, rtol=RTOL)
    np.testing.assert_allclose(float(loss), l64, atol=atol, rtol=RTOL)
    grads = grads_of(m)
    assert set(grads) == set(g64) | set(n64) and len(grads) == 36
    worst = check_grads(grads, g64, g32, tag=f"{case} ")
    for k, ref in n64.items():
        got_n = float(torch.linalg.norm(grads[k].double()))
        if ref == 0.0:
            assert float(grads[k].abs().max()) == 0.0, k
            continue
        bound = max(1e-4 * ref, 10 * abs(n32[k] - ref))
        print(f"{case} {k}: norm {got_n:.6e} stored {ref:.6e} bound {bound:.3e}")
        assert abs(got_n - ref) <= bound, (k, got_n, ref, bound)
    print("worst err / bound per tensor kind:", {k: round(v, 4) for k, v in sorted(worst.items())})


# ------------------------------------------------------------------ 4. end to end
def test_ten_adam_steps_lower_the_loss(dev):
    """The (24, 8, H = 2) golden model on the golden batch at p = 0, ten Adam(lr = 1e-3) steps: the last loss is
    below the first.  The reference-shaped formulation (tests/tgat_train_ref.py, fp32, torch.optim.Adam) does this
    on the CPU: 1.9563, 1.4681, 1.3691, 1.4013, 1.3967, 1.3753, 1.3647, 1.3656, 1.3724, 1.3732 -- a drop of 0.58,
    not monotone, so only first against last is asserted."""
    m = TT.build_model("small24").to(dev)
    m.train_on_hip()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    batch = TT.batch()
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss, _, _ = bce_step(m, batch)
        opt.step()
        losses.append(loss)
    losses = [float(x) for x in torch.stack(losses).cpu()]
    print("losses", losses)
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    # evaluation after training (learn_base.eval_one_epoch: eval mode, no_grad, the frozen pack rebuilt from the
    # updated parameters) gives the logits of the training path on the same weights (drop_out 0: the same function;
    # two fp32 evaluations that differ in the fold's precision, held to tgat_inputs.logit_atol's floor)
    moved = max(float((v.detach().cpu() - TT.build_model("small24").state_dict()[k]).abs().max())
                for k, v in m.named_parameters() if v.requires_grad)
    assert moved > 1e-3, "the parameters did not move"
    pos_t, neg_t = m.contrast(batch[0], batch[1], batch[2], batch[3], None, *batch[4:], if_explain=False)
    m.eval()
    with torch.no_grad():
        pos_e, neg_e = m.contrast(batch[0], batch[1], batch[2], batch[3], None, *batch[4:], if_explain=False)
    m.train()
    got, want = torch.cat([pos_e, neg_e]).cpu().numpy(), torch.cat([pos_t, neg_t]).detach().cpu().numpy()
    print("max |eval - train path| after the steps", float(np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=RTOL)


def test_train_epoch_runs_and_reproduces(dev):
    """learn_base.train_epoch with a TGAT on the uslegis fixture, 3 steps at bs = 32, N = 20, p = 0.1: finite
    losses, and the same seeds give the same bits."""
    import pandas as pd

    from tempme_amd import learn_base
    from tempme_amd.tgat import TGAT
    G = os.path.join(TI.G, "data")
    g_df = pd.read_csv(os.path.join(G, "ml_uslegis_sampled.csv"))
    ef = np.load(os.path.join(G, "ml_uslegis_sampled.npy"))
    nf = np.load(os.path.join(G, "ml_uslegis_sampled_node.npy"))
    sp = learn_base.split_data(g_df, device=dev)
    idx = np.random.default_rng(0).permutation(len(sp.train_src_l))
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        m = TGAT(nf, ef, 20, num_layers=2, n_head=3, drop_out=0.1).to(dev)   # model_dim 172 + 1 + 172 = 3 * 115
        m.train_on_hip()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        out = learn_base.train_epoch(m, opt, sp.train_ngh_finder, sp.train_rand_sampler, sp.train_src_l, sp.train_dst_l,
                                     sp.train_ts_l, sp.train_e_idx_l, 32, idx_list=idx, max_steps=3, metrics=False)
        assert m._tgat_train_key == (3 * 32, 20, True)
        m.check_errors()
        runs.append(out["loss"])
    print("losses", runs[0])
    assert len(runs[0]) == 3 and np.isfinite(runs[0]).all()
    assert runs[0] == runs[1]
