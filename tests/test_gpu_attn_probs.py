"""tm_tgn_attn_probs / tm_tgat_attn_probs (csrc/attn_probs.h) through the C ABI, both flavours, against the fp64
restatement tests/attn_probs_ref.py.  Every output sits between guard floats.

Shapes are the smallest at which each path of the kernels runs: 7 rows (two workgroups of the wave-per-row form, the
second partly filled) or 6 rows in two segments of 3; N = 3 (one wave per row), 5 (one row per workgroup, wave 0 gets
two neighbours), 70 (a lane's second trip over j in the softmax) and 4096 (the largest n_ngh the LDS rule admits);
H = 1..4 (the 2-head and the 4-head instance, each full and partly filled); key layouts from 12 to 576 columns.

Bounds.  Probabilities against fp64: 1e-5 absolute (a probability is at most 1, so this is the project's
1e-5 max(1, max |ref|)).  Row sums: 1 within 1e-6.  ``mean``: the head-ordered fp32 sum of ``probs`` divided by H, bit
for bit.  The tie to the model, sum_j probs[r,h,j] key[r,j] against tm_*_attn_fwd's z without weights:
1e-5 max(1, max |z|), the wide-key tests' bound on z.  Measured on an MI355X (all cases): worst |p - fp64| 2.0e-7
(0.02 of the bound), worst |row sum - 1| 1.7e-7, worst |z - sum p key| 5.8e-7 (0.025 of its bound).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_probs_ref as AP
import test_gpu_tgat_train as TGT

pytestmark = pytest.mark.gpu

LAYOUTS = [(5, 3, 4), (60, 3, 1), (40, 20, 5), (8, 0, 4), (172, 172, 172), (192, 192, 192)]
FLAVOURS = ("tgn", "tgat")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    return torch.device("cuda", 0)


def lid(d):
    return "x".join(str(v) for v in d)


def make_case(flavour, dims, N, H, rows=7, seg=0, head_major=True, node_gather=False, edge_gather=False, seed=0):
    dn, de, dtm = dims
    dk = dn + de + dtm
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen, dtype=torch.float64) * scale).float()
    x = SimpleNamespace(flavour=flavour, R=rows, N=N, H=H, dk=dk, dims=dims, seg=seg, head_major=head_major,
                        T=float(np.sqrt(dk / H)) if flavour == "tgat" else float(np.sqrt(dk)))
    x.node_idx = x.edge_idx = None
    if node_gather:
        x.node_tab = rnd(rows * N + 3, dn)
        x.node_idx = torch.randint(0, rows * N + 3, (rows, N), generator=gen, dtype=torch.int32)
        x.node = x.node_tab[x.node_idx.long()]
    else:
        x.node = x.node_tab = rnd(rows, N, dn)
    if edge_gather:
        x.edge_tab = rnd(rows * N + 5, de)
        x.edge_idx = torch.randint(0, rows * N + 5, (rows, N), generator=gen, dtype=torch.int32)
        x.edge = x.edge_tab[x.edge_idx.long()]
    else:
        x.edge = x.edge_tab = rnd(rows, N, de)
    x.dt = torch.rand(rows, N, generator=gen).float() * 50.0
    x.tw = (1.0 / 10 ** torch.linspace(0, 4, dtm)).float()
    x.tb = rnd(dtm, scale=0.5)
    x.qf = rnd(rows, H, dk)
    x.mask = torch.randint(1, 9, (rows, N), generator=gen, dtype=torch.int32)      # row 0 stays unmasked
    x.mask[1, 0] = 0
    x.mask[3] = 0                                                                  # a fully masked row
    x.mask[5, :N - 1] = 0                                                          # only the last neighbour live
    x.ew_junk = rnd(rows, N, scale=1e3)
    x.ew_junk[2, 1] = float("nan")
    return x


def device_inputs(dev, x):
    t = {k: getattr(x, k).to(dev).contiguous() for k in ("node_tab", "edge_tab", "dt", "tw", "tb", "qf", "mask",
                                                         "ew_junk")}
    for k in ("node_idx", "edge_idx"):
        t[k] = getattr(x, k).to(dev).contiguous() if getattr(x, k) is not None else None
    t["err"] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def describe(L, x, t, ew=None):
    a = L.Attn()
    a.rows, a.n_ngh, a.n_head = x.R, x.N, x.H
    a.d_node, a.d_edge, a.d_time = x.dims
    a.node_rows = t["node_tab"].shape[0] if t["node_idx"] is not None else 0
    a.edge_rows = t["edge_tab"].shape[0] if t["edge_idx"] is not None else 0
    a.head_major_rows, a.seg_rows = int(x.head_major), x.seg
    a.temperature = x.T
    a.node_tab = t["node_tab"].data_ptr()
    a.node_idx = t["node_idx"].data_ptr() if t["node_idx"] is not None else None
    a.edge_tab = t["edge_tab"].data_ptr() if x.dims[1] else None
    a.edge_idx = t["edge_idx"].data_ptr() if t["edge_idx"] is not None else None
    a.dt, a.time_w, a.time_b = t["dt"].data_ptr(), t["tw"].data_ptr(), t["tb"].data_ptr()
    a.mask_node, a.qf = t["mask"].data_ptr(), t["qf"].data_ptr()
    a.ew = ew.data_ptr() if ew is not None else None
    a.err_flag = t["err"].data_ptr()
    return a


def entry(L, x, name):
    return getattr(L.lib(), f"tm_{x.flavour}_attn_{name}")


def run_probs(L, dev, x, t, probs=True, mean=True, ew=None):
    """One launch on guarded outputs -> (probs view or None, mean view or None)."""
    a = describe(L, x, t, ew)
    bp, p = TGT.guarded(dev, x.R, x.H, x.N) if probs else (None, None)
    bm, m = TGT.guarded(dev, x.R, x.N) if mean else (None, None)
    L.check(entry(L, x, "probs")(C.byref(a), L.ptr(p), L.ptr(m), L.stream_ptr(dev)), "probs")
    torch.cuda.synchronize()
    for b in (bp, bm):
        assert b is None or TGT.guards_intact(b), "a store outside an output"
    return p, m


def check_case(dev, x, tag):
    from tempme_amd import _lib as L
    t = device_inputs(dev, x)
    key = AP.keys(x.flavour, x.node, x.edge, x.dt, x.tw, x.tb)
    ref = AP.probs(x.qf, key, x.mask, x.T, x.head_major, x.seg)
    p, m = run_probs(L, dev, x, t)
    assert int(t["err"].item()) == 0
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(m).all())
    pc = p.cpu()
    # against fp64
    err = float((pc.double() - ref).abs().max())
    rs = float((pc.double().sum(-1) - 1).abs().max())
    print(tag, "max |p - fp64|", err, "bound 1e-5; max |row sum - 1|", rs)
    assert err <= 1e-5
    assert rs <= 1e-6
    assert bool((pc >= 0).all())
    # the masks: a fully masked (row, head) is uniform, a masked slot of any other is 0, one live slot is 1
    pr = AP.pair_rows(x.R, x.H, x.head_major, x.seg)
    live = (x.mask != 0)[pr]                                              # [R, H, N]
    full = ~live.any(-1)
    assert bool(full.any()) and bool((pc[full] == (np.float32(1) / np.float32(x.N)).item()).all())
    assert bool((pc[~live & ~full.unsqueeze(-1)] == 0).all())
    single = live.sum(-1) == 1
    assert bool(single.any()) and bool((pc[single][:, x.N - 1] == 1).all())
    assert bool(live.all(-1).any())
    # mean: the head-ordered fp32 sum / H, bit for bit
    assert np.array_equal(m.cpu().numpy(), AP.head_mean32(pc.numpy()))
    # either output alone, a second launch, and junk explanation weights: the same bits
    p1, none = run_probs(L, dev, x, t, mean=False)
    assert none is None and torch.equal(p1, p)
    none, m1 = run_probs(L, dev, x, t, probs=False)
    assert none is None and torch.equal(m1, m)
    p2, m2 = run_probs(L, dev, x, t, ew=t["ew_junk"])
    assert torch.equal(p2, p) and torch.equal(m2, m)
    # the tie to the model: the forward's z without weights is sum_j p_j key_j
    a = describe(L, x, t)
    bz, z = TGT.guarded(dev, x.R, x.H * x.dk)
    bs, stats = TGT.guarded(dev, x.R, x.H, 2)
    L.check(entry(L, x, "fwd")(C.byref(a), L.ptr(z), L.ptr(stats), L.stream_ptr(dev)), "fwd")
    torch.cuda.synchronize()
    assert TGT.guards_intact(bz) and TGT.guards_intact(bs)
    zp = torch.einsum("rhj,rjc->rhc", pc.double(), key)
    zerr = float((z.cpu().double().view(x.R, x.H, x.dk) - zp).abs().max())
    ztol = 1e-5 * max(1.0, float(zp.abs().max()))
    print(tag, "max |z - sum p key|", zerr, "bound", ztol)
    assert zerr <= ztol
    return err, rs, zerr / ztol


# ------------------------------------------------------------------ 1. layouts x N x H, both flavours
@pytest.mark.parametrize("H", [1, 2, 3, 4])
@pytest.mark.parametrize("N", [3, 5, 70])
@pytest.mark.parametrize("dims", LAYOUTS, ids=lid)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_probs_match_fp64(dev, flavour, dims, N, H):
    x = make_case(flavour, dims, N, H, seed=1000 * N + 10 * H + dims[0] + (flavour == "tgn"))
    check_case(dev, x, (flavour, dims, N, H))


# ------------------------------------------------------------------ 2. gathers, pairing, segments
@pytest.mark.parametrize("rows,seg", [(7, 0), (6, 3)])
@pytest.mark.parametrize("head_major", [True, False])
@pytest.mark.parametrize("edge_gather", [False, True])
@pytest.mark.parametrize("node_gather", [False, True])
@pytest.mark.parametrize("N,H,dims", [(3, 2, (5, 3, 4)), (5, 3, (40, 20, 5))], ids=["N3-H2-12", "N5-H3-65"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_gathers_pairing_and_segments(dev, flavour, N, H, dims, node_gather, edge_gather, head_major, rows, seg):
    x = make_case(flavour, dims, N, H, rows=rows, seg=seg, head_major=head_major, node_gather=node_gather,
                  edge_gather=edge_gather, seed=7 * N + H + rows)
    check_case(dev, x, (flavour, dims, N, H, node_gather, edge_gather, head_major, rows, seg))


# ------------------------------------------------------------------ 3. the largest n_ngh
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_largest_n_ngh(dev, flavour):
    """n_ngh = 4096: a row's scores fill the 64 KiB the LDS rule admits, every lane makes 64 trips over j.  The
    normaliser is then a chain of 64 additions per lane and 6 butterfly steps, and a probability takes two more
    roundings: a row sum is held to 72 x 2^-24 = 4.3e-6 here (1e-6 is the bound of the N <= 70 cases)."""
    from tempme_amd import _lib as L
    x = make_case(flavour, (5, 3, 4), 4096, 3, rows=6, seed=3)
    t = device_inputs(dev, x)
    ref = AP.probs(x.qf, AP.keys(x.flavour, x.node, x.edge, x.dt, x.tw, x.tb), x.mask, x.T, x.head_major, x.seg)
    p, m = run_probs(L, dev, x, t)
    pc = p.cpu()
    err = float((pc.double() - ref).abs().max())
    rs = float((pc.double().sum(-1) - 1).abs().max())
    print(flavour, "N = 4096: max |p - fp64|", err, "max |row sum - 1|", rs)
    assert err <= 1e-5 and rs <= 72 * 2.0 ** -24
    assert np.array_equal(m.cpu().numpy(), AP.head_mean32(pc.numpy()))
    p2, m2 = run_probs(L, dev, x, t)
    assert torch.equal(p2, p) and torch.equal(m2, m)


# ------------------------------------------------------------------ 4. the inherited error flag
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_out_of_range_id_sets_the_flag(dev, flavour):
    from tempme_amd import _lib as L
    x = make_case(flavour, (5, 3, 4), 5, 2, node_gather=True, edge_gather=True, seed=11)
    x.node_idx[2, 1] = x.node_tab.shape[0]                      # one past the table: the kernel reads row 0
    x.node[2, 1] = x.node_tab[0]
    t = device_inputs(dev, x)
    p, _ = run_probs(L, dev, x, t)
    assert int(t["err"].item()) == L.TM_E_ARG
    ref = AP.probs(x.qf, AP.keys(x.flavour, x.node, x.edge, x.dt, x.tw, x.tb), x.mask, x.T, x.head_major, x.seg)
    assert float((p.cpu().double() - ref).abs().max()) <= 1e-5


# ------------------------------------------------------------------ 5. refusals and the empty input
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refusals_name_their_limit(dev, flavour):
    from tempme_amd import _lib as L
    lib = L.lib()
    st = L.stream_ptr(dev)
    x = make_case(flavour, (5, 3, 4), 5, 2, seed=1)
    t = device_inputs(dev, x)
    who = f"tm_{flavour}_attn_probs"
    fn = entry(L, x, "probs")
    buf = torch.empty(1 << 12, device=dev)

    def refused(a, code, text, probs=buf, mean=buf):
        rc = fn(C.byref(a), L.ptr(probs), L.ptr(mean), st)
        msg = lib.tm_last_error().decode()
        assert rc == code, (rc, msg)
        assert text in msg and who in msg, msg

    a = describe(L, x, t)
    a.d_node, a.d_edge, a.d_time = 300, 200, 77                 # 577
    refused(a, L.TM_E_UNSUPPORTED, "d_key > 576")
    a = describe(L, x, t)
    a.n_head = 5
    refused(a, L.TM_E_UNSUPPORTED, "n_head > 4")
    a = describe(L, x, t)
    a.n_ngh = 4097                                              # 4097 x 4 floats: past 64 KiB of LDS
    refused(a, L.TM_E_UNSUPPORTED, "n_ngh too large")
    a = describe(L, x, t)
    refused(a, L.TM_E_ARG, "NULL output", probs=None, mean=None)
    a = describe(L, x, t)
    a.rows, a.seg_rows = 7, 3
    refused(a, L.TM_E_SHAPE, "seg_rows")
    # rows = 0: TM_OK, nothing is launched or written
    a = describe(L, x, t)
    a.rows = 0
    bp, p = TGT.guarded(dev, 4)
    assert fn(C.byref(a), L.ptr(p), L.ptr(p), st) == L.TM_OK
    assert fn(C.byref(a), None, None, st) == L.TM_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(bp).all())
