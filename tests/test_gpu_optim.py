"""FusedAdam (tempme_amd/optim.py, csrc/optim.hip tm_adam_step): torch.optim.Adam's update (temp_exp_main.py:555,
:631-632) as one kernel over the explainer's flat fp32 bucket -- equal to torch.optim.Adam within fp32 rounding over
several steps (with and without weight decay, parameters that get no gradient untouched), replayable from a HIP
graph (the device step count advances per replay), state-dict round trip, and the explainer's training step at
Enron dims with FusedAdam against the reference's Adam update.

Below those: ``tm_adam_step`` and ``tm_copy_many`` called directly (guard floats around every buffer, the fp64
restatement tests/adam_ref.py as the yardstick): every unaligned head and tail, the grid-stride loop above the block
cap, the hyper-parameter corners, a step split into runs, the argument rejections; FusedAdam over 70 parameters with
unreached ones in the middle; ``zero_grad(set_to_none=False)``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nets(seed=0):
    torch.manual_seed(seed)
    a = torch.nn.Sequential(torch.nn.Linear(13, 37), torch.nn.ReLU(), torch.nn.Linear(37, 5),
                            torch.nn.Linear(3, 3)).cuda()            # the last layer never gets a gradient
    b = torch.nn.Sequential(torch.nn.Linear(13, 37), torch.nn.ReLU(), torch.nn.Linear(37, 5),
                            torch.nn.Linear(3, 3)).cuda()
    b.load_state_dict(a.state_dict())
    return a, b


def _loss(net, k):
    x = torch.randn(64, 13, generator=torch.Generator().manual_seed(100 + k)).cuda()
    return net[2](net[1](net[0](x))).pow(2).mean()


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_fused_adam_equals_torch_adam(wd):
    from tempme_amd.optim import FusedAdam
    a, b = _nets()
    oa = torch.optim.Adam(a.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ob = FusedAdam(b.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p3 = b[3].weight.detach().clone()
    for k in range(6):
        for net, opt in ((a, oa), (b, ob)):
            opt.zero_grad()
            _loss(net, k).backward()
            opt.step()
        for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
            torch.testing.assert_close(pb, pa, rtol=1e-5, atol=1e-6, msg=f"step {k} {na}")
    assert float(ob.step_t.item()) == 6.0
    if wd == 0.0:
        assert torch.equal(b[3].weight, p3)          # no gradient reached it: it does not move (torch skips it)
    # the parameters, their gradients and the moments are views of the flat buckets
    assert all(p.grad.data_ptr() >= ob.flat_grad.data_ptr() for p in b.parameters() if p.grad is not None)
    assert b[3].weight.grad is None                  # not reached: torch's None, as torch.optim.Adam leaves it


def test_fused_adam_graph_replay_equals_eager():
    from tempme_amd.optim import FusedAdam
    a, b = _nets(1)
    oa = FusedAdam(a.parameters(), lr=5e-3)
    ob = FusedAdam(b.parameters(), lr=5e-3)
    for k in range(2):                               # eager warm-up on both
        for net, opt in ((a, oa), (b, ob)):
            opt.zero_grad()
            _loss(net, k).backward()
            opt.step()
    x = torch.randn(64, 13, generator=torch.Generator().manual_seed(7)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ob.zero_grad()
        b[2](b[1](b[0](x))).pow(2).mean().backward()
        ob.step()
    torch.cuda.current_stream().wait_stream(s)
    oa.zero_grad()
    a[2](a[1](a[0](x))).pow(2).mean().backward()
    oa.step()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        ob.zero_grad()
        b[2](b[1](b[0](x))).pow(2).mean().backward()
        ob.step()
    for _ in range(3):                               # capture did not run the step; 3 replays = 3 eager steps
        gr.replay()
        oa.zero_grad()
        a[2](a[1](a[0](x))).pow(2).mean().backward()
        oa.step()
    torch.cuda.synchronize()
    assert float(ob.step_t.item()) == float(oa.step_t.item()) == 6.0
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)


def test_fused_adam_state_dict_round_trip():
    from tempme_amd.optim import FusedAdam
    a, b = _nets(2)
    oa = torch.optim.Adam(a.parameters(), lr=1e-2)
    for k in range(3):
        oa.zero_grad()
        _loss(a, k).backward()
        oa.step()
    b.load_state_dict(a.state_dict())
    ob = FusedAdam(b.parameters(), lr=1e-2)
    ob.load_state_dict(oa.state_dict())
    assert float(ob.step_t.item()) == 3.0
    for k in range(3, 5):
        for net, opt in ((a, oa), (b, ob)):
            opt.zero_grad()
            _loss(net, k).backward()
            opt.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        torch.testing.assert_close(pb, pa, rtol=1e-5, atol=1e-6)


def test_train_step_with_fused_adam_matches_reference_enron():
    """test_gpu_enron.py's one-iteration reference check (losses, every gradient, the Adam update) with the
    explainer's optimizer = FusedAdam: the update equals the reference's torch.optim.Adam update."""
    import enron_inputs as EI
    from tempme_amd import TempME
    from tempme_amd.optim import FusedAdam
    from tempme_amd.train import Batch, train_step
    dev = torch.device("cuda", 0)
    z = EI.golden()
    g = EI.graph(z)
    N, B = 20, EI.SETS[20]
    base = EI.build_tgn(z, g).to(dev)
    ex = TempME(base, "tgn", "enron", out_dim=40, hid_dim=64, temp=0.07, if_cat_feature=True, dropout_p=0.1,
                device=dev, null_model=EI.null(z))
    _, unexpected = ex.load_state_dict(EI.weights(z, "train"), strict=False)
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
    opt = FusedAdam(ex.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    p0 = {k: v.detach().clone() for k, v in ex.named_parameters()}
    ex.eval()
    out = train_step(ex, base, opt, batch, beta=0.5, prior_p=0.3, if_bern=False)
    got = np.array([out["loss"].item(), out["pred_loss"].item(), out["kl_loss"].item()])
    np.testing.assert_allclose(got, z["train_losses"], rtol=1e-5, atol=1e-6)
    ref_keys = {k[len("train_grad_"):] for k in z.files if k.startswith("train_grad_")}
    for k, v in ex.named_parameters():
        upd = (v.detach() - p0[k]).cpu().numpy()
        if k not in ref_keys:
            # no gradient reaches it in the reference (its .grad stays None there): zero gradient, no update here
            assert v.grad is None or not v.grad.any(), k
            assert not upd.any(), k
            continue
        gr = z[f"train_grad_{k}"].astype(np.float64)
        ga = v.grad.detach().cpu().numpy().astype(np.float64)
        scale = np.abs(gr).max()
        assert np.linalg.norm(ga - gr) <= 2e-4 * np.linalg.norm(gr) + 1e-9, k
        sure = np.abs(gr) > max(1e-3 * scale, 1e-7)
        np.testing.assert_allclose(upd[sure], z[f"train_upd_{k}"][sure], atol=2e-6, rtol=1e-3, err_msg=k)


# ------------------------------------------------------------------ tm_adam_step called directly
# The kernel against tests/adam_ref.py (fp64, the same steps).  Bound per buffer x in (p, m, v), max-norm:
#     max(10 * |x_32 - x_64|_inf, 4 ulp of max|x|)
# x_32 = torch.optim.Adam in fp32 on the CPU from the same inputs (gradients pre-multiplied by grad_scale): DESIGN.md
# §6i's envelope for one formula under another rounding order; the ulp floor covers the few roundings between m and p
# when the fp32 run happens to land on the fp64 value.  A skipped element or a wrong step count is off by about lr.
SENT = -7.25                                             # outside [off, off + n): must survive bitwise
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
HEAD_SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 1023, 1024, 1025, 1029]
GRID_N = 2 * 2097152 + 4 * 256 * 5 + 3                   # the 2048-block cap: some threads make three trips, some two


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _guarded(x, off):
    """[SENT * off | x | SENT * 8] on the GPU (allocations are at least 16-byte aligned: head = (4 - off) % 4)."""
    buf = torch.full((off + x.size + 8,), SENT, dtype=torch.float32)
    buf[off:off + x.size] = torch.from_numpy(x)
    buf = buf.cuda()
    assert buf.data_ptr() % 16 == 0
    return buf


def _inputs(n, steps, seed, gscale=1.0, zero_moments=False, zero_every=0):
    """fp32 p, per-step g, and starting moments of the gradients' own scale (what running averages of them hold)."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    gs = [(gscale * rng.standard_normal(n)).astype(np.float32) for _ in range(steps)]
    if zero_every:
        for g in gs:
            g[::zero_every] = 0.0
    m = (0.3 * gscale * rng.standard_normal(n)).astype(np.float32)
    v = ((0.3 * gscale * rng.standard_normal(n)) ** 2).astype(np.float32)
    if zero_moments:
        m[:], v[:] = 0.0, 0.0
    return p, gs, m, v


def _adam_call(bufs, g, off, lo, n, hp, step_t, done, advance=1):
    """tm_adam_step over elements [lo, lo + n) of the guarded buffers; returns the code, raises nothing."""
    from tempme_amd import _lib as L
    at = lambda t: t.data_ptr() + 4 * (off + lo)  # noqa: E731
    return L.lib().tm_adam_step(at(bufs[0]), at(g), at(bufs[1]), at(bufs[2]), n, hp["lr"], hp["b1"], hp["b2"],
                                hp["eps"], hp["wd"], hp["gscale"], L.ptr(step_t), L.ptr(done), advance,
                                L.stream_ptr(bufs[0].device))


def _references(p, gs, m, v, t_before, hp):
    """Per step (p, m, v): adam_ref carried in fp64, and torch.optim.Adam in fp32 on the CPU."""
    from adam_ref import adam_ref
    r64, r32 = [], []
    x = [a.astype(np.float64) for a in (p, m, v)]
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"],
                           foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(t_before)), "exp_avg": torch.from_numpy(m.copy()),
                     "exp_avg_sq": torch.from_numpy(v.copy())}
    for k, g in enumerate(gs):
        x = list(adam_ref(x[0], g, x[1], x[2], t_before + k, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"],
                          hp["gscale"]))
        r64.append(x)
        tp.grad = torch.from_numpy(g) * hp["gscale"]
        opt.step()
        st = opt.state[tp]
        r32.append([tp.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()])
    return r64, r32


def _hp(**kw):
    return dict(dict(lr=LR, b1=B1, b2=B2, eps=EPS, wd=0.0, gscale=1.0), **kw)


def _run_kernel_case(n, off, steps, t_before, hp, label, **inp):
    """``steps`` consecutive kernel steps with no host sync in between (the buffers are snapshotted on the stream
    after every call), then: guards and gradients bitwise intact after every call, p / m / v within the bound of
    adam_ref after every step, the step count advanced, the completion counter back at 0.  Returns the final p."""
    from tempme_amd import _lib as L
    p, gs, m, v = _inputs(n, steps, seed=1000 * off + n % 997, **inp)
    bufs = [_guarded(a, off) for a in (p, m, v)]
    gbufs = [_guarded(g, off) for g in gs]
    g0 = [_bits(g) for g in gbufs]
    step_t = torch.full((1,), float(t_before), dtype=torch.float32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    snaps = []
    for k in range(steps):
        assert _adam_call(bufs, gbufs[k], off, 0, n, hp, step_t, done) == L.TM_OK, label
        snaps.append([b.clone() for b in bufs] + [g.clone() for g in gbufs])
    torch.cuda.synchronize()
    assert float(step_t.item()) == t_before + steps and int(done.item()) == 0, label
    r64, r32 = _references(p, gs, m, v, t_before, hp)
    sent = _bits(torch.full((1,), SENT))[0]
    worst = {}
    for k, snap in enumerate(snaps):
        for name, b in zip("pmv", snap[:3]):
            bb = _bits(b)
            assert bool((bb[:off] == sent).all()) and bool((bb[off + n:] == sent).all()), (label, k, name, "guard")
        for j, g in enumerate(snap[3:]):
            assert torch.equal(_bits(g), g0[j]), (label, k, "grad written")
        for i, name in enumerate("pmv"):
            got = snap[i][off:off + n].cpu().numpy().astype(np.float64)
            x64, x32 = r64[k][i], r32[k][i].astype(np.float64)
            bound = max(10.0 * np.abs(x32 - x64).max(), 4.0 * float(np.spacing(np.float32(np.abs(x64).max()))))
            worst[name] = max(worst.get(name, 0.0), float(np.abs(got - x64).max()) / bound)
    print(f"tm_adam_step {label}: worst err/bound " + " ".join(f"{k}={r:.3f}" for k, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), (label, worst)
    return snaps[-1][0][off:off + n].cpu().numpy(), p


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_adam_kernel_heads_and_tails(off):
    """Every head (off floats past a 16-byte boundary: head = (4 - off) % 4), n < head, head only, head + tail with
    no float4 in between, all four tails; three steps from non-zero moments, t_before 0 and 5."""
    for n in HEAD_SIZES:
        for t_before in (0, 5):
            _run_kernel_case(n, off, 3, t_before, _hp(wd=1e-2), f"n={n} off={off} t={t_before}")


@pytest.mark.parametrize("off", [0, 3])
def test_adam_kernel_grid_stride(off):
    """Above the 2048-block cap: the grid-stride loop's second and third trips, the completion counter at 2048
    blocks; two steps."""
    _run_kernel_case(GRID_N, off, 2, 5, _hp(wd=1e-2), f"n={GRID_N} off={off}")


@pytest.mark.parametrize("t_before", [0, 999, 99999])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.0, 0.999), (0.9, 0.0)])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_kernel_hyper_parameters(wd, gscale, betas, t_before):
    _run_kernel_case(1029, 1, 3, t_before, _hp(wd=wd, gscale=gscale, b1=betas[0], b2=betas[1]),
                     f"wd={wd} gscale={gscale} betas={betas} t={t_before}")


@pytest.mark.parametrize("gscale", [1e-6, 1e3])
def test_adam_kernel_gradient_scales(gscale):
    _run_kernel_case(1029, 1, 3, 0, _hp(), f"|g|~{gscale}", gscale=gscale)


def test_adam_kernel_zero_gradients_leave_p_alone():
    """g = 0 at every 7th element, zero moments, no weight decay: those p are bitwise unchanged (0 / eps = 0)."""
    got, p0 = _run_kernel_case(1029, 1, 3, 0, _hp(), "zeros every 7th", zero_moments=True, zero_every=7)
    assert np.array_equal(got[::7].view(np.int32), p0[::7].view(np.int32))
    assert not np.array_equal(got, p0)


def test_adam_kernel_runs_share_one_step():
    """A step as two launches over [0, a) and [a, n), a odd (advance = 0, then advance = 1: both read the same t)
    = the single launch over [0, n) bitwise; the count advances once, and not at all after the advance = 0 launch."""
    from tempme_amd import _lib as L
    n, a, off, t_before = 1029, 333, 1, 5
    p, gs, m, v = _inputs(n, 1, seed=77)
    hp = _hp(wd=1e-2)
    res = []
    for split in (False, True):
        bufs, g = [_guarded(x, off) for x in (p, m, v)], _guarded(gs[0], off)
        step_t = torch.full((1,), float(t_before), dtype=torch.float32, device="cuda")
        done = torch.zeros(1, dtype=torch.int32, device="cuda")
        if split:
            assert _adam_call(bufs, g, off, 0, a, hp, step_t, done, advance=0) == L.TM_OK
            assert float(step_t.item()) == t_before and int(done.item()) == 0
            assert _adam_call(bufs, g, off, a, n - a, hp, step_t, done, advance=1) == L.TM_OK
        else:
            assert _adam_call(bufs, g, off, 0, n, hp, step_t, done, advance=1) == L.TM_OK
        assert float(step_t.item()) == t_before + 1 and int(done.item()) == 0
        res.append([_bits(b) for b in bufs])
    for name, one, two in zip("pmv", *res):
        assert torch.equal(one, two), name
    assert not torch.equal(res[0][0], _bits(_guarded(p, off)))


def test_adam_kernel_gate():
    """tm_adam_step_gated: a non-zero device flag = tm_adam_step bitwise; a zero flag writes nothing to p / m / v
    and the step count still advances (the span no rank reached, as the last launch of a step)."""
    from tempme_amd import _lib as L
    n, off, t_before = 1029, 1, 5
    p, gs, m, v = _inputs(n, 1, seed=78)
    hp = _hp(wd=1e-2)
    res = {}
    for flag in (None, 0.5, 0.0):
        bufs, g = [_guarded(x, off) for x in (p, m, v)], _guarded(gs[0], off)
        step_t = torch.full((1,), float(t_before), dtype=torch.float32, device="cuda")
        done = torch.zeros(1, dtype=torch.int32, device="cuda")
        if flag is None:
            assert _adam_call(bufs, g, off, 0, n, hp, step_t, done) == L.TM_OK
        else:
            gate = torch.full((1,), flag, dtype=torch.float32, device="cuda")
            at = lambda t: t.data_ptr() + 4 * off  # noqa: E731
            assert L.lib().tm_adam_step_gated(at(bufs[0]), at(g), at(bufs[1]), at(bufs[2]), n, hp["lr"], hp["b1"],
                                              hp["b2"], hp["eps"], hp["wd"], hp["gscale"], L.ptr(step_t), L.ptr(done),
                                              1, L.ptr(gate), L.stream_ptr(g.device)) == L.TM_OK
        assert float(step_t.item()) == t_before + 1 and int(done.item()) == 0, flag
        res[flag] = [_bits(b) for b in bufs]
    untouched = [_bits(_guarded(x, off)) for x in (p, m, v)]
    for i, name in enumerate("pmv"):
        assert torch.equal(res[0.5][i], res[None][i]), name
        assert torch.equal(res[0.0][i], untouched[i]), name
        assert not torch.equal(res[None][i], untouched[i]), name


def test_adam_kernel_rejects_bad_arguments():
    """TM_E_ARG and nothing written: grad at another 16-byte offset than param, n < 0, beta1 = 1, NaN lr; n = 0 is
    TM_OK and writes nothing either."""
    from tempme_amd import _lib as L
    n, off = 64, 1
    p, gs, m, v = _inputs(n, 1, seed=5)
    bufs, g = [_guarded(x, off) for x in (p, m, v)], _guarded(gs[0], off)
    step_t = torch.full((1,), 3.0, dtype=torch.float32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    before = [_bits(b) for b in bufs + [g, step_t, done]]
    fn, st = L.lib().tm_adam_step, L.stream_ptr(bufs[0].device)
    at = lambda t, extra=0: t.data_ptr() + 4 * (off + extra)  # noqa: E731

    def call(n_=n, lr=LR, b1=B1, g_extra=0):
        return fn(at(bufs[0]), at(g, g_extra), at(bufs[1]), at(bufs[2]), n_, lr, b1, B2, EPS, 1e-2, 1.0,
                  L.ptr(step_t), L.ptr(done), 1, st)
    assert call(g_extra=1) == L.TM_E_ARG
    assert call(n_=-1) == L.TM_E_ARG
    assert call(b1=1.0) == L.TM_E_ARG
    assert call(lr=float("nan")) == L.TM_E_ARG
    assert call(n_=0) == L.TM_OK
    torch.cuda.synchronize()
    for was, now in zip(before, bufs + [g, step_t, done]):
        assert torch.equal(was, _bits(now))


# ------------------------------------------------------------------ tm_copy_many and sync_grads
COPY_SIZES = [0, 1, 3, 255, 256, 257, 65536, 65537, 90000, 2, 5, 7, 31, 33, 63, 64, 65, 127, 129, 511, 513, 1000, 1023,
              1025, 2047, 4097, 8191, 10001, 16385, 32769, 70001, 131073]


def test_copy_many_32_jobs_of_mixed_sizes():
    """One launch, 32 jobs from empty to 131,073 elements (the 256-block cap: above 65,536 a job grid-strides),
    sources and destinations at every offset within 16 bytes; destinations bitwise, their guards intact."""
    from tempme_amd import _lib as L
    assert len(COPY_SIZES) == 32
    rng = np.random.default_rng(3)
    srcs, dsts, jobs = [], [], []
    for i, k in enumerate(COPY_SIZES):
        s = _guarded(rng.standard_normal(k).astype(np.float32), i % 4)
        d = torch.full((4 + (i // 4) % 4 + k + 8,), SENT, dtype=torch.float32, device="cuda")
        srcs.append(s)
        dsts.append(d)
        jobs.append(L.CopyJob(s.data_ptr() + 4 * (i % 4), d.data_ptr() + 4 * (4 + (i // 4) % 4), k))
    arr = (L.CopyJob * 32)(*jobs)
    assert L.lib().tm_copy_many(arr, 32, L.stream_ptr(dsts[0].device)) == L.TM_OK
    torch.cuda.synchronize()
    sent = _bits(torch.full((1,), SENT))[0]
    for i, (k, s, d) in enumerate(zip(COPY_SIZES, srcs, dsts)):
        lo = 4 + (i // 4) % 4
        db = _bits(d)
        assert torch.equal(db[lo:lo + k], _bits(s)[i % 4:i % 4 + k]), (i, k)
        assert bool((db[:lo] == sent).all()) and bool((db[lo + k:] == sent).all()), (i, k, "guard")


def test_copy_many_rejects_bad_jobs():
    from tempme_amd import _lib as L
    s = torch.ones(16, device="cuda")
    d = torch.full((16,), SENT, device="cuda")
    st = L.stream_ptr(d.device)
    ok = L.CopyJob(s.data_ptr(), d.data_ptr(), 16)
    assert L.lib().tm_copy_many((L.CopyJob * 33)(*[ok] * 33), 33, st) == L.TM_E_ARG
    assert L.lib().tm_copy_many((L.CopyJob * 2)(ok, L.CopyJob(s.data_ptr(), d.data_ptr(), -1)), 2, st) == L.TM_E_ARG
    assert L.lib().tm_copy_many((L.CopyJob * 2)(ok, L.CopyJob(None, d.data_ptr(), 4)), 2, st) == L.TM_E_ARG
    torch.cuda.synchronize()
    assert bool((d == SENT).all())


class _Many(torch.nn.Module):
    """70 parameters of odd sizes (most spans start off a 16-byte boundary) and one 300 x 300 weight; three in the
    middle of the list never enter the loss."""
    SKIP = (20, 21, 45)
    BIG = 33

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(9)
        shapes = [(300, 300) if i == self.BIG else (2 * (i % 9) + 3,) if i % 3 else (3, 2 * (i % 5) + 1)
                  for i in range(70)]
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes])

    def loss(self, k):
        g = torch.Generator().manual_seed(50 + k)
        tot = 0.0
        for i, p in enumerate(self.ps):
            if i not in self.SKIP:
                tot = tot + (p - torch.randn(*p.shape, generator=g).to(p.device)).pow(2).sum() / (i + 1)
        return tot


def test_fused_adam_many_parameters_unaligned_runs():
    """70 parameters (three tm_copy_many launches), three unreached in the middle (three runs, the later ones with
    non-zero heads), a non-contiguous caller-assigned .grad in one step (sync_grads' fallback copy, still reached):
    four steps = torch.optim.Adam; the unreached stay put under weight decay; one shared step count."""
    from tempme_amd.optim import FusedAdam
    a, b = _Many().cuda(), _Many().cuda()
    oa = torch.optim.Adam(a.parameters(), lr=1e-2, weight_decay=1e-2)
    ob = FusedAdam(b.parameters(), lr=1e-2, weight_decay=1e-2)
    assert sum(off % 4 != 0 for _, off, _ in ob._spans) > 35
    assert any(ob._spans[i + 1][1] % 4 for i in _Many.SKIP)          # a run after a gap starts with a head
    before = [b.ps[i].detach().clone() for i in _Many.SKIP]
    for k in range(4):
        for net, opt in ((a, oa), (b, ob)):
            opt.zero_grad()
            net.loss(k).backward()
            if k == 2:
                w = net.ps[_Many.BIG]
                w.grad = w.grad.t().contiguous().t()
                assert not w.grad.is_contiguous()
            opt.step()
        for i, (pa, pb) in enumerate(zip(a.ps, b.ps)):
            torch.testing.assert_close(pb, pa, rtol=1e-5, atol=1e-6, msg=f"step {k} parameter {i}")
    assert float(ob.step_t.item()) == 4.0
    for i, was in zip(_Many.SKIP, before):
        assert torch.equal(b.ps[i], was) and b.ps[i].grad is None
    assert b.ps[_Many.BIG].grad.data_ptr() == ob.flat_grad[ob._spans[_Many.BIG][1]:].data_ptr()


def test_fused_adam_zero_grad_keeping_the_views():
    """zero_grad(set_to_none=False): every .grad is a (zero) tensor, and torch.optim.Adam updates every such
    parameter -- the layer the loss skips too (its moments decay, weight decay applies).  FusedAdam does the same."""
    from tempme_amd.optim import FusedAdam
    a, b = _nets(3)
    oa = torch.optim.Adam(a.parameters(), lr=1e-2, weight_decay=1e-2)
    ob = FusedAdam(b.parameters(), lr=1e-2, weight_decay=1e-2)

    def loss_all(net, k):
        x = torch.randn(64, 13, generator=torch.Generator().manual_seed(100 + k)).cuda()
        y = net[2](net[1](net[0](x)))
        return y.pow(2).mean() + net[3](y[:, :3]).pow(2).mean()
    for k in range(4):
        for net, opt in ((a, oa), (b, ob)):
            if k < 2:
                opt.zero_grad()
                loss_all(net, k).backward()
            else:
                opt.zero_grad(set_to_none=False)
                _loss(net, k).backward()
            opt.step()
        if k == 1:
            skipped = a[3].weight.detach().clone()
        for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
            torch.testing.assert_close(pb, pa, rtol=1e-5, atol=1e-6, msg=f"step {k} {na}")
    assert not torch.equal(a[3].weight, skipped)         # torch moved the skipped layer
    assert float(ob.step_t.item()) == 4.0
