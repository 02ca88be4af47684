"""walk_kernel applies A1G (attention.MLP.0 folded with W2 and event_gcn's second layer) once per walk, to the
mixed hidden vector alpha_0 H_0 + alpha_1 H_1, instead of once per position: exact algebra (A1G is linear,
alpha_0 + alpha_1 = 1), a re-association in fp32.  Position 0's hidden vector and score are carried to the
position-1 pass, so these tests hold the kernel to oracle/encoder_ref.forward (CPU, torch fp32, on the walks the
pipeline itself sampled) at the project's contract rtol=1e-5, atol=1e-6 where a wrong, swapped or stale mix
shows:

* saturated attention: attention.W1.weight scaled by W1_SCALE, so that for many walks |s0 - s1| is past the
  point where fp32 expf underflows (alpha exactly (1, 0) or (0, 1): the output then depends on one position
  alone, no averaging hides a swap), for others not; the conditions are asserted on the oracle's own scores,
  and the oracle's fp32 result is asserted to be within a tenth of the contract of its fp64 result there;
* partial units (slot count no multiple of 16) and null positions (events at the very start of the timeline:
  eid 0 at position 0, at position 1, in whole slots; this sampler never leaves positions 0 and 1 both null
  under a valid slot, so that pattern cannot be had);
* M = 1 and 3 walks per slot (3 and 7 passes per unit);
* both launch forms: the split form (fewer than 512 units) and the persistent form with the grid capped at 8
  workgroups, so that every wave takes about 16 units through tickets (what one unit carries must never reach
  the next); each against the oracle, and the two against each other;
* both node-feature forms (zero-node instance, two-branch instance) and both attention classes.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6
N = 20
# chosen on the CPU with the oracle (the conditions below are asserted in every case): the default-initialised
# scores are O(0.1-1), fp32 expf(-x) is 0 from x ~ 104
W1_SCALE = 2000.0
SAT, MIXED, FEW = 110.0, 5.0, 8     # |s0 - s1| of a saturated / a truly mixed walk; how many of each at least
EARLY = (3, 11, 43)                  # rows of the timeline's start: a wholly null event, then sparse ones


@functools.lru_cache(maxsize=None)
def _graph(node_feat):
    from tempme_amd.workload import enron_like, split
    g = enron_like(n_nodes=120, n_edges=6000, seed=11, node_feat=node_feat)
    (src, dst, ts, eidx), rows, pool = split(g)
    assert rows.all()
    return g, (src, dst, ts, eidx), pool


def events(g, late, E):
    """E target events: the EARLY rows of the timeline, then the first late (test-split) ones."""
    e = np.array(EARLY)
    k = E - len(e)
    return tuple(np.concatenate([g[n][e], a[:k]]) for n, a in zip(("src", "dst", "ts", "eidx"), late))


def oracle_scores(sd, n_feat, e_feat, node, eid, ts, cut, cnt, temporal):
    """The two attention scores of every walk as oracle/encoder_ref.forward forms them (its lines up to the
    softmax, from its own building blocks)."""
    from oracle import encoder_ref as er
    node, eid = torch.as_tensor(node, dtype=torch.long), torch.as_tensor(eid, dtype=torch.long)
    t = torch.as_tensor(np.asarray(ts, dtype=np.float64)).float()
    cut = torch.as_tensor(np.asarray(cut, dtype=np.float64)).float()
    cnt = torch.as_tensor(np.asarray(cnt, dtype=np.float64)).float()
    B, W = eid.shape[:2]
    tf = er.time_encode(sd, (t[:, :, 2:3] - t).reshape(B, -1)).reshape(B, W, 3, -1)
    ev = torch.cat([e_feat[eid], cnt, tf], dim=-1)
    xs, xt = n_feat[node[:, :, [0, 2, 4]]], n_feat[node[:, :, [1, 3, 5]]]
    lev = er._lin(sd, "event_conv.lin_event", ev)

    def mlp(x):
        return er._lin(sd, "event_conv.MLP.2", torch.relu(er._lin(sd, "event_conv.MLP.0", x)))
    f = torch.cat([mlp(xs + torch.relu(xt + lev)), mlp(xt + torch.relu(xs + lev))], dim=-1)
    wp = er._lin(sd, "attention.W1", f[:, :, 2, :])
    wq = er._lin(sd, "attention.W2", f[:, :, 0:2, :])
    sc = (wp.unsqueeze(2) * wq).sum(-1)
    if temporal:
        diff = torch.abs(cut.view(B, 1, 1) - t[:, :, :2])
        sc = sc * (1.0 - 0.3 + 0.3 * torch.exp(-diff / (diff.std() + 1e-6)))
    return sc.numpy()


def oracle(sd, g, walks, cut, B, temporal):
    """walks: side-major arrays (node6, eid3, ts3, cat, cnt) [3, E, W, ...]; one oracle call per group (side,
    batch of B events: the std of |cut - t| is per group).  Returns imp [3, E, W] in fp32, the same in fp64,
    and the score differences s0 - s1 [3, E, W]."""
    from oracle import encoder_ref as er
    nf, ef = torch.from_numpy(g["n_feat"]), torch.from_numpy(g["e_feat"])
    sd64 = {k: v.double() for k, v in sd.items()}
    node6, eid3, ts3, cat, cnt = walks
    E = eid3.shape[1]
    r32, r64, ds = (np.zeros(eid3.shape[:3], dt) for dt in (np.float32, np.float64, np.float32))
    for s in range(3):
        for b in range(0, E, B):
            q = slice(b, b + B)
            a = (node6[s, q], eid3[s, q], ts3[s, q], cat[s, q], cut[q], cnt[s, q].astype(np.float64))
            r32[s, q] = er.forward(sd, nf, ef, *a, temporal=temporal).numpy()[..., 0]
            r64[s, q] = er.forward(sd64, nf, ef, *a, temporal=temporal).numpy()[..., 0]
            sc = oracle_scores(sd, nf, ef, a[0], a[1], a[2], a[4], torch.from_numpy(a[5]), temporal)
            ds[s, q] = sc[..., 0] - sc[..., 1]
    return r32, r64, ds


def check_oracle_conditions(r32, r64, ds, eid3, saturated):
    """What the case relies on, on the oracle's own numbers."""
    # the fp32 oracle is a reference at this input: a tenth of the contract from its fp64 self
    assert np.all(np.abs(r32 - r64) <= 0.1 * (ATOL + RTOL * np.abs(r64)))
    if saturated:
        assert (ds > SAT).sum() >= FEW and (ds < -SAT).sum() >= FEW, "alpha saturates both ways"
        assert (np.abs(ds) < MIXED).sum() >= FEW, "and is a true mix elsewhere"
    else:
        assert np.abs(ds).max() < MIXED
    p = eid3 != 0
    assert (~p[..., 0] & p[..., 1] & p[..., 2]).sum() >= FEW, "null position 0"
    assert (p[..., 0] & ~p[..., 1] & p[..., 2]).sum() >= FEW, "null position 1"
    assert (~p[..., 2]).reshape(-1, N, p.shape[2] // N).all(-1).sum() >= FEW, "whole null slots"
    assert p.all(-1).sum() >= FEW, "complete walks"


@functools.lru_cache(maxsize=None)
def _model(node_feat, tg, scale):
    import tempme_amd as tm
    g, _, _ = _graph(node_feat)
    dev = torch.device("cuda", 0)
    f = tm.NeighborFinder.from_edges(g["src"], g["dst"], g["eidx"], g["ts"], g["n_nodes"], device=dev, seed=3)

    class Base:
        n_feat_th = torch.from_numpy(g["n_feat"])
        e_feat_th = torch.from_numpy(g["e_feat"])
        node_raw_features = torch.nn.Embedding.from_pretrained(n_feat_th, padding_idx=0, freeze=True)
        edge_raw_features = torch.nn.Embedding.from_pretrained(e_feat_th, padding_idx=0, freeze=True)

    torch.manual_seed(0)
    ex = tm.TempME(Base(), "tgn", "enron", 40, 64, device=dev, null_model={k: 1 / 12 for k in range(1, 13)},
                   use_temporal_guidance=tg).to(dev).eval()
    with torch.no_grad():
        ex.attention.W1.weight.mul_(scale)
    sd = {k: v.detach().cpu() for k, v in ex.state_dict().items()}
    return ex, f, sd


def _run(node_feat, tg, scale, M, ev, B, walk_blocks=0):
    """One pipeline call over the events ev -> (imp [3, E, W], the sampled walks), numpy."""
    from tempme_amd import _lib as L
    from tempme_amd.pipeline import ExplainPipeline
    ex, f, _ = _model(node_feat, tg, scale)
    _, _, pool = _graph(node_feat)
    dev = torch.device("cuda", 0)
    src, dst, ts, eidx, ids = ev
    pipe = ExplainPipeline(ex, f.graph, torch.from_numpy(pool), N, M, B, seed=3)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    L.check(L.lib().tm_debug_set(L.TM_DEBUG_WALK_BLOCKS, walk_blocks), "tm_debug_set")
    try:
        with torch.no_grad():
            imp, _, _ = pipe.run(t(src, np.int32), t(dst, np.int32), t(ts, np.float64), t(eidx, np.int32),
                                 t(ids, np.int32))
        torch.cuda.synchronize()
    finally:
        L.check(L.lib().tm_debug_set(L.TM_DEBUG_WALK_BLOCKS, 0), "tm_debug_set")
    pipe.check_errors()
    assert pipe.etab is not None, "the pipeline's table mode is off"
    assert ex._node_zero == (node_feat == "zeros")
    b = pipe.buf
    return imp.cpu().numpy(), tuple(x.cpu().numpy() for x in (b.node6, b.eid3, b.ts3, b.cat, b.cnt))


def _close(a, ref):
    d = np.abs(a - ref)
    print("max |diff| %.3g, worst diff / bound %.3g" % (d.max(), (d / (ATOL + RTOL * np.abs(ref))).max()))
    np.testing.assert_allclose(a, ref, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("scale", [1.0, W1_SCALE])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("tg", [True, False])
@pytest.mark.parametrize("node_feat", ["zeros", "uniform"])
def test_split_form_partial_units(node_feat, tg, M, scale):
    """7 events = 420 slots = 26 units and a quarter (the last unit has 4 valid columns), split form."""
    g, late, _ = _graph(node_feat)
    E = 7
    ev = events(g, late, E) + (np.arange(E),)
    imp, walks = _run(node_feat, tg, scale, M, ev, E)
    r32, r64, ds = oracle(_model(node_feat, tg, scale)[2], g, walks, ev[2], E, tg)
    check_oracle_conditions(r32, r64, ds, walks[1], scale != 1.0)
    _close(imp, r32)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("tg", [True, False])
@pytest.mark.parametrize("node_feat", ["zeros", "uniform"])
def test_persistent_form_many_units_per_wave(node_feat, tg, M):
    """140 events = 525 units in one call: the persistent form, its grid capped at 8 workgroups (32 waves, about
    16 units each through tickets); the same events in two calls of 70 (263 units each): the split form.  Both
    against the oracle and against each other, saturated attention."""
    g, late, _ = _graph(node_feat)
    E, B = 140, 70
    ev = events(g, late, E) + (np.arange(E),)
    imp, walks = _run(node_feat, tg, W1_SCALE, M, ev, B, walk_blocks=8)
    r32, r64, ds = oracle(_model(node_feat, tg, W1_SCALE)[2], g, walks, ev[2], B, tg)
    check_oracle_conditions(r32, r64, ds, walks[1], True)
    _close(imp, r32)
    halves = [_run(node_feat, tg, W1_SCALE, M, tuple(a[q] for a in ev), B) for q in (slice(0, B), slice(B, E))]
    for k in range(5):      # the same walks (sampling depends on the event id, not on the call)
        assert np.array_equal(np.concatenate([h[1][k] for h in halves], axis=1), walks[k])
    split = np.concatenate([h[0] for h in halves], axis=1)
    _close(split, r32)
    _close(imp, split)
