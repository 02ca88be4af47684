"""TEST INFRASTRUCTURE ONLY -- the GraphMixer shape matrix: one case per kernel instance that the channel width C
(the edge-feature width), the time/node width T, the token count N and the layer count L select in
csrc/graphmixer.hip and csrc/graphmixer_train.hip, and one builder for a case's inputs.

  gm_fused_kernel<NC, NTT>      NC = ceil(C / 16) in 1..16, NTT = 1 + (N > 16); taken when tm_gm_fused_ok
                                (C, T and HC = 4 C multiples of 4)
  gm_embed_kernel<NMT, NTW>     the LDS-tiled fallback: NMT = 1 + (N > 16), NTW = 3 + (C > 192)
  gm_bwd_kernel<NMT, NTW, TS8>  d explanation weights: same NMT / NTW, TS8 = (N > 16); tm_gm_embed_bwd_ok is its
                                LDS plan ((L + 3) images of [32][r16(C) + 4] floats and a scratch within 160 KB)
  gt_fwd_kernel / gt_bwd_layer_kernel   runtime dimensions; a wave owns output tiles wave + 4 i, i < 4

Every case carries the seed of its inputs and weights: tests/test_gm_shapes_cpu.py holds the fp32 torch formulation
of each case to a margin against fp64, and the seeds were picked so that it keeps that margin (a ReLU of
affinity_score.fc1 that sits within rounding of zero flips between fp32 and fp64 and moves a gradient by far
more than any summation order).
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

V, E, B = 60, 200, 5

# N tokens, C channels (edge-feature width), T node-feature / time-encoding width, L mixer layers, B batch (R = 3 B
# rows: 15 is no multiple of the fused kernel's 4 or 2 rows per workgroup), seed, edge_attr given
Case = namedtuple("Case", "id N C T L B seed edge_attr")


# seed 0 unless a unit of affinity_score.fc1 then sits within the logit tolerance of its ReLU's kink (relu_margin):
# at (12, 240, 240, 1) seed 0 leaves one pre-activation at 1.4e-7, fp32 and fp64 take different sides of it and
# d ew differs by 0.12 ||g64|| -- or, at the narrow shapes (narrow()), unless the fp32 torch formulation's d ew is
# then more than 3e-6 ||g64|| off on some thread count (seed 0 at (2, 256): 1.3e-5 on 8 threads, 3.3e-5 on 4)
_SEEDS = {(17, 228, 20, 2): 1, (12, 240, 240, 1): 1, (20, 172, 172, 3): 1,
          (2, 256, 20, 2): 1, (16, 2, 172, 2): 1, (2, 48, 20, 2): 4}


def _case(N, C, T=20, L=2, edge_attr=False, B=B):
    seed = _SEEDS.get((N, C, T, L), 0)
    cid = f"N{N}-C{C}-T{T}-L{L}" + ("-attr" if edge_attr else "")
    return Case(cid, N, C, T, L, B, seed, edge_attr)


def fused_width(nc):
    """The channel width that stands for NC = nc channel tiles: a full last tile for even nc, four channels of it
    for odd nc (4, 32, 36, 64, ..., 224, 228, 256)."""
    return 16 * nc if nc % 2 == 0 else 16 * nc - 12


FUSED = ([_case(N, fused_width(nc)) for nc in range(1, 17) for N in (16, 17)]
         + [_case(N, C) for C in (4, 172, 256) for N in (2, 32)]
         + [_case(17, 48, L=0), _case(17, 48, L=4),      # HC = 192: exactly one GM_HCH chunk
            _case(32, 256, T=256, L=4),
            _case(17, 256, edge_attr=True)])

FALLBACK = [_case(16, 2, T=172),        # <1, 3>
            _case(17, 50),              # <2, 3>
            _case(16, 250),             # <1, 4>
            _case(17, 224, T=6),        # <2, 4>: C aligned, T % 4 != 0 alone refuses the fused kernel
            _case(17, 193),             # the smallest NTW = 4 width, 15 padded columns
            _case(16, 250, L=4),
            _case(17, 50, L=0)]

EW_BWD = [_case(16, 196, T=196, L=1),
          _case(20, 224, T=20, L=1),
          _case(12, 240, T=240, L=1),   # the largest shape tm_gm_embed_bwd_ok admits: 144 floats of LDS to spare
          _case(17, 100, L=4),
          _case(17, 48, L=0),
          _case(2, 48, L=2),
          _case(32, 172, T=172, L=2),
          _case(16, 4, L=2)]

EW_REFUSED = [_case(12, 256, T=256, L=1),
              _case(20, 172, T=172, L=3)]

# (N, C, T, L, p, B) for tests/test_gpu_gm_train.py's make_case (its own V, E and seeds)
TRAIN = [(17, 196, 196, 1, 0.5, 7),     # NT = 13: wave 0 alone has a fourth tile; HC = 784 = 6 * 128 + 16
         (32, 256, 256, 4, 0.5, 5),
         (16, 224, 224, 2, 0.0, 7),
         (17, 196, 20, 1, 0.5, 7),      # T < C
         (2, 4, 20, 1, 0.5, 5)]
TRAIN_V, TRAIN_E = 300, 2000


def dims(N, C):
    """(HT, HC): the token and channel FFN's hidden widths at the model's default expansion factors."""
    return int(0.5 * N), int(4.0 * C)


def instance(N, C):
    """The template arguments a shape selects: (NC, NTT) of gm_fused_kernel, (NMT, NTW) of gm_embed_kernel and
    gm_bwd_kernel."""
    return SimpleNamespace(NC=(C + 15) // 16, NTT=1 + (N > 16), NMT=1 + (N > 16), NTW=3 + (C > 192))


def make_inputs(N, C, T, L, B=B, seed=0, V=V, E=E):
    """One case's inputs, built as test_hip_ew_gradient_vs_oracle builds them (padding neighbours at rate 0.25,
    row 1 of every side without a valid neighbour): nf [V, T], ef [E + 1, C] with row 0 zero, cut [B], the three
    sides' (node, eid, ts) records, src / dst / fake [B] and ew0 [3 B, N]."""
    rng = np.random.default_rng(seed)
    nf = rng.uniform(0, 1, (V, T)).astype(np.float32)
    ef = rng.uniform(0, 1, (E + 1, C)).astype(np.float32)
    nf[0] = ef[0] = 0
    cut = np.floor(rng.uniform(5e7, 1e8, B))
    sgs = []
    for _ in range(3):
        node = rng.integers(1, V, (B, N))
        node[rng.uniform(size=node.shape) < 0.25] = 0
        node[1] = 0
        eid = np.where(node > 0, rng.integers(1, E + 1, node.shape), 0)
        ts = np.where(node > 0, np.floor(cut[:, None] - rng.uniform(0, 5e7, node.shape)), 0.0)
        sgs.append(([node.astype(np.float64), None], [eid.astype(np.float64), None], [ts, None]))
    src, dst, fake = (rng.integers(1, V, B) for _ in range(3))
    ew0 = rng.uniform(0, 1, (3 * B, N)).astype(np.float32)
    pad = np.concatenate([sg[0][0] for sg in sgs]) == 0
    return SimpleNamespace(nf=nf, ef=ef, cut=cut, sgs=sgs, src=src, dst=dst, fake=fake, ew0=ew0, pad=pad, N=N, C=C, T=T,
                           L=L, B=B)


def make_model(inp, seed, device, dropout=0.1):
    """The case's GraphMixer with seeded initial weights (on the CPU unless moved)."""
    from tempme_amd.graphmixer import GraphMixer
    torch.manual_seed(seed)
    return GraphMixer(inp.nf, inp.ef, n_neighbors=inp.N, device=device, num_tokens=inp.N, num_layers=inp.L,
                      dropout=dropout)


_cases = {}


def build(case):
    """(inputs, CPU state_dict, edge_attr or None) of a case, computed once."""
    if case not in _cases:
        inp = make_inputs(case.N, case.C, case.T, case.L, case.B, case.seed)
        sd = {k: v.detach().clone() for k, v in make_model(inp, case.seed, "cpu").state_dict().items()}
        ea = None
        if case.edge_attr:
            ea = np.random.default_rng(case.seed + 1).uniform(0, 1, (3 * case.B, case.N, case.C)).astype(np.float32)
        _cases[case] = (inp, sd, ea)
    return _cases[case]


def oracle_logits(case, ew, dtype):
    """oracle.graphmixer_ref.contrast's logits [2 B] (ew: a [3 B, N] tensor of `dtype`, or None)."""
    from oracle import graphmixer_ref as O
    inp, sd, ea = build(case)
    p, n = O.contrast(sd, case.L, inp.src, inp.dst, inp.fake, inp.cut, *inp.sgs,
                      explain_weights=None if ew is None else [ew],
                      edge_attr=None if ea is None else torch.from_numpy(ea).to(dtype), dtype=dtype)
    return torch.cat([p, n]).reshape(-1)


def relu_margin(case, dtype=torch.float64):
    """min |z| over affinity_score.fc1's pre-activations z (the only ReLU of the model) with the explanation
    weights applied: how far every unit sits from the kink where d ew jumps."""
    from oracle import graphmixer_ref as O
    inp, sd, ea = build(case)
    ew = torch.from_numpy(inp.ew0).to(dtype)
    ea = None if ea is None else torch.from_numpy(ea).to(dtype)
    side = lambda x, k: None if x is None else x[k * case.B:(k + 1) * case.B]  # noqa: E731
    s, d, n = (O.node_embeddings(sd, case.L, nodes, inp.cut, sg[0][0], sg[1][0], sg[2][0], side(ew, k), side(ea, k),
                                 dtype)
               for k, (nodes, sg) in enumerate(zip((inp.src, inp.dst, inp.fake), inp.sgs)))
    x = torch.cat([torch.cat([s, s], 0), torch.cat([d, n], 0)], dim=1)
    return float(O._lin(sd, "affinity_score.fc1", x).abs().min())


def bce_targets(B, dtype=torch.float32):
    return torch.cat([torch.ones(B), torch.zeros(B)]).to(dtype)


_refs = {}


def oracle_ew_grad(case, dtype):
    """(logits [2 B], d ew [3 B, N]) of a BCE loss on the oracle's logits, by autograd in `dtype`; once per case."""
    key = (case, dtype)
    if key not in _refs:
        inp = build(case)[0]
        ew = torch.from_numpy(inp.ew0).to(dtype).requires_grad_(True)
        logits = oracle_logits(case, ew, dtype)
        torch.nn.functional.binary_cross_entropy_with_logits(logits, bce_targets(case.B, dtype)).backward()
        _refs[key] = (logits.detach(), ew.grad.detach())
    return _refs[key]


def narrow(case):
    """Two tokens or two channels: a LayerNorm over two values (x_hat = +-1 up to eps) amplifies rounding where the
    two are close, and the fp32 torch formulation's own d ew is anything from 1e-7 to 6.6e-5 ||g64|| off from one
    seed, and 1.3e-5 to 3.3e-5 from one thread count, to another."""
    return min(case.N, case.C) <= 2


def ew_grad_bound(case):
    """The bound on ||g - g64|| for a case's d ew: 1e-5 ||g64||, which tests/test_gm_shapes_cpu.py requires of the
    fp32 torch formulation too; at the narrow shapes check_grads' max(1e-4 ||g64||, 10 ||g32 - g64||), which that
    test caps at 3e-4 ||g64||.  Which of the two applies depends on the shape alone."""
    g64, g32 = oracle_ew_grad(case, torch.float64)[1], oracle_ew_grad(case, torch.float32)[1]
    nrm, e32 = float(torch.linalg.norm(g64)), float(torch.linalg.norm(g32.double() - g64))
    return max(1e-4 * nrm, 10 * e32) if narrow(case) else 1e-5 * nrm
