"""Shared loader for the base-TGN training goldens (tests/golden/make_tgn_train_goldens.py): the cases, their
seeded models with the committed time bias, the golden batch cut into its four steps, and the stored results put
back into tensors."""
import os

import numpy as np
import torch

import tgn_inputs as TI

# case -> (d_node, d_edge (None = all columns of synth), heads, seed)
CASES = {"small8": (8, 4, 2, 41), "small10": (10, 5, 3, 42), "synth": (None, None, 2, 43)}
SMALL = ("small8", "small10")
STEPS, STEP_B = 4, 8


def golden():
    return np.load(os.path.join(TI.G, "tgn_train.npz"))


def heads(case):
    return CASES[case][2]


def case_feats(case):
    dn, de, _, _ = CASES[case]
    nf, ef = TI.feats("synth")
    if dn is not None:
        nf, ef = np.ascontiguousarray(nf[:, :dn]), np.ascontiguousarray(ef[:, :de])
    return nf, ef


def build_model(case, dropout=0.0, n_layers=3):
    """torch.manual_seed(seed); TGN(...) exactly as the golden run (forbidden_memory_update left at its default,
    False), the committed time bias, .train()."""
    from tempme_amd.tgn import TGN
    nf, ef = case_feats(case)
    torch.manual_seed(CASES[case][3])
    m = TGN(nf, ef, n_neighbors=TI.N_DEG, device=torch.device("cpu"), n_layers=n_layers, n_heads=heads(case),
            dropout=dropout)
    with torch.no_grad():
        m.time_encoder.w.bias.data.copy_(torch.from_numpy(TI.golden()["synth_pert_time_bias"][:m.n_node_features].copy()))
    return m.train()


def full_batch():
    d = TI.load_batch()
    return (d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], d["sg_src"], d["sg_tgt"], d["sg_bgd"])


def step_batches():
    """The golden batch as 4 consecutive steps of 8 events, each (src, dst, fake, ts, e_idx, sg_src, sg_tgt, sg_bgd)."""
    d = TI.load_batch()
    out = []
    for k in range(STEPS):
        sl = slice(k * STEP_B, (k + 1) * STEP_B)
        sg = [tuple([x[sl] for x in part] for part in d["sg_" + s]) for s in TI.SIDES]
        out.append((d["src"][sl], d["dst"][sl], d["fake"][sl], d["ts_cut"][sl], d["e_idx"][sl], sg[0], sg[1], sg[2]))
    return out


def stored(g, case, k, tag, shapes):
    """Step k of the fp32 (tag '32') or fp64 (tag '64') reference run -> (loss, logits [2 * STEP_B], names,
    {name: full fp64 gradient}, {name: Frobenius norm}).  ``shapes``: {parameter name: shape} of the model.  Every
    name is in exactly one of the two dicts."""
    pre = f"{case}_s{k}_"
    names = [str(x) for x in g[pre + "grad_names"]]
    flat = g[pre + "grad32"].astype(np.float64)
    small = case in SMALL
    grads, norms, off, ni = {}, {}, 0, 0
    for name in names:
        sh = tuple(shapes[name])
        if small or len(sh) == 1:
            n = int(np.prod(sh))
            v = flat[off:off + n].copy()
            if tag == "64":      # the fp16 distance to the fp32 run, in the tensor's own unit
                v += g[pre + "grad_delta64"][off:off + n].astype(np.float64) * float(g[pre + "grad_unit64"][len(grads)])
            grads[name] = torch.from_numpy(v.reshape(sh))
            off += n
        else:
            norms[name] = float(g[pre + "norm" + tag][ni])
            ni += 1
    assert off == len(flat) and ni == len(g[pre + "norm" + tag])
    logits = np.concatenate([g[pre + "pos" + tag], g[pre + "neg" + tag]]).astype(np.float64).reshape(-1)
    return float(g[pre + "loss" + tag]), logits, names, grads, norms


def shapes_of(model):
    return {k: tuple(v.shape) for k, v in model.named_parameters()}


# ------------------------------------------------------------------ inputs of the kernel-level tests
# (rows, N, d_node, d_edge, d_time, H, seg_rows, node table: rows of a gathered table or 0 = dense, explanation weights)
KERNEL_CASES = [
    (15, 3, 8, 4, 8, 2, 0, 50, True),           # N < 4: one wave per row; rows no multiple of 4
    (21, 5, 8, 4, 8, 3, 0, 50, True),           # split forward; d_key = 20, one ragged register; 3 heads
    (8, 4, 172, 1, 172, 4, 0, 50, False),       # d_key = 345 (uslegis): 6 registers per lane; 4 heads
    (60, 20, 172, 32, 172, 2, 20, 50, False),   # d_key = 376 (the golden dims), head-major inside segments
    (21, 5, 24, 18, 24, 3, 7, 0, False),        # layer 1's form: a dense node table with the d_node output
    # more than 4 * 1024 rows: a wave of the backward walks more than one row and more than one reduction partial
    # exists; 50 table rows take 16,404 slots, so every row is hit many times
    (4101, 4, 8, 4, 8, 2, 0, 50, True),
]


def kernel_inputs(case, seed):
    """fp32 CPU inputs of one attention pass: a quarter of the slots padding (node 0, masked as the model masks
    them: mask = node id), row 3 fully masked, (row 2, last head) with every keep byte 0, dt = floor(U[0, 1e6))."""
    from types import SimpleNamespace
    Rr, N, dn, de, dtm, H, seg, V, with_ew = case
    dk = dn + de + dtm
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen, dtype=torch.float64) * scale).float()
    x = SimpleNamespace(R=Rr, N=N, H=H, dk=dk, dims=(dn, de, dtm), seg=seg, dense=V == 0, node_rows=V,
                        T=float(np.sqrt(dk / H)))
    ids = torch.randint(1, max(V, 9), (Rr, N), generator=gen, dtype=torch.int32)
    ids[torch.rand(Rr, N, generator=gen) < 0.25] = 0
    ids[3] = 0                                                  # one row with no valid neighbour
    x.mask = ids.clone()
    if V:
        x.tab = rnd(V, dn)
        x.node_idx = ids
        x.node = x.tab[ids.long()]
    else:
        x.tab, x.node_idx = None, None
        x.node = rnd(Rr, N, dn)
    x.edge = rnd(Rr, N, de)
    x.dt = torch.floor(torch.rand(Rr, N, generator=gen, dtype=torch.float64) * 1e6).float()
    x.tw = (1.0 / 10 ** torch.linspace(0, 9, dtm)).float()
    x.tb = rnd(dtm, scale=0.5)
    x.qf, x.gz = rnd(Rr, H, dk), rnd(Rr, H, dk)
    x.ew = torch.rand(Rr, N, generator=gen).float() if with_ew else None
    x.keep = (torch.rand(Rr * H * N, generator=gen) < 0.6).to(torch.uint8)
    x.keep.view(Rr, H, N)[2, H - 1] = 0                         # one (row, head) with every byte dropped
    x.scale = float(1.0 / 0.6)
    return x
