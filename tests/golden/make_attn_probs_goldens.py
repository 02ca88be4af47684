"""Generate tests/golden/attn_probs_uslegis.npz by running the REFERENCE base TGN and base TGAT on the CPU with
forward hooks on their attention modules.

    python tests/golden/make_attn_probs_goldens.py <path to a checkout of dharunm236/TempME>

Run where the reference is available; the tests only read the committed .npz.  Nothing of the reference is stored
but what its programs compute: attention probabilities.

Inputs: the first 8 events of tests/tgn_inputs.load_batch() as their own batch (N = 20), the "uslegis" features,
the seeded models of tgn_inputs.build_model / tgat_inputs.build_model (same seeds, same committed perturbations),
eval mode, no explanation weights.  A forward hook on every ``multi_head_target`` (MultiHeadAttention returns
``(output, attn_map [B, N_src, n_head, N])``) records the softmax's output of each call during one ``contrast``:

  TGN   attention_models[0]: the 3B N hop-1 nodes over their hop-2 neighbours  -> tgn_hop2  [3B N, H, N]
        attention_models[1]: the 3B roots over the hop-1 embeddings            -> tgn_hop1  [3B, H, N]
  TGAT  contrast runs forward_msg for src, tgt, src, bgd; per call attn_model_list[0] sees the roots over their raw
        hop-1 neighbours and then the hop-1 nodes over their hop-2 neighbours, attn_model_list[1] the roots over
        the hop-1 embeddings.  The sides src, tgt, bgd (the first src call) are stacked:
        attn_model_list[0], second call of a side -> tgat_hop2 [3B N, H, N]
        attn_model_list[1]                        -> tgat_hop1 [3B, H, N]

Each is stored from the fp32 model (``*_32``) and from the same model cast to fp64 (``*_64``, rounded once to fp32:
3e-8 on a probability, below the fp32 model's own distance to it).  The tolerance of everything compared against
this file is 10 x max |p32 - p64| of the file itself, at least 1e-6 (tests/attn_probs_ref.golden_tol).
"""
import contextlib
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tgn_inputs as TI  # noqa: E402

CASE = "uslegis"
BSZ = 8
TGAT_SEED, TGAT_HEADS = 21, 3          # tgat_inputs.SEEDS / HEADS of the case


def hooked(modules):
    """Forward hooks on ``modules`` -> (per-module lists of attn_map [rows, H, N] in call order, the handles)."""
    seen = [[] for _ in modules]
    handles = []
    for i, m in enumerate(modules):
        def hook(mod, args, out, i=i):
            a = out[1].detach()
            seen[i].append(a.reshape(-1, a.shape[-2], a.shape[-1]).clone())
        handles.append(m.register_forward_hook(hook))
    return seen, handles


@contextlib.contextmanager
def all_double():
    """The reference's TGN creates fp32 tensors on its way (``.float()`` on the time deltas, ``torch.zeros`` for the
    query's time): for the fp64 run they are made fp64, so the whole model runs in double."""
    orig, dflt = torch.Tensor.float, torch.get_default_dtype()
    torch.Tensor.float = lambda self, *a, **k: self.double()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.Tensor.float = orig
        torch.set_default_dtype(dflt)


def run_tgn(model, a):
    mods = [lay.multi_head_target for lay in model.embedding_module.attention_models[:2]]
    seen, handles = hooked(mods)
    with torch.no_grad():
        model.contrast(*a)
    for h in handles:
        h.remove()
    assert len(seen[0]) == 1 and len(seen[1]) == 1
    return seen[1][0], seen[0][0]


def run_tgat(model, a):
    mods = [am.multi_head_target for am in model.attn_model_list]
    seen, handles = hooked(mods)
    with torch.no_grad():
        model.contrast(*a, test=True, if_explain=False)
    for h in handles:
        h.remove()
    assert len(seen[0]) == 8 and len(seen[1]) == 4        # src, tgt, src, bgd
    sides = (0, 1, 3)
    return torch.cat([seen[1][s] for s in sides]), torch.cat([seen[0][2 * s + 1] for s in sides])


def main(ref):
    sys.path.insert(0, ref)
    # the shims of make_goldens.py that importing the reference's TGN package needs: a stub ``turtle`` (names
    # imported, unused, by TGN/tgn.py:2 and embedding_module.py:1), ``numba.jit`` -> identity and a
    # ``torch_scatter`` that is never called here (the samplers and the "mean" aggregator do not run)
    turtle = types.ModuleType("turtle")
    turtle.pos = turtle.position = None
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: a[0] if a and callable(a[0]) and not k else (lambda f: f)
    tsc = types.ModuleType("torch_scatter")
    tsc.scatter = None
    for name, mod in (("turtle", turtle), ("numba", numba), ("torch_scatter", tsc)):
        sys.modules.setdefault(name, mod)
    from TGAT.TGAT import TGAT
    from TGN.tgn import TGN
    d = TI.load_batch(bsz=BSZ)
    a = (d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], d["sg_src"], d["sg_tgt"], d["sg_bgd"])
    B, N = d["B"], d["N"]
    res = {}

    tgn = TI.build_model(CASE, cls=TGN)
    nf, ef = TI.feats(CASE)
    torch.manual_seed(TGAT_SEED)
    tgat = TGAT(nf, ef, TI.N_DEG, num_layers=2, n_head=TGAT_HEADS)
    tgat.eval()
    pert = np.load(os.path.join(HERE, "tgat_uslegis.npz"))[f"{CASE}_pert_phase"]
    with torch.no_grad():
        tgat.time_encoder.phase.data.copy_(torch.from_numpy(pert))

    for name, model, run in (("tgn", tgn, run_tgn), ("tgat", tgat, run_tgat)):
        h1, h2 = run(model, a)
        m64 = copy.deepcopy(model).double()
        if name == "tgn":
            m64.memory.messages = {k: [(r.double(), t.double()) for r, t in v]
                                   for k, v in model.memory.messages.items()}
        with all_double():
            g1, g2 = run(m64, a)
        assert g1.dtype == torch.float64 and g2.dtype == torch.float64, "the fp64 run did not stay in fp64"
        H = h1.shape[1]
        assert tuple(h1.shape) == (3 * B, H, N) and tuple(h2.shape) == (3 * B * N, H, N)
        for tag, p32, p64 in (("hop1", h1, g1), ("hop2", h2, g2)):
            res[f"{name}_{tag}_32"] = p32.numpy().astype(np.float32)
            res[f"{name}_{tag}_64"] = p64.numpy().astype(np.float32)
            print(name, tag, tuple(p32.shape), "max |p32 - p64|", float((p32.double() - p64).abs().max()),
                  "row sums", float(p32.sum(-1).min()), float(p32.sum(-1).max()))
    out = os.path.join(HERE, "attn_probs_uslegis.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
