"""Shared loader for the base-TGAT training goldens (tests/golden/make_tgat_train_goldens.py): the cases, their
seeded models with the committed phase, the golden batch, and the stored results put back into tensors."""
import os

import numpy as np
import torch

import tgn_inputs as TI

# case -> (feature set, d_node, d_edge (None = all columns), heads, seed)
CASES = {"small24": ("synth", 24, 8, 2, 31), "small40": ("synth", 40, 25, 3, 32),
         "uslegis": ("uslegis", None, None, 3, 21), "synth": ("synth", None, None, 2, 22)}
SMALL = ("small24", "small40")
FULL = ("uslegis", "synth")


def golden():
    return np.load(os.path.join(TI.G, "tgat_train.npz"))


def heads(case):
    return CASES[case][3]


def case_feats(case):
    fs, dn, de, _, _ = CASES[case]
    nf, ef = TI.feats(fs)
    if dn is not None:
        nf, ef = np.ascontiguousarray(nf[:, :dn]), np.ascontiguousarray(ef[:, :de])
    return nf, ef


def build_model(case, drop_out=0.0):
    """torch.manual_seed(seed); TGAT(...) exactly as the golden run, the committed phase, .train()."""
    from tempme_amd.tgat import TGAT
    nf, ef = case_feats(case)
    torch.manual_seed(CASES[case][4])
    m = TGAT(nf, ef, TI.N_DEG, num_layers=2, n_head=heads(case), drop_out=drop_out)
    pert = np.load(os.path.join(TI.G, "tgat_uslegis.npz"))[f"{CASES[case][0]}_pert_phase"][:m.time_dim]
    with torch.no_grad():
        m.time_encoder.phase.data.copy_(torch.from_numpy(pert.copy()))
    return m.train()


def batch():
    d = TI.load_batch()
    return (d["src"], d["dst"], d["fake"], d["ts_cut"], d["sg_src"], d["sg_tgt"], d["sg_bgd"])


def stored(g, case, tag):
    """-> (loss, logits [2B], {name: full fp64 gradient}, {name: Frobenius norm}) of the fp32 (tag '32') or the
    fp64 (tag '64') reference run.  Every parameter is in exactly one of the two dicts."""
    grads, norms = {}, {}
    for k in (str(x) for x in g[f"{case}_grad_names"]):
        if f"{case}_grad{tag}_{k}" in g.files:
            grads[k] = torch.from_numpy(g[f"{case}_grad{tag}_{k}"].astype(np.float64))
        elif f"{case}_delta64_{k}" in g.files and tag == "64":
            grads[k] = torch.from_numpy(g[f"{case}_grad32_{k}"].astype(np.float64)
                                        + g[f"{case}_delta64_{k}"].astype(np.float64) * float(g[f"{case}_unit64_{k}"]))
        else:
            norms[k] = float(g[f"{case}_norm{tag}_{k}"])
    logits = np.concatenate([g[f"{case}_pos{tag}"], g[f"{case}_neg{tag}"]]).astype(np.float64).reshape(-1)
    return float(g[f"{case}_loss{tag}"]), logits, grads, norms


def logit_atol(g, case):
    """tgat_inputs.logit_atol's rule on this fixture: 10 x the reference's own fp32-vs-fp64 envelope, never below 2e-5."""
    env = float(np.abs(stored(g, case, "32")[1] - stored(g, case, "64")[1]).max())
    return 10.0 * max(env, 2e-6)
