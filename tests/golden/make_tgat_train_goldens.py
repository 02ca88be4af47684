"""Generate tests/golden/tgat_train.npz by running the REFERENCE base TGAT's training step on the CPU.

    python tests/golden/make_tgat_train_goldens.py <path to a checkout of dharunm236/TempME>

Run where the reference is available; the tests only read the committed .npz.  Nothing of the reference is
stored but what its programs compute: a loss, logits, gradients, gradient norms and parameter names.

Inputs are the golden batch of tests/tgn_inputs.py (32 test events of uslegis_sampled at N = 20).  Per case:
  * ``torch.manual_seed(seed); TGAT(nf, ef, 20, num_layers=2, n_head=H, drop_out=0.0)`` in ``.train()`` mode
    (dropout 0.0: the step is deterministic), the time encoder's phase set to the committed perturbation of
    tgat_uslegis.npz cut to the time dimension;
  * ``contrast(..., if_explain=False)`` as learn_base.py:227-229 calls it, the loss of learn_base.py:233-235
    (BCEWithLogits(pos, 1) + BCEWithLogits(neg, 0)) and ``loss.backward()``, by the fp32 model (``<case>_...32``)
    and by the same model cast to fp64 (``<case>_...64``, stored as fp32).
A small model's fp64 matrix gradients are stored as their distance to the fp32 ones (``<case>_delta64_<name>``
fp16, times ``<case>_unit64_<name>``), which keeps the file under 1 MiB; tests/tgat_train_inputs.py puts them
back together.
Cases: two small models on the synth features truncated to (d_node, d_edge) columns -- ``small24`` (24, 8,
H = 2, seed 31) and ``small40`` (40, 25, H = 3, seed 32) -- with every parameter gradient stored in full, and
the full-size ``uslegis`` (H = 3, seed 21) and ``synth`` (H = 2, seed 22) with every 1-D gradient in full and the
Frobenius norm of every 2-D gradient (the full matrices would be ~10 MB).
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tgn_inputs as TI  # noqa: E402

# case -> (feature set, d_node, d_edge (None = all columns), heads, seed)
CASES = {"small24": ("synth", 24, 8, 2, 31), "small40": ("synth", 40, 25, 3, 32),
         "uslegis": ("uslegis", None, None, 3, 21), "synth": ("synth", None, None, 2, 22)}


def case_feats(case):
    fs, dn, de, _, _ = CASES[case]
    nf, ef = TI.feats(fs)
    if dn is not None:
        nf, ef = np.ascontiguousarray(nf[:, :dn]), np.ascontiguousarray(ef[:, :de])
    return nf, ef


def case_phase(case, dim):
    g = np.load(os.path.join(HERE, "tgat_uslegis.npz"))
    return g[f"{CASES[case][0]}_pert_phase"][:dim].copy()


def main(ref):
    sys.path.insert(0, ref)
    from TGAT.TGAT import TGAT
    d = TI.load_batch()
    B = d["B"]
    a = (d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], d["sg_src"], d["sg_tgt"], d["sg_bgd"])
    res = {}
    for case, (_, dn, _, H, seed) in CASES.items():
        nf, ef = case_feats(case)
        torch.manual_seed(seed)
        base = TGAT(nf, ef, TI.N_DEG, num_layers=2, n_head=H, drop_out=0.0)
        with torch.no_grad():
            base.time_encoder.phase.data.copy_(torch.from_numpy(case_phase(case, base.time_dim)))
        base.train()
        for tag, m in (("32", base), ("64", copy.deepcopy(base).double())):
            pos, neg = m.contrast(*a, test=False, if_explain=False)
            crit = torch.nn.BCEWithLogitsLoss()
            loss = crit(pos, torch.ones((B, 1), dtype=pos.dtype)) + crit(neg, torch.zeros((B, 1), dtype=neg.dtype))
            loss.backward()
            res[f"{case}_loss{tag}"] = np.array(loss.item(), dtype=np.float64)
            res[f"{case}_pos{tag}"] = pos.detach().to(torch.float32).numpy()
            res[f"{case}_neg{tag}"] = neg.detach().to(torch.float32).numpy()
            names = []
            for k, v in m.named_parameters():
                if v.grad is None:
                    continue
                names.append(k)
                if v.grad.dim() == 1 or (dn is not None and tag == "32"):
                    res[f"{case}_grad{tag}_{k}"] = v.grad.detach().to(torch.float32).numpy()
                elif dn is not None:
                    # a small model's fp64 matrix: its distance to the fp32 one, in units of the largest distance,
                    # as fp16 (5e-4 of a distance that is itself ~1e-6 of the gradient: finer than an fp32 copy)
                    delta = v.grad.detach().numpy() - res[f"{case}_grad32_{k}"].astype(np.float64)
                    unit = float(np.abs(delta).max()) or 1.0
                    res[f"{case}_delta64_{k}"] = (delta / unit).astype(np.float16)
                    res[f"{case}_unit64_{k}"] = np.array(unit)
                else:
                    res[f"{case}_norm{tag}_{k}"] = np.array(torch.linalg.norm(v.grad.detach().double()).item())
            res[f"{case}_grad_names"] = np.array(names)
            print(case, tag, "loss", loss.item(), "params with grad", len(names))
    out = os.path.join(HERE, "tgat_train.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
