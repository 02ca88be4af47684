"""Generate tests/golden/tgat_uslegis.npz by running the REFERENCE base TGAT itself on the CPU.

    python tests/golden/make_tgat_goldens.py <path to a checkout of dharunm236/TempME>

Run where the reference is available; the tests only read the committed .npz.  Nothing of the reference
is stored but what its programs compute: logits, gradients, masks, metrics and parameter names.

Inputs are the committed uslegis fixtures tests/tgn_inputs.py loads (32 test events at N = 20, the two
feature sets, TempME's explanation and the random weights of the TGN golden).  Per case:
  * ``torch.manual_seed(seed); TGAT(nf, ef, 20, num_layers=2, n_head=H)`` in eval mode, with the time
    encoder's phase perturbed to N(0, 0.5) (stored) so that the add rounding of TimeEncode matters;
  * contrast without weights (``ori``), with the explanation (``expl``) and with the random weights
    (``rand``), in fp32, and ``ori`` with the model cast to fp64;
  * the gradient of pos.sum() + neg.sum() with respect to the six explanation tensors (src, tgt, bgd x
    hop-1, hop-2) at the explanation, from the fp64 model and from the fp32 model.  Both are stored as
    fp32 (the fp64 gradient rounded once, 6e-8 relative: below the fp32 model's own distance to it);
  * threshold_test's tgat branch (temp_exp_main.py:216-250): the zero masks of every ratio (bit-packed),
    the per-ratio logits and the five metrics;
  * the state_dict's key names, shapes and per-tensor (sum, |sum|, sum of squares) of the seeded init.
"""
import ast
import copy
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tgn_inputs as TI  # noqa: E402

SEEDS = {"uslegis": 21, "synth": 22}
HEADS = {"uslegis": 3, "synth": 2}
RATIOS = [0.01, 0.02, 0.04, 0.06, 0.08, 0.10, 0.12, 0.14, 0.16, 0.18, 0.2, 0.22, 0.24, 0.26, 0.28, 0.30]
SIDES = ("src", "tgt", "bgd")


def load_ref_function(ref, relpath, name, **ns):
    """One FunctionDef of a reference module that cannot be imported (temp_exp_main.py parses argv)."""
    path = os.path.join(ref, relpath)
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    ns.setdefault("__name__", "golden_" + name)
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def phase_perturbation(case, dim):
    return np.random.default_rng(SEEDS[case]).normal(0, 0.5, dim).astype(np.float32)


def build(case, cls):
    nf, ef = TI.feats(case)
    torch.manual_seed(SEEDS[case])
    m = cls(nf, ef, TI.N_DEG, num_layers=2, n_head=HEADS[case])
    m.eval()
    return m


def side_weights(ws, B, dtype=None, grad=False):
    """[hop-1 [3B, N], hop-2 [3B, N^2]] -> per side (hop-1 [B, N], hop-2 [B, N^2]) leaf tensors."""
    out = []
    for s in range(3):
        pair = []
        for w in ws:
            x = w[s * B:(s + 1) * B].detach().clone()
            if dtype is not None:
                x = x.to(dtype)
            pair.append(x.requires_grad_(grad))
        out.append(tuple(pair))
    return out


def main(ref):
    sys.path.insert(0, ref)
    from sklearn.metrics import average_precision_score, roc_auc_score
    from TGAT.TGAT import TGAT
    threshold_test = load_ref_function(ref, "temp_exp_main.py", "threshold_test", math=math, np=np, torch=torch,
                                       average_precision_score=average_precision_score, roc_auc_score=roc_auc_score)
    d = TI.load_batch()
    B, N = d["B"], d["N"]
    a = (d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], d["sg_src"], d["sg_tgt"], d["sg_bgd"])
    res = {"ratios": np.array(RATIOS)}
    for case in ("uslegis", "synth"):
        base = build(case, TGAT)
        sd = base.state_dict()
        res[f"{case}_sd_names"] = np.array(list(sd.keys()))
        res[f"{case}_sd_shapes"] = np.array([",".join(str(int(x)) for x in v.shape) for v in sd.values()])
        res[f"{case}_sd_stats"] = np.array([[v.double().sum().item(), v.double().abs().sum().item(),
                                             (v.double() ** 2).sum().item()] for v in sd.values()])
        pert = phase_perturbation(case, base.time_dim)
        res[f"{case}_pert_phase"] = pert
        with torch.no_grad():
            base.time_encoder.phase.data.copy_(torch.from_numpy(pert))
        base64 = copy.deepcopy(base).double()

        def run(model, w):
            if w is None:
                return model.contrast(*a, test=True, if_explain=False)
            return model.contrast(*a, test=True, if_explain=True, exp_weights=[[w[0], w[1]], [w[0], w[2]]])

        expl, rand = TI.explanation(case), TI.rand_weights(case)
        with torch.no_grad():
            pos_o, neg_o = run(base, None)
            res[f"{case}_ori"] = torch.cat([pos_o, neg_o]).numpy()
            res[f"{case}_ori64"] = torch.cat(run(base64, None)).numpy()
            res[f"{case}_expl"] = torch.cat(run(base, side_weights(expl, B))).numpy()
            res[f"{case}_rand"] = torch.cat(run(base, side_weights(rand, B))).numpy()
        for tag, model, dtype in (("grad32", base, torch.float32), ("grad64", base64, torch.float64)):
            w = side_weights(expl, B, dtype, grad=True)
            pos, neg = run(model, w)
            (pos.sum() + neg.sum()).backward()
            for s, side in enumerate(SIDES):
                for h in (0, 1):
                    res[f"{case}_{tag}_{side}{h}"] = w[s][h].grad.to(torch.float32).numpy()

        # threshold_test, capturing every masked-subgraph contrast it makes
        y_ori = torch.where(torch.cat([pos_o, neg_o]).sigmoid() > 0.5, 1., 0.).view(-1, 1)
        calls = []
        orig = base.contrast

        def capture(*x, **k):
            out = orig(*x, **k)
            calls.append(([np.concatenate(x[i][0], axis=1) == 0 for i in (5, 6, 7)], torch.cat(out).numpy()))
            return out
        base.contrast = capture

        class A:
            pass
        args = A()
        args.ratios, args.base_type, args.n_degree, args.bs = RATIOS, "tgat", N, B
        six = [w for s in range(3) for w in (expl[0][s * B:(s + 1) * B], expl[1][s * B:(s + 1) * B])]
        metrics = threshold_test(args, six, base, d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], pos_o, neg_o,
                                 y_ori, d["sg_src"], d["sg_tgt"], d["sg_bgd"])
        base.contrast = orig
        res[f"{case}_thr_metrics"] = np.array([float(m) for m in metrics])
        res[f"{case}_thr_logits"] = np.stack([c[1] for c in calls])
        res[f"{case}_thr_zero_bits"] = np.packbits(np.stack([np.concatenate(c[0], axis=0) for c in calls]))
        env = float(np.abs(res[f"{case}_ori"] - res[f"{case}_ori64"]).max())
        print(case, "ori", float(res[f"{case}_ori"].mean()), "expl", float(res[f"{case}_expl"].mean()),
              "rand", float(res[f"{case}_rand"].mean()), "fp32 envelope", env, "thr", res[f"{case}_thr_metrics"])
    out = os.path.join(HERE, "tgat_uslegis.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
