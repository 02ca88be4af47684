"""Generate tests/golden/graphmixer_train.npz by running the REFERENCE base GraphMixer's training step on the CPU.

    python tests/golden/make_gm_train_goldens.py <path to a checkout of dharunm236/TempME>

Run where the reference is available; the tests only read the committed .npz.  Nothing of the reference is
stored but what its programs compute: a loss, logits, gradients and parameter names.

Inputs are the golden batch of graphmixer_uslegis.npz (tests/tgn_inputs.py: 32 test events of uslegis_sampled at
N = 20) and the two feature sets ``uslegis`` (C = 1) and ``synth``, with the seeds of
tests/test_graphmixer_oracle.py.  Per case:
  * ``torch.manual_seed(seed); GraphMixer(nf, ef, 20, cpu, num_tokens=20, num_layers=3, dropout=0.0)`` in
    ``.train()`` mode (dropout 0.0: the step is deterministic; the same seed draws the same initial weights as
    with any other dropout, which takes no random numbers at construction);
  * ``contrast(..., explain_weights=None, edge_attr=None)`` as learn_base.py:231-232 calls it, the loss of
    learn_base.py:233-235 (BCEWithLogits(pos, 1) + BCEWithLogits(neg, 0)) and ``loss.backward()``;
  * stored: the loss, both logit vectors and the gradient of every parameter that received one
    (``<case>_grad_<name>``), all in fp32 as the reference computed them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tgn_inputs as TI  # noqa: E402

SEEDS = {"uslegis": 21, "synth": 22}


def main(ref):
    sys.path.insert(0, ref)
    from GraphM import GraphMixer
    d = TI.load_batch()
    B = d["B"]
    res = {}
    for case in ("uslegis", "synth"):
        nf, ef = TI.feats(case)
        torch.manual_seed(SEEDS[case])
        m = GraphMixer(nf, ef, n_neighbors=TI.N_DEG, device=torch.device("cpu"), num_tokens=TI.N_DEG, num_layers=3,
                       dropout=0.0)
        m.train()
        pos, neg = m.contrast(d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], d["sg_src"], d["sg_tgt"],
                              d["sg_bgd"], explain_weights=None, edge_attr=None)
        crit = torch.nn.BCEWithLogitsLoss()
        pos_label = torch.ones((B, 1), dtype=torch.float, requires_grad=False)
        neg_label = torch.zeros((B, 1), dtype=torch.float, requires_grad=False)
        loss = crit(pos, pos_label) + crit(neg, neg_label)
        loss.backward()
        res[f"{case}_loss"] = np.array(loss.item(), dtype=np.float32)
        res[f"{case}_pos"] = pos.detach().numpy()
        res[f"{case}_neg"] = neg.detach().numpy()
        names = []
        for k, v in m.named_parameters():
            if v.grad is not None:
                res[f"{case}_grad_{k}"] = v.grad.detach().numpy()
                names.append(k)
        res[f"{case}_grad_names"] = np.array(names)
        print(case, "loss", loss.item(), "params with grad", len(names))
    out = os.path.join(HERE, "graphmixer_train.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
