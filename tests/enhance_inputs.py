"""Shared inputs of the enhance (motif-enhanced link prediction) tests and of their golden generator
(tests/golden/make_enhance_goldens.py): the committed uslegis walks of tests/encoder_inputs.py (32 test events,
N = 20, W = 60 = 20 hop-1 slots x M = 3, the three sides), node degrees counted from the committed edge list, and
the tensors the golden file does not store because they are redrawn from a seed: affinity_score's weights and the
three base-model embeddings (``*_gat``)."""
import os

import numpy as np
import torch

import encoder_inputs as EI

G = EI.G
SIDES = EI.SIDES
CASES = ("uslegis", "synth")
SEEDS = {"uslegis": 31, "synth": 32}
SUB_BATCHES = (32, 5, 2, 1)          # the group sizes the tests run (statistics are per group: one golden each)
M_SLOT = 3                           # walks per hop-1 slot of the committed walks (find_k_walks' layout)
FC1_ROW_STEP = 2                     # the golden stores rows 0, 2, 4, ... of fc1.weight's gradient (file size)
GRAD_KEYS = ("affinity_score.fc1.weight", "attention.W1.weight", "event_conv.lin_event.weight")


def edge_list():
    """(u, i) of tests/golden/data/ml_uslegis_sampled.csv (columns: row, u, i, ts, label, idx)."""
    a = np.loadtxt(os.path.join(G, "data", "ml_uslegis_sampled.csv"), delimiter=",", skiprows=1, usecols=(1, 2))
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64)


def node_degrees(num_nodes):
    """compute_node_degrees.py:53-62 / :95-108 by hand: undirected counts, 1 for untouched ids, padded with ones."""
    u, i = edge_list()
    deg = np.ones(max(num_nodes, int(max(u.max(), i.max())) + 1), dtype=np.float32)
    cnt = {}
    for a, b in zip(u.tolist(), i.tolist()):
        cnt[a] = cnt.get(a, 0) + 1
        cnt[b] = cnt.get(b, 0) + 1
    for k, v in cnt.items():
        deg[k] = v
    return deg[:num_nodes]


def drawn(case, hid=64, if_cat=True):
    """affinity_score's parameters (reference shapes, explainer_new.py:62-69, :127-128) and the src / tgt / bgd base
    embeddings [32, node_dim], from numpy.default_rng(SEEDS[case])."""
    d = EI.load(case)
    dn = d["n_feat"].shape[1]
    D = hid + (12 if if_cat else 0) + dn
    rng = np.random.default_rng(SEEDS[case])
    f = lambda *s, sc=1.0: torch.from_numpy((rng.normal(0, 1, s) * sc).astype(np.float32))  # noqa: E731
    sd = {"affinity_score.fc1.weight": f(D, 2 * D, sc=(2.0 / (3 * D)) ** 0.5), "affinity_score.fc1.bias": f(D, sc=0.05),
          "affinity_score.fc2.weight": f(1, D, sc=(2.0 / (D + 1)) ** 0.5), "affinity_score.fc2.bias": f(1, sc=0.05)}
    gats = [f(d["B"], dn) for _ in SIDES]
    return sd, gats


def load(case):
    """encoder_inputs.load plus ``deg`` (float32 [n_nodes]), ``aff`` (affinity_score state dict) and ``gats``."""
    d = EI.load(case)
    d["deg"] = node_degrees(d["n_feat"].shape[0])
    d["aff"], d["gats"] = drawn(case)
    return d


def side_walks(d, side, bsz):
    """(walks tuple as batch_loader.get_item hands it to TempME, edge_identify) of the first bsz events."""
    s = d[side]
    return (s["node"][:bsz], s["eid"][:bsz], s["ts"][:bsz], s["cat"][:bsz], s["marg"][:bsz]), s["cnt"][:bsz]


def golden():
    return np.load(os.path.join(G, "enhance_uslegis.npz"))


# ------------------------------------------------------------------ helpers shared by the CPU and GPU tests
class Base:
    def __init__(self, n_feat, e_feat):
        self.n_feat_th, self.e_feat_th = n_feat, e_feat
        self.node_raw_features = torch.nn.Embedding.from_pretrained(n_feat, padding_idx=0, freeze=True)
        self.edge_raw_features = torch.nn.Embedding.from_pretrained(e_feat, padding_idx=0, freeze=True)


def make_explainer(d, device=torch.device("cpu"), **kw):
    import tempme_amd as tm
    torch.manual_seed(0)
    ex = tm.TempME(Base(d["n_feat"], d["e_feat"]), "tgn", "uslegis_sampled", 40, kw.pop("hid_dim", 64), device=device,
                   null_model={k: 1.0 / 12 for k in range(1, 13)}, **kw)
    missing, unexpected = ex.load_state_dict(d["sd_all"], strict=False)
    assert not unexpected
    return ex.to(device)


def agg_with_grads(ex, d):
    B = d["B"]
    sides = [side_walks(d, s, B) for s in SIDES]
    dev = ex.affinity_score.fc1.weight.device
    gats = [g.clone().to(dev).requires_grad_(k == 0) for k, g in enumerate(d["gats"])]
    ex.zero_grad()
    pos, neg = ex.enhance_predict_agg(d["ts_cut"][:B], sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides],
                                      *gats)
    (pos.sum() + neg.sum()).backward()
    params = dict(ex.named_parameters())
    grads = {k: params[k].grad.detach().cpu() for k in GRAD_KEYS}
    grads["src_gat"] = gats[0].grad.detach().cpu()
    grads["affinity_score.fc1.weight"] = grads["affinity_score.fc1.weight"][::FC1_ROW_STEP]
    return pos.detach().cpu(), neg.detach().cpu(), grads


def check_agg_against_golden(pos, neg, grads, gold, c):
    tol = 10 * float(gold[f"{c}_env_logit"])
    dl = max(float(np.abs(pos.numpy() - gold[f"{c}_pos"]).max()), float(np.abs(neg.numpy() - gold[f"{c}_neg"]).max()))
    print(c, "logits", dl, "tolerance", tol)
    assert pos.shape == (gold[f"{c}_pos"].shape[0], 1) and neg.shape == pos.shape
    assert dl <= tol
    missed = []
    for k, g in grads.items():
        gt = 10 * float(gold[f"{c}_genv_{k}"])
        dg = float(np.abs(g.numpy() - gold[f"{c}_grad_{k}"]).max())
        print(c, "grad", k, dg, "tolerance", gt)
        if not dg <= gt:
            missed.append((k, dg, gt))
    assert not missed, missed                       # every gradient is measured before the first miss is reported
