"""Shared inputs of the edge-feature-width tests (test_edge_width_cpu.py, test_gpu_edge_width.py): which kernel
instance each edge-feature width `de` selects at dn = 172, hid_dim = 64, if_cat_feature = True, and a seeded model
per width.  Not a test.

WIDTHS is written out by hand from the dispatch code; test_edge_width_cpu.py restates that code's arithmetic and
checks every row against it, and that the rows reach every class a constructible width can reach.
"""
import functools

import numpy as np
import torch

from test_gpu_lin_split import N, N_EDGES, N_NODES, _walks  # noqa: F401  (the walks of test_gpu_lin_split, re-exported)

DN, HID = 172, 64
RTOL, ATOL = 1e-5, 1e-6
SMALL = (1, 7)          # groups, events per group: 140 slots = 8.75 units
BIG = (3, 137)          # 8220 slots = 513.75 units: the persistent form
TESTED_BEFORE = (1, 32, 172)

# de, lin_event K steps of 16 (nqe), the dependency gate's (d1nq), per-edge-id table, fused walk kernel, plain-mode
# edge-feature load (load_ef's branch per 32-wide step, or the streamed ring), gate-table kernel, training event_gcn
_ROWS = [
    (1, 11, 11, False, True, "scalar", "reg<11>", "lds"),
    (4, 12, 11, False, True, "scalar", "reg<11>", "reg12"),
    (16, 12, 12, False, True, "scalar", "reg<12>", "reg12"),
    (17, 12, 12, False, True, "scalar", "reg<12>", "lds"),
    (20, 13, 12, False, True, "scalar", "reg<12>", "reg13"),
    (24, 13, 13, False, True, "scalar", "reg<13>", "reg13"),
    (32, 13, 13, True, True, "float4", "reg<13,3,13>", "reg13"),
    (33, 13, 13, True, True, "scalar+scalar", "reg<13,3,13>", "lds"),
    (36, 14, 13, True, True, "float4+scalar", "reg<13,3,14>", "reg14"),
    (37, 14, 14, False, True, "scalar+scalar", "lds", "lds"),
    (48, 14, 14, False, True, "float4+scalar", "lds", "reg14"),
    (49, 14, 14, False, True, "scalar+scalar", "lds", "lds"),
    (50, 15, 14, False, False, "none", "lds", "lds"),
    (148, 21, 20, False, True, "streamed", "lds", "lds"),
    (160, 21, 21, False, True, "streamed", "lds", "lds"),
    (164, 22, 21, False, True, "streamed", "lds", "lds"),
    (168, 22, 22, True, True, "streamed", "reg<22,11,22>", "lds"),
    (172, 22, 22, True, True, "streamed", "reg<22,11,22>", "lds"),
    (176, 22, 22, False, True, "streamed", "reg<22>", "lds"),
]
_KEYS = ("de", "nqe", "d1nq", "table", "fused", "load_ef", "gate", "train")
WIDTHS = {r[0]: dict(zip(_KEYS, r)) for r in _ROWS}
NEW_WIDTHS = tuple(de for de in WIDTHS if de not in TESTED_BEFORE)


class Base:
    def __init__(self, n_feat, e_feat):
        self.n_feat_th = torch.from_numpy(n_feat)
        self.e_feat_th = torch.from_numpy(e_feat)
        self.node_raw_features = torch.nn.Embedding.from_pretrained(self.n_feat_th, padding_idx=0, freeze=True)
        self.edge_raw_features = torch.nn.Embedding.from_pretrained(self.e_feat_th, padding_idx=0, freeze=True)


@functools.lru_cache(maxsize=None)
def features(de, node_feat):
    """e_feat ~ U(0, 1) [N_EDGES + 1, de] with row 0 zero; n_feat [N_NODES + 1, 172] uniform or all zero."""
    rng = np.random.RandomState(5)
    e_feat = rng.uniform(0, 1, (N_EDGES + 1, de)).astype(np.float32)
    e_feat[0] = 0
    n_feat = np.zeros((N_NODES + 1, DN), np.float32)
    if node_feat != "zeros":
        n_feat[1:] = rng.uniform(0, 1, (N_NODES, DN))
    return n_feat, e_feat


@functools.lru_cache(maxsize=None)
def model(de, node_feat="uniform", device=None):
    """Seeded TempME(..., 40, 64) over features(de, node_feat) -> (explainer, state dict on the CPU, n_feat, e_feat).
    The parameters are drawn on the CPU, so the state dict is the same with and without a device."""
    import tempme_amd as tm
    n_feat, e_feat = features(de, node_feat)
    torch.manual_seed(7)
    ex = tm.TempME(Base(n_feat, e_feat), "tgn", "synthetic", 40, HID, device=device,
                   null_model={k: 1 / 12 for k in range(1, 13)})
    if device is not None:
        ex = ex.to(device)
    ex = ex.eval()
    sd = {k: v.detach().cpu().clone() for k, v in ex.state_dict().items()}
    return ex, sd, torch.from_numpy(n_feat), torch.from_numpy(e_feat)


def oracle(sd, nf, ef, G, B, M, double=False):
    """oracle/encoder_ref.forward over _walks(G, B, M) -> [G, B, W] in sd's precision (double: in fp64)."""
    from oracle import encoder_ref as er
    if double:
        sd = {k: v.double() for k, v in sd.items()}
    node6, eid3, ts3, cat, cut, cnt = _walks(G, B, M)
    out = [er.forward(sd, nf, ef, node6[g], eid3[g], ts3[g], cat[g], cut[g], cnt[g].astype(np.float64)).numpy()[..., 0]
           for g in range(G)]
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def oracle32(de, node_feat, G, B, M):
    _, sd, nf, ef = model(de, node_feat)
    return oracle(sd, nf, ef, G, B, M)


def bound(ref):
    return ATOL + RTOL * np.abs(ref)
