"""CPU-side checks of the attention-probability entry points and the baseline explainers: the fp64 comparator
(tests/attn_probs_ref.py) against the reference's own probabilities, the C ABI's surface, and the host logic of
tempme_amd/baselines.py that needs no device.

The golden (tests/golden/attn_probs_uslegis.npz) holds what hooks on the reference's attention modules recorded on the
first 8 events of the uslegis batch.  The comparator is held to it on the two hop-2 passes, whose queries and keys
come from the raw tables alone (the hop-1 passes read the first layer's output, which only the device computes; the
GPU tests hold the models to the hop-1 goldens): TGN's hop-2 pass is one segment of 3B N rows, TGAT's has one segment
of B N rows per side, so both forms of the head-major pairing are exercised, and dropping the pairing must miss.
Tolerance: 10 x max |p32 - p64| of the golden itself, at least 1e-6 (1.7e-5 and 1.8e-5 for the two passes; the
comparator sits 3.2e-8 and 7.1e-8 from the reference's fp64 run).
"""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_probs_ref as AP
import tgat_inputs as TA
import tgn_inputs as TI

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hop2(flavour):
    d = AP.golden_batch()
    nf, _ = TI.feats("uslegis")
    if flavour == "tgn":
        m = TI.build_model("uslegis")
        tab = torch.from_numpy(TI.golden()["uslegis_updated_memory"]).double() + torch.from_numpy(nf).double()
    else:
        m = TA.build_model("uslegis")
        tab = torch.from_numpy(nf).double()
    return m, AP.hop2_inputs(flavour, m, d, tab)


@pytest.mark.parametrize("flavour", ["tgn", "tgat"])
def test_restatement_reproduces_reference_probabilities(flavour):
    g = AP.golden()
    m, (qf, key, mask, T, seg) = _hop2(flavour)
    p = AP.probs(qf, key, mask, T, m.head_major_rows, seg).numpy()
    name = f"{flavour}_hop2"
    tol = AP.golden_tol(g, name)
    err = float(np.abs(p - g[name + "_64"]).max())
    print(flavour, "max |restatement - reference fp64|", err, "tol", tol)
    assert p.shape == g[name + "_64"].shape and err <= tol
    assert float(np.abs(p - g[name + "_32"]).max()) <= tol
    # the pairing matters: row r against mask row r misses by far
    plain = AP.probs(qf, key, mask, T, False, seg).numpy()
    assert float(np.abs(plain - g[name + "_64"]).max()) > 1e-2
    # and so do the segments, where there is more than one (TGAT: one per side)
    if seg:
        one = AP.probs(qf, key, mask, T, True, 0).numpy()
        assert float(np.abs(one - g[name + "_64"]).max()) > 1e-2


def test_golden_is_a_softmax():
    g = AP.golden()
    B, N = AP.GOLDEN_B, TI.N_DEG
    for name, rows, H in (("tgn_hop1", 3 * B, 2), ("tgn_hop2", 3 * B * N, 2), ("tgat_hop1", 3 * B, 3),
                          ("tgat_hop2", 3 * B * N, 3)):
        for tag in ("_32", "_64"):
            p = g[name + tag]
            assert p.shape == (rows, H, N) and p.dtype == np.float32
            assert (p >= 0).all() and np.abs(p.astype(np.float64).sum(-1) - 1).max() < 1e-6
        assert AP.golden_tol(g, name) < 1e-4


def test_pair_rows_segments():
    assert AP.pair_rows(6, 2, True, 3).tolist() == [[0, 1], [2, 0], [1, 2], [3, 4], [5, 3], [4, 5]]
    assert AP.pair_rows(6, 2, True, 0).tolist() == [[0, 1], [2, 3], [4, 5], [0, 1], [2, 3], [4, 5]]
    assert AP.pair_rows(4, 3, False, 2).tolist() == [[r] * 3 for r in range(4)]
    with pytest.raises(ValueError):
        AP.pair_rows(7, 2, True, 3)


def test_head_mean_is_head_ordered():
    p = np.array([[[0.1, 0.9], [0.7, 0.3], [1e-8, 1.0]]], dtype=np.float32)
    want = ((p[:, 0] + p[:, 1]) + p[:, 2]) / np.float32(3)
    assert np.array_equal(AP.head_mean32(p), want)


def test_header_and_exports_carry_the_entry_points():
    from tempme_amd import _lib
    src = open(os.path.join(REPO, "include", "tempme.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("tm_tgn_attn_probs", "tm_tgat_attn_probs"):
        assert re.search(r"\bint\s+%s\s*\(const tm_t\w+_attn \*a, float \*probs, float \*mean, void \*stream\)" % name,
                         code), name
        assert name in _lib.EXPORTS
    import tempme_amd
    L = tempme_amd.lib()
    assert L.tm_tgn_attn_probs.argtypes == L.tm_tgat_attn_probs.argtypes
    assert len(L.tm_tgn_attn_probs.argtypes) == 4 and L.tm_version() == 3


# ------------------------------------------------------------------ baselines: host logic
def _batch(B=3, N=4, seed=0):
    from tempme_amd.train import Batch
    rng = np.random.default_rng(seed)
    sgs = []
    for _ in range(3):
        n1 = rng.integers(0, 5, (B, N))
        n2 = rng.integers(0, 3, (B, N * N))
        sgs.append(([torch.from_numpy(n1), torch.from_numpy(n2)], [torch.from_numpy(n1 * 0), torch.from_numpy(n2 * 0)],
                    [torch.zeros(B, N), torch.zeros(B, N * N)]))
    ev = torch.arange(1, B + 1)
    return Batch(ev, ev + 1, ev.double(), ev, ev + 2, sgs, None, None)


def test_unknown_method_is_a_value_error():
    from tempme_amd import baselines
    args = SimpleNamespace(base_type="tgn", n_degree=4, ratios=[0.5])
    with pytest.raises(ValueError, match="magic"):
        baselines.baseline_explanation("magic", args, None, _batch())
    with pytest.raises(ValueError, match="magic"):
        baselines.threshold_rows(args, None, _batch(), methods=("random", "magic"))
    with pytest.raises(NotImplementedError, match="jodie"):
        baselines.baseline_explanation("random", SimpleNamespace(base_type="jodie"), None, _batch())
    assert baselines.METHODS == ("attention", "saliency", "random")


def test_attention_on_a_base_without_attention_points_to_saliency():
    from tempme_amd import baselines

    class NoAttention:
        pass
    with pytest.raises(NotImplementedError, match="saliency"):
        baselines.attention_explanation(NoAttention(), _batch())
    with pytest.raises(NotImplementedError, match="saliency"):
        baselines.baseline_explanation("attention", SimpleNamespace(base_type="graphmixer"), NoAttention(), _batch())


@pytest.mark.parametrize("hops", [1, 2])
def test_random_explanation_masks_and_repeats(hops):
    from tempme_amd import baselines
    b = _batch()
    cpu = torch.device("cpu")
    e = baselines.random_explanation(b, 5, hops, cpu)
    nodes = baselines.node_records(b, cpu, hops)
    assert len(e) == hops and [tuple(x.shape) for x in e] == [(9, 4), (9, 16)][:hops]
    for x, n in zip(e, nodes):
        assert x.dtype == torch.float32 and x.device == cpu
        assert bool((x[n == 0] == 0).all()) and bool((x[n != 0] > 0).any()) and bool((x >= 0).all()) and bool((x < 1).all())
        assert bool((n == 0).any())
    again = baselines.random_explanation(b, 5, hops, cpu)
    other = baselines.random_explanation(b, 6, hops, cpu)
    assert all(torch.equal(x, y) for x, y in zip(e, again))
    assert not torch.equal(e[0], other[0])
    # the default device is where the batch's events live
    assert baselines.random_explanation(b, 5, hops)[0].device == cpu
    # hop-1 scores do not depend on whether hop-2 is drawn after them
    assert torch.equal(baselines.random_explanation(b, 5, 1, cpu)[0], baselines.random_explanation(b, 5, 2, cpu)[0])
