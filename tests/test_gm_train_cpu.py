"""Base-GraphMixer training (learn_base.py for --base_type graphmixer) on the CPU: the torch formulation of the
training step (tests/gm_train_ref.py) against the reference's own step (tests/golden/graphmixer_train.npz),
learn_base.split_data on the uslegis fixture, and the C ABI of the HIP training pair."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gm_train_ref as GR
import tgn_inputs as TI
from tests.test_graphmixer_oracle import ATOL, CASES, RTOL, build

DATA = os.path.join(TI.G, "data", "ml_uslegis_sampled.csv")


def train_golden():
    return np.load(os.path.join(TI.G, "graphmixer_train.npz"))


def golden_batch():
    d = TI.load_batch()
    return (d["src"], d["dst"], d["fake"], d["ts_cut"], d["sg_src"], d["sg_tgt"], d["sg_bgd"])


def sibling_bias(name):
    return name[:-len("weight")] + "bias"


@pytest.mark.parametrize("case", CASES)
def test_fp64_formulation_matches_reference_step(case):
    """keep = None, fp64: logits within the eval oracle's ATOL / RTOL of the reference's, the loss with them, and
    every parameter gradient within 1e-5 relative norm of the reference's.

    One kind of tensor has no relative norm to measure against: with a single channel (uslegis, C = 1) the channel
    LayerNorm normalises one value, its output is its bias, and the gradient of channel_norm.weight is exactly
    zero; the reference's fp32 step leaves rounding residue there (norms 1.2e-8, 1.2e-9, 5.2e-12 for the three
    layers, against 3.0e-3, 8.0e-4, 1.4e-4 for the bias of the same LayerNorm, which sums the same dY).  A tensor
    whose fp64 gradient is identically zero (below 1e-12 of its sibling bias gradient) is therefore held to the
    same 1e-5, taken of the sibling bias gradient's norm."""
    g = train_golden()
    m = build(case)
    loss, pos, neg, grads = GR.loss_and_grads(m.state_dict(), 3, golden_batch(), dtype=torch.float64)
    np.testing.assert_allclose(pos.numpy(), g[f"{case}_pos"], atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(neg.numpy(), g[f"{case}_neg"], atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(float(loss), float(g[f"{case}_loss"]), atol=ATOL, rtol=RTOL)
    names = [str(k) for k in g[f"{case}_grad_names"]]
    assert set(names) == {k for k, v in m.named_parameters() if v.requires_grad}
    assert len(names) == 2 + 12 * 3 + 2 + 4
    for k in names:
        ref = g[f"{case}_grad_{k}"].astype(np.float64)
        got = grads[k].numpy()
        err, nref = np.linalg.norm(got - ref), np.linalg.norm(ref)
        if k.endswith("norm.weight"):
            nb = np.linalg.norm(g[f"{case}_grad_{sibling_bias(k)}"].astype(np.float64))
            if np.linalg.norm(got) <= 1e-12 * nb:
                assert err <= 1e-5 * nb, (k, err, nb)
                continue
        assert err <= 1e-5 * nref, (k, err, nref)


def test_keep_masks_change_the_step_and_scale():
    """The mask layout: all-ones masks with keep_scale 1 are the no-dropout step; a zeroed ch_o part of the last
    layer removes that layer's channel FFN from the output."""
    m = build("synth")
    sd, batch = m.state_dict(), golden_batch()
    R, N, C = 3 * TI.BSZ, TI.N_DEG, m.num_channels
    HT, HC = N // 2, 4 * C
    per = R * (C * HT + C * N + N * HC + N * C)
    ones = torch.ones(3 * per, dtype=torch.uint8)
    l0, p0, n0, _ = GR.loss_and_grads(sd, 3, batch)
    l1, p1, n1, _ = GR.loss_and_grads(sd, 3, batch, keep=ones, keep_scale=1.0)
    assert torch.equal(p0, p1) and torch.equal(n0, n1)
    z = ones.clone()
    z[3 * per - R * N * C:] = 0
    _, p2, _, g2 = GR.loss_and_grads(sd, 3, batch, keep=z, keep_scale=1.0)
    assert not torch.equal(p0, p2)
    assert float(g2["mlp_mixers.2.channel_feedforward.ffn.3.weight"].abs().max()) == 0.0
    assert float(g2["mlp_mixers.2.token_feedforward.ffn.3.weight"].abs().max()) > 0.0


def _csv():
    import pandas as pd
    return pd.read_csv(DATA)


def test_split_data_is_chronological_masked_and_seeded():
    from tempme_amd.learn_base import split_data
    g_df = _csv()
    s = split_data(g_df, seed=2023, finders=False)
    ts = g_df.ts.values
    assert [s.val_time, s.test_time] == list(np.quantile(ts, [0.70, 0.85]))
    assert s.train_ts_l.max() <= s.val_time < s.val_ts_l.min()
    assert s.val_ts_l.max() <= s.test_time < s.test_ts_l.min()
    assert len(s.val_ts_l) + len(s.test_ts_l) == int((ts > s.val_time).sum())
    # 10 % of all nodes, all of them seen after val_time, none of them in a training edge
    nodes = np.unique(np.hstack([g_df.u.values, g_df.i.values]))
    assert len(s.mask_node_set) == int(0.1 * len(nodes))
    later = set(g_df.u.values[ts > s.val_time]) | set(g_df.i.values[ts > s.val_time])
    assert s.mask_node_set <= later
    assert not (set(s.train_src_l) | set(s.train_dst_l)) & s.mask_node_set
    early = ts <= s.val_time
    clean = ~np.isin(g_df.u.values, list(s.mask_node_set)) & ~np.isin(g_df.i.values, list(s.mask_node_set))
    assert np.array_equal(s.train_e_idx_l, g_df.idx.values[early & clean])
    assert 0 < len(s.train_e_idx_l) < int(early.sum())
    # the same seed gives the same split, another seed another mask
    s2 = split_data(g_df, seed=2023, finders=False)
    assert s2.mask_node_set == s.mask_node_set and np.array_equal(s2.train_e_idx_l, s.train_e_idx_l)
    assert split_data(g_df, seed=7, finders=False).mask_node_set != s.mask_node_set


def test_learn_base_cli_rejects_other_bases():
    from tempme_amd import learn_base
    for base in ("tgn", "tgat"):
        with pytest.raises(NotImplementedError, match="GraphMixer"):
            learn_base.main(["--base_type", base, "-d", "uslegis_sampled"])


def test_library_exports_the_training_pair():
    """The four new symbols, and tm_gm_train_ok at learn_base.py's default dims (C = T = 172, N = 30, L = 3)."""
    from tempme_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tm_gm_train_ok", "tm_gm_train_workspace_bytes", "tm_gm_train_fwd", "tm_gm_train_bwd"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    ok = lib.tm_gm_train_ok
    ok.argtypes = [ctypes.c_int32] * 6
    assert ok(30, 172, 172, 3, 15, 688) == 1
    assert ok(33, 172, 172, 3, 15, 688) == 0
    assert ok(32, 256, 256, 4, 16, 1024) == 1
    assert ok(30, 172, 172, 5, 15, 688) == 0 and ok(30, 257, 172, 3, 15, 1028) == 0 and ok(30, 172, 172, 3, 17, 688) == 0
    wb = lib.tm_gm_train_workspace_bytes
    wb.restype = ctypes.c_int64
    wb.argtypes = [ctypes.c_int64] + [ctypes.c_int32] * 6
    R, N, C, T, Lr, HT, HC = 60, 30, 172, 172, 3, 15, 688
    # at least the projection input, the L layer inputs and d X
    assert wb(R, N, C, T, Lr, HT, HC) >= 4 * R * N * ((C + T) + (Lr + 1) * C)
    assert wb(R, 33, C, T, Lr, HT, HC) == -1
    # the layer inputs live in the workspace: one more layer costs one more [R N][C] image, nothing else
    assert wb(R, N, C, T, 4, HT, HC) - wb(R, N, C, T, 3, HT, HC) == 4 * R * N * C
