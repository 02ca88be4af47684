"""CPU-side checks: the C-ABI library builds for gfx950, loads, and exports every symbol the
header declares (no compute calls without a GPU); host logic that needs no device."""
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(REPO, "include", "tempme.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_known_surface():
    fns = header_functions()
    for f in ("tm_graph_build", "tm_sample_khop", "tm_sample_walks", "tm_sample_events", "tm_encoder_fwd",
              "tm_edge_importance", "tm_motif_hist", "tm_edge_counts", "tm_neg_sample", "tm_last_error"):
        assert f in fns


def test_library_exports_every_header_symbol():
    import tempme_amd
    from tempme_amd import _lib
    L = tempme_amd.lib()
    for f in header_functions():
        assert hasattr(L, f), f
    assert set(header_functions()) == set(_lib.EXPORTS)
    assert L.tm_version() == 3


def test_library_is_gfx950_code_object():
    from tempme_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob


def test_no_oracle_in_product():
    """The product package never imports the checker."""
    pkg = os.path.join(REPO, "tempme_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(root, f)).read()
                assert "oracle" not in re.sub(r'""".*?"""', "", txt, flags=re.S).replace("# ", ""), f


def test_requires_gpu_loudly():
    import torch
    import pytest
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import tempme_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tempme_amd.NeighborFinder.from_edges([1], [2], [1], [1.0], 3)


def test_adjacency_construction_matches_oracle():
    from oracle.oracle import adjacency_from_edges as a_or
    from tempme_amd.graph import adjacency_from_edges as a_tm
    rng = np.random.RandomState(0)
    src, dst = rng.randint(0, 20, 300), rng.randint(0, 20, 300)
    ts, e = np.sort(rng.randint(0, 50, 300)).astype(float), np.arange(1, 301)
    for x, y in zip(a_or(src, dst, e, ts, 20), a_tm(src, dst, e, ts, 20)):
        assert np.array_equal(x, y)


def test_flops_model_matches_survey():
    import bench
    fm = bench.flops_model(32, 172, 64, 20, 3)
    # 315,500 MAC = 631,000 FLOP per walk at Enron dims (lin_event shared)
    assert abs(fm["per_walk"] - 631_000) / 631_000 < 1e-3
    assert bench.sampling_bytes_per_event(20, 3) == 78_816
    assert bench.sampling_bytes_per_event(30, 3) == 143_376


def test_encoder_workspace_sizes():
    """Python callers size their buffers from these three calls, and the backward reads F and the groups' std at the
    offsets the forward wrote them: the byte counts are pinned.  No device is touched.  The size functions read only
    tm_weights::h -- the struct begins with int device, de, dn, h (csrc/encoder_common.h) -- so a zeroed block with
    that field set stands in for weights at hid_dim 32 (creating real ones needs a GPU); NULL means hid_dim 64."""
    import ctypes as C
    import tempme_amd
    L = tempme_amd.lib()
    want = {   # (h, n_walks): (tm_encoder_workspace_bytes, the two pooled sizes)
        (32, 0): (512, 768), (32, 1): (1284, 1920), (32, 42): (32936, 38656), (32, 2 ** 20): (809501184, 943719168),
        (64, 0): (512, 768), (64, 1): (2052, 2816), (64, 42): (65192, 76288), (64, 2 ** 20): (1614807552, 1883243264),
    }
    for (h, n), (plain, pool) in want.items():
        # the layout itself: F [n][3][2h] | std, n + 64 floats | 256 spare bytes; pooled: that rounded up to 256,
        # then the partials [n][h] and 256 spare bytes
        assert plain == 4 * (6 * h * n + n + 64) + 256 and pool == (plain + 255) // 256 * 256 + 4 * h * n + 256
        block = (C.c_int32 * 4096)()
        block[3] = h
        for w in ([C.addressof(block)] + ([None] if h == 64 else [])):
            assert L.tm_encoder_workspace_bytes(w, n) == plain, (h, n)
            assert L.tm_encoder_pool_workspace_bytes(w, n) == pool, (h, n)
            assert L.tm_encoder_pool_train_workspace_bytes(w, n) == pool, (h, n)


def test_encoder_train_supported_is_pinned():
    """tm_encoder_train_supported decides whether Python takes the HIP training path at all; it is a pure host
    function (no device), and its answers over edge_dim x node_dim x hid_dim x if_cat are pinned here: per
    (hid_dim, cat) one digit per (de, dn), de-major.  hid_dim must be a multiple of 16 up to 256; past that the
    three LDS sizes decide.  Both answers occur with head_bwd_kernel's tile the only one deciding (hid_dim 192
    against 256, and 208 with and without the category columns) and with gcn_bwd_kernel's (dn 176 against 1024 at
    hid_dim 64).  The gate's tile can never be the only one over the budget: its bytes, 128 (r16(de + dn) + r16(h) +
    r16(h / 2) + 24), are below gcn_bwd_kernel's, at least 128 (r16(de + 3 + dn) + 8) + 256 (r16(dn) + 8) +
    256 (h + 8), for every h >= 16 -- so no grid shows it deciding, and it is pinned through the other two."""
    import tempme_amd
    L = tempme_amd.lib()
    DE, DN = (1, 4, 32, 172, 512, 4096), (4, 172, 176, 1024, 8192)
    none = "0" * 30
    want = {
        (0, 0): none, (0, 1): none, (8, 0): none, (8, 1): none,
        (16, 0): "111001110011100111001110000000", (16, 1): "111001110011100111001110000000",
        (32, 0): "111001110011100111001110000000", (32, 1): "111001110011100111001110000000",
        (64, 0): "111001110011100111001000000000", (64, 1): "111001110011100111001000000000",
        (128, 0): "111001110011100111001000000000", (128, 1): "111001110011100111001000000000",
        (192, 0): "111001110011100111001000000000", (192, 1): "111001110011100111001000000000",
        (208, 0): "100001000010000100001000000000", (208, 1): none,
        (256, 0): none, (256, 1): none, (272, 0): none, (272, 1): none,
    }
    for (h, cat), row in want.items():
        got = "".join(str(L.tm_encoder_train_supported(de, dn, h, cat)) for de in DE for dn in DN)
        assert got == row, (h, cat, got)


def test_dropin_extension_loads(monkeypatch):
    """The drop-in fast path's C++ host side (csrc/dropin_ext.cpp, built by build(), used whenever it is built)
    imports on the CPU and exposes its entry points (constructing one needs a HIP device)."""
    from tempme_amd import explainer as X
    monkeypatch.setattr(X, "_EXT", [None, False])
    m = X._dropin_ext()
    assert m is not None, "tempme_amd/lib/_dropin_ext*.so missing: python tempme_amd/_build_ext.py"
    for name in ("forward", "retrieve", "push", "current"):
        assert hasattr(m.Fast, name)
