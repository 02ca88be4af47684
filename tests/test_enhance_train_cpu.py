"""The pooled encoder's training path (TempME.enhance_train_groups, tm_encoder_pool_train_fwd / _bwd / _wgrad), the
parts that need no GPU: the gradient index list against the header's documented order, the ctypes prototypes, the
masked restatement (tests/enhance_train_ref.py) against tests/enhance_ref.py, and the CPU device's unchanged
routing (the torch-op formulation, bitwise)."""
import os
import re

import numpy as np
import pytest
import torch

import enhance_inputs as XI
import enhance_ref as XR
import enhance_train_ref as TR
from enhance_inputs import make_explainer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tm_encoder_pool_train_workspace_bytes", "tm_encoder_pool_train_fwd", "tm_encoder_pool_bwd",
       "tm_encoder_pool_wgrad")


@pytest.fixture(scope="module")
def case():
    d = XI.load("uslegis")
    d["sd_all"] = dict(d["sd"], **d["aff"])
    return d


def test_pool_gradient_index_list_names_the_documented_parameters(case):
    """_POOL_IDX / _pool_params: the 16 tensors include/tempme.h lists for tm_encoder_pool_wgrad, in its order."""
    from tempme_amd import explainer as X
    hdr = open(os.path.join(REPO, "include", "tempme.h")).read()
    assert re.search(r"#define\s+TM_N_POOL_GRADS\s+16\b", hdr)
    doc = re.search(r"/\* Weight gradients of the pooled encoder.*?\*/", hdr, flags=re.S).group(0)
    doc = " ".join(l.strip(" *") for l in doc.splitlines())
    assert ("lin_event w/b, event_conv.MLP.0 w/b, .MLP.2 w/b, attention.W1 w/b, .W2 w/b, .MLP.0 w/b, .MLP.3 w/b, "
            "time_encoder.basis_freq, .phase") in doc
    assert X._POOL_IDX == tuple(range(14)) + (26, 27) and len(X._POOL_IDX) == 16
    assert set(X._POOL_IDX) < set(X._ENC_IDX) and set(X._ENC_IDX) - set(X._POOL_IDX) == set(range(14, 20))
    ex = make_explainer(case)
    named = {id(p): k for k, p in ex.named_parameters()}
    assert tuple(named[id(p)] for p in ex._pool_params()) == TR.POOL_PARAMS
    enc = ex._encoder_params()
    assert [id(p) for p in ex._pool_params()] == [id(enc[i]) for i in range(14)] + [id(enc[20]), id(enc[21])]


def test_new_prototypes_load():
    import tempme_amd
    from tempme_amd import _lib
    lib = tempme_amd.lib()
    for name in NEW:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None
    assert lib.tm_encoder_pool_train_workspace_bytes.restype is _lib.i64
    assert len(lib.tm_encoder_pool_train_fwd.argtypes) == 19
    assert len(lib.tm_encoder_pool_bwd.argtypes) == 20
    assert len(lib.tm_encoder_pool_wgrad.argtypes) == 8
    # host-side argument checks run before any device call
    assert lib.tm_encoder_pool_train_workspace_bytes(None, 0) >= lib.tm_encoder_workspace_bytes(None, 0)
    assert lib.tm_encoder_pool_train_fwd(*([None] * 3), 1, 1, 1, *([None] * 8), 1.0, None, None, 0, None) == _lib.TM_E_ARG
    assert lib.tm_encoder_pool_bwd(*([None] * 3), 1, 1, 1, *([None] * 8), 1.0, None, None, 0, None, None) == _lib.TM_E_ARG
    assert lib.tm_encoder_pool_wgrad(None, 1, 1, 1, None, None, None, None) == _lib.TM_E_ARG


def test_masked_restatement_without_masks_is_the_restatement(case):
    walks, cnt = XI.side_walks(case, "tgt", 5)
    cut = case["ts_cut"][:5]
    args = (case["sd_all"], case["n_feat"], case["e_feat"], case["deg"], walks, cut, cnt)
    want = XR.predict_walks(*args)
    assert torch.equal(TR.predict_walks(*args), want)
    ones = np.ones((5, 60, 66), dtype=np.uint8)
    assert torch.equal(TR.predict_walks(*args, keep=ones, scale=1.0), want)
    rng = np.random.default_rng(0)
    keep = (rng.uniform(0, 1, (5, 60, 66)) >= 0.5).astype(np.uint8)
    assert not torch.equal(TR.predict_walks(*args, keep=keep, scale=2.0), want)


def test_cpu_device_keeps_the_torch_formulation_bitwise(case):
    """On a CPU device enhance_predict_* route as before: results and gradients equal _enhance_agg_torch's bit for
    bit (eval mode with gradients: no dropout draws)."""
    ex = make_explainer(case).eval()
    ex.set_node_degree(case["deg"])
    assert not ex._enhance_train()
    B = 5
    sides = [XI.side_walks(case, s, B) for s in XI.SIDES]
    cut = case["ts_cut"][:B]

    def grads_of(fn):
        gats = [g[:B].clone().requires_grad_(True) for g in case["gats"]]
        ex.zero_grad()
        pos, neg = fn(gats)
        (pos.sum() + neg.sum()).backward()
        return pos.detach(), neg.detach(), [g.grad.clone() for g in gats], \
            {k: p.grad.clone() for k, p in ex.named_parameters() if p.grad is not None}

    a = grads_of(lambda g: ex.enhance_predict_agg(cut, sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides], *g))
    b = grads_of(lambda g: ex._enhance_agg_torch(cut, sides, g))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert set(a[3]) == set(b[3]) and set(TR.POOL_PARAMS) <= set(a[3])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    with torch.enable_grad():
        w = ex.enhance_predict_walks(sides[0][0], cut, sides[0][1])
        s, t = ex.enhance_predict_pairs(sides[0][0], sides[1][0], cut, sides[0][1], sides[1][1])
    assert torch.equal(w, ex._enhance_walks_torch(sides[0][0], cut, sides[0][1])) and torch.equal(w, s)
    assert torch.equal(t, ex._enhance_walks_torch(sides[1][0], cut, sides[1][1]))
    ex.train()
    assert not ex._enhance_train()
