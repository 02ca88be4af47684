"""Motif-enhanced link prediction (TempME.enhance_predict_*, explainer_new.py:203-306), the parts that need no GPU:
the torch restatement (tests/enhance_ref.py) against the reference's own outputs (tests/golden/enhance_uslegis.npz,
written by tests/golden/make_enhance_goldens.py), compute_node_degrees / set_node_degree, and the torch-op
formulation the module runs in training (or with gradients wanted) on CPU tensors, logits and gradients.

Tolerances come from the golden file: env_* = max |reference fp32 - restatement fp64| (the fp32 envelope of each
quantity), genv_* the same for each gradient; a second fp32 evaluation of the same function is asked to stay within
the envelope (the restatement, which repeats the reference's operations) or 10x it (the module's formulation, whose
products associate differently)."""
import numpy as np
import pytest
import torch

import enhance_inputs as XI
import enhance_ref as XR
from enhance_inputs import agg_with_grads, check_agg_against_golden, make_explainer


@pytest.fixture(scope="module")
def gold():
    return XI.golden()


@pytest.fixture(scope="module", params=XI.CASES)
def case(request):
    d = XI.load(request.param)
    d["case"] = request.param
    d["sd_all"] = dict(d["sd"], **d["aff"])
    return d


def test_restatement_fp32_matches_reference(case, gold):
    c = case["case"]
    env_emb, env_logit = float(gold[f"{c}_env_emb"]), float(gold[f"{c}_env_logit"])
    for bsz in XI.SUB_BATCHES:
        cut = case["ts_cut"][:bsz]
        for side in XI.SIDES:
            walks, cnt = XI.side_walks(case, side, bsz)
            wgt = XR.walk_importance(case["deg"], walks[2], walks[0], cut)
            dw = float(np.abs(wgt.numpy() - gold[f"{c}_wgt_{side}_{bsz}"]).max())
            emb = XR.predict_walks(case["sd_all"], case["n_feat"], case["e_feat"], case["deg"], walks, cut, cnt)
            de = float(np.abs(emb.numpy() - gold[f"{c}_emb_{side}_{bsz}"]).max())
            print(c, bsz, side, "wgt", dw, "emb", de, "envelope", env_emb)
            assert dw <= 1e-6
            assert de <= env_emb
    B = case["B"]
    sides = [XI.side_walks(case, s, B) for s in XI.SIDES]
    pos, neg, _ = XR.predict_agg(case["sd_all"], case["n_feat"], case["e_feat"], case["deg"], case["ts_cut"][:B], sides,
                                 case["gats"])
    dl = max(float(np.abs(pos.numpy() - gold[f"{c}_pos"]).max()), float(np.abs(neg.numpy() - gold[f"{c}_neg"]).max()))
    print(c, "logits", dl, "envelope", env_logit)
    assert dl <= env_logit


def test_reduce64_formula_is_within_the_envelope(case, gold):
    """What tm_walk_importance computes (fp32 elements, the three group reductions in fp64) against the golden."""
    c = case["case"]
    for bsz in XI.SUB_BATCHES:
        for side in XI.SIDES:
            walks, _ = XI.side_walks(case, side, bsz)
            wgt = XR.walk_importance(case["deg"], walks[2], walks[0], case["ts_cut"][:bsz], reduce64=True)
            assert float(np.abs(wgt.numpy() - gold[f"{c}_wgt_{side}_{bsz}"]).max()) <= 10 * float(gold[f"{c}_env_wgt"])


def test_compute_node_degrees_hand_count():
    import tempme_amd as tm
    # node 0 and node 4 isolated, node 2 has a self-loop (counted at both ends), node 5 is the largest id
    src, dst = [1, 2, 1, 5], [3, 2, 5, 1]
    want = [1.0, 3.0, 2.0, 1.0, 1.0, 2.0]
    got = tm.compute_node_degrees(src, dst)
    assert got.dtype == torch.float32 and got.tolist() == want
    assert tm.compute_node_degrees(np.array(src), torch.tensor(dst), 9).tolist() == want + [1.0, 1.0, 1.0]   # padded
    assert tm.compute_node_degrees(src, dst, 4).tolist() == want[:4]                                        # truncated
    u, i = XI.edge_list()
    assert np.array_equal(tm.compute_node_degrees(u, i, 224).numpy(), XI.node_degrees(224))
    with pytest.raises(ValueError):
        tm.compute_node_degrees([1, 2], [1])


def test_set_node_degree_validates_length(case):
    ex = make_explainer(case)
    n = case["n_feat"].shape[0]
    assert ex.node_degree.shape == (n,) and bool((ex.node_degree == 1).all())
    ex.set_node_degree(case["deg"])
    assert ex.node_degree.dtype == torch.float32 and np.array_equal(ex.node_degree.numpy(), case["deg"])
    for bad in (np.ones(n - 1, dtype=np.float32), np.ones(n + 1, dtype=np.float32), np.ones((n, 1), dtype=np.float32)):
        with pytest.raises(ValueError):
            ex.set_node_degree(bad)
    assert "node_degree" not in ex.state_dict()          # a plain attribute, as in the reference


def test_torch_formulation_on_cpu_matches_reference_logits_and_gradients(case, gold):
    ex = make_explainer(case).eval()             # eval: no dropout, as the golden; gradients wanted -> torch ops
    ex.set_node_degree(case["deg"])
    pos, neg, grads = agg_with_grads(ex, case)
    check_agg_against_golden(pos, neg, grads, gold, case["case"])
    # the pieces, per side: [bsz, n_walk] weights and [bsz, hid + 12] embeddings
    walks, cnt = XI.side_walks(case, "tgt", 5)
    with torch.no_grad():
        wgt = ex.compute_walk_importance(walks[2], walks[0], case["ts_cut"][:5])
        emb = ex.enhance_predict_walks(walks, case["ts_cut"][:5], cnt)
    c = case["case"]
    assert tuple(wgt.shape) == (5, 60) and tuple(emb.shape) == (5, 76)
    assert float(np.abs(wgt.numpy() - gold[f"{c}_wgt_tgt_5"]).max()) <= 1e-6
    assert float(np.abs(emb.numpy() - gold[f"{c}_emb_tgt_5"]).max()) <= 10 * float(gold[f"{c}_env_emb"])


def test_forward_torch_is_unchanged_by_the_split(case):
    """_forward_torch (now _attention_torch + the scoring MLP) still gives the committed graphlet importances."""
    ex = make_explainer(case).eval()
    walks, cnt = XI.side_walks(case, "src", 32)
    with torch.no_grad():
        imp = ex._forward_torch(walks, case["ts_cut"], cnt)
    np.testing.assert_allclose(imp.numpy(), case["src"]["imp"], rtol=1e-5, atol=1e-6)
