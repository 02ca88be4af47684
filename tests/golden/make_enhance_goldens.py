"""Generate tests/golden/enhance_uslegis.npz by running the REFERENCE TempME itself on the CPU.

    python tests/golden/make_enhance_goldens.py <path to a checkout of dharunm236/TempME>

Run where the reference is available; the tests only read the committed .npz.  Nothing of the reference is stored
but what its programs compute.

Inputs are the committed fixtures tests/enhance_inputs.py loads: the uslegis walks of the first 32 test events
(N = 20, W = 60, three sides), both feature cases (``uslegis``: zero node features and a 1-wide edge feature;
``synth``: non-zero node features and a 32-wide edge feature), the committed encoder weights, node degrees counted
from tests/golden/data/ml_uslegis_sampled.csv, and affinity_score's weights and the three ``*_gat`` inputs drawn from
numpy.default_rng(seed) (not stored: redrawn by the tests).  Per case, in eval mode and fp32:
  * for every sub-batch size the tests run (the statistics of compute_walk_importance and of the attention are per
    call) and every side: ``wgt`` = compute_walk_importance and ``emb`` = enhance_predict_walks;
  * ``pos`` / ``neg`` of enhance_predict_agg on the 32 events;
  * the gradients of pos.sum() + neg.sum() with respect to affinity_score.fc1.weight, attention.W1.weight,
    event_conv.lin_event.weight and src_gat (of fc1.weight's 248 x 496 gradient every second row, all columns:
    the whole matrix of both cases alone would exceed the 1 MB a committed file may have);
  * the fp32 envelopes: max |reference fp32 - tests/enhance_ref.py in fp64| of wgt, emb and the logits (the GPU
    tests' tolerances are 10x these, read from the file), and the same distance for each gradient.
The generator asserts that the group std of the walks' mean degree exceeds 1.0 for every side and sub-batch:
below ~1e-6 (the all-ones default) the degree weights are rounding noise and no parity can be asked for.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import enhance_inputs as XI  # noqa: E402
import enhance_ref as XR  # noqa: E402


def import_reference(ref):
    """models.explainer_new with the two imports the encoder does not need stubbed: torch_scatter (kl_loss and
    retrieve_edge_imp_node only) and utils.get_null_distribution (kl_loss only; it samples the whole graph)."""
    tsc = types.ModuleType("torch_scatter")
    tsc.scatter = None
    sys.modules["torch_scatter"] = tsc
    ut = types.ModuleType("utils")
    ut.get_null_distribution = lambda data_name: {}
    sys.modules["utils"] = ut
    sys.path.insert(0, ref)
    from models.explainer_new import TempME
    return TempME


class Base:
    def __init__(self, n_feat, e_feat):
        self.n_feat_th, self.e_feat_th = n_feat, e_feat
        self.node_raw_features = torch.nn.Embedding.from_pretrained(n_feat, padding_idx=0, freeze=True)
        self.edge_raw_features = torch.nn.Embedding.from_pretrained(e_feat, padding_idx=0, freeze=True)


def main(ref):
    TempME = import_reference(ref)
    res = {"sub_batches": np.array(XI.SUB_BATCHES)}
    for case in XI.CASES:
        d = XI.load(case)
        torch.manual_seed(0)
        ex = TempME(Base(d["n_feat"], d["e_feat"]), base_model_type="tgn", data="uslegis_sampled", out_dim=40,
                    hid_dim=64, temp=0.07, if_cat_feature=True, dropout_p=0.1, device=torch.device("cpu"))
        sd = dict(d["sd"])
        sd.update(d["aff"])
        missing, unexpected = ex.load_state_dict(sd, strict=False)
        used = ("event_conv", "attention.W1", "attention.W2", "attention.MLP", "affinity_score", "time_encoder")
        assert not unexpected and not [k for k in missing if k.startswith(used)]
        ex.node_degree = torch.from_numpy(d["deg"])
        ex.eval()
        sd64 = {k: v.double() for k, v in sd.items()}
        env = {"wgt": 0.0, "emb": 0.0, "logit": 0.0}
        for bsz in XI.SUB_BATCHES:
            cut = d["ts_cut"][:bsz]
            for side in XI.SIDES:
                walks, cnt = XI.side_walks(d, side, bsz)
                s_avg = XR.avg_degree_std(d["deg"], walks[0])
                assert s_avg > 1.0, (case, bsz, side, s_avg)
                with torch.no_grad():
                    wgt = ex.compute_walk_importance(walks[2], walks[0], cut)
                    emb = ex.enhance_predict_walks(walks, cut, cnt)
                res[f"{case}_wgt_{side}_{bsz}"] = wgt.numpy()
                res[f"{case}_emb_{side}_{bsz}"] = emb.numpy()
                w64 = XR.walk_importance(d["deg"], walks[2], walks[0], cut, dtype=torch.float64)
                e64 = XR.predict_walks(sd64, d["n_feat"], d["e_feat"], d["deg"], walks, cut, cnt)
                env["wgt"] = max(env["wgt"], float((wgt.double() - w64).abs().max()))
                env["emb"] = max(env["emb"], float((emb.double() - e64).abs().max()))
                print(case, bsz, side, "std(avg degree)", round(s_avg, 2))
        B = d["B"]
        cut = d["ts_cut"][:B]
        sides = [XI.side_walks(d, s, B) for s in XI.SIDES]
        gats = [g.clone().requires_grad_(k == 0) for k, g in enumerate(d["gats"])]
        pos, neg = ex.enhance_predict_agg(cut, sides[0][0], sides[1][0], sides[2][0], [s[1] for s in sides], *gats)
        (pos.sum() + neg.sum()).backward()
        res[f"{case}_pos"], res[f"{case}_neg"] = pos.detach().numpy(), neg.detach().numpy()
        params = dict(ex.named_parameters())
        g32 = {k: params[k].grad for k in XI.GRAD_KEYS}
        g32["src_gat"] = gats[0].grad
        # the same function in fp64 (tests/enhance_ref.py) for the envelopes
        p64 = {k: v.clone().requires_grad_(k in XI.GRAD_KEYS) for k, v in sd64.items()}
        gat64 = [g.double().requires_grad_(k == 0) for k, g in enumerate(d["gats"])]
        pos64, neg64, _ = XR.predict_agg(p64, d["n_feat"], d["e_feat"], d["deg"], cut, sides, gat64)
        (pos64.sum() + neg64.sum()).backward()
        env["logit"] = float(max((pos.detach().double() - pos64.detach()).abs().max(),
                                 (neg.detach().double() - neg64.detach()).abs().max()))
        g64 = {k: p64[k].grad for k in XI.GRAD_KEYS}
        g64["src_gat"] = gat64[0].grad
        for k, g in g32.items():
            g_st = g[::XI.FC1_ROW_STEP] if k == "affinity_score.fc1.weight" else g
            res[f"{case}_grad_{k}"] = g_st.numpy().astype(np.float32)
            res[f"{case}_genv_{k}"] = np.array(float((g.double() - g64[k]).abs().max()))
            print(case, "grad", k, "max |g|", float(g.abs().max()), "fp32 envelope", float(res[f"{case}_genv_{k}"]))
        for k, v in env.items():
            res[f"{case}_env_{k}"] = np.array(v)
        print(case, "pos", float(pos.mean()), "neg", float(neg.mean()), "fp32 envelopes", env)
    out = os.path.join(HERE, "enhance_uslegis.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
