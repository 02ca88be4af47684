"""Host-side pieces of the explainer drivers over a TGAT base (tempme_amd/train.py, evaluate.py): the views of
the stacked explanation weights, explain_sides off the HIP path, the dispatch on the base, the exported names."""
import numpy as np
import pytest
import torch

import tgat_inputs as TA
import tgn_inputs as TI
from tests.encoder_inputs import SIDES, load as load_enc


def test_split_stacked_weights_returns_views():
    from tempme_amd.train import split_stacked_weights
    B, N = 5, 4
    ew1 = torch.arange(3 * B * N, dtype=torch.float32).reshape(3 * B, N)
    ew2 = torch.arange(3 * B * N * N, dtype=torch.float32).reshape(3 * B, N * N)
    (s, t), (s2, b) = split_stacked_weights(ew1, ew2)
    assert s is s2                                    # contrast then runs the src side once
    six = split_stacked_weights(ew1, ew2, flat=True)
    assert len(six) == 6
    for side, pair in enumerate((s, t, b)):
        for h, (x, base) in enumerate(zip(pair, (ew1, ew2))):
            assert x.shape == (B, base.shape[1]) and x.is_contiguous()
            assert x.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
            assert x.data_ptr() == base.data_ptr() + side * B * base.shape[1] * base.element_size()
            y = six[2 * side + h]
            assert y.data_ptr() == x.data_ptr() and y.shape == x.shape
    # gradients flow back to the two tensors through the views
    e1, e2 = ew1.clone().requires_grad_(True), ew2.clone().requires_grad_(True)
    (s, t), (_, b) = split_stacked_weights(e1, e2)
    (s[0].sum() + 2 * t[1].sum() + 3 * b[0].sum()).backward()
    assert torch.equal(e1.grad[:B], torch.ones(B, N)) and torch.equal(e2.grad[B:2 * B], torch.full((B, N * N), 2.0))
    assert torch.equal(e1.grad[2 * B:], torch.full((B, N), 3.0)) and float(e2.grad[:B].abs().sum()) == 0
    with pytest.raises(ValueError, match="3B rows"):
        split_stacked_weights(ew1[:7], ew2[:7])


def _host_batch(case="uslegis", B=4):
    from tempme_amd.train import Batch
    enc, d = load_enc(case), TI.load_batch()
    walks = [tuple(enc[s][k][:B] for k in ("node", "eid", "ts", "cat", "marg")) for s in SIDES]
    sgs = [tuple([x[:B] for x in d["sg_" + s][i]] for i in range(3)) for s in SIDES]
    return Batch(d["src"][:B], d["dst"][:B], d["ts_cut"][:B], d["e_idx"][:B], d["fake"][:B], sgs, walks,
                 [enc[s]["cnt"][:B] for s in SIDES])


class _HostExplainer:
    """The explainer's interface as explain_sides uses it off the HIP path.  TempME itself needs the HIP device
    for every retrieve_edge_imp_node call, so the host-side check runs on this stand-in: per-side outputs that
    depend on the side's subgraph and importances, and a record of the calls."""

    def __init__(self, base_type):
        self.base_type, self.calls = base_type, []

    def _hip_ok(self):
        return False

    def retrieve_edge_imp_node(self, subgraph, graphlet_imp, walks, training=True):
        self.calls.append(("node", training))
        n1, n2 = (torch.from_numpy(np.asarray(x, dtype=np.float32)) for x in subgraph[0])
        w = graphlet_imp.reshape(graphlet_imp.shape[0], -1).mean(1, keepdim=True)
        return n1 * w, n2 * w

    def retrieve_explanation(self, sg_s, g_s, w_s, sg_t, g_t, w_t, sg_b, g_b, w_b, training=True):
        self.calls.append(("all", training))
        pairs = [self.retrieve_edge_imp_node(sg, g, w, training) for sg, g, w in
                 ((sg_s, g_s, w_s), (sg_t, g_t, w_t), (sg_b, g_b, w_b))]
        out = [torch.cat([p[h] for p in pairs]) for h in (0, 1)]
        return out if self.base_type == "tgn" else out[:1]


def test_explain_sides_fallback_returns_both_hops():
    """Off the HIP path explain_sides gives a TGAT base's two [3B, ...] tensors: three retrieve_edge_imp_node calls
    concatenated in side order (retrieve_explanation keeps hop-2 for a TGN base only, so it is not the route)."""
    from tempme_amd.train import explain_sides
    b = _host_batch()
    B, N = len(b), TI.N_DEG
    gen = torch.Generator().manual_seed(1)
    imps = [torch.rand(B, np.shape(w[1])[1], 1, generator=gen) for w in b.walks]
    ex = _HostExplainer("tgat")
    e1, e2 = explain_sides(ex, b, imps, False)
    assert ex.calls == [("node", False)] * 3
    pairs = [ex.retrieve_edge_imp_node(sg, g, w, training=False) for sg, g, w in zip(b.subgraphs, imps, b.walks)]
    assert e1.shape == (3 * B, N) and e2.shape == (3 * B, N * N)
    assert torch.equal(e1, torch.cat([p[0] for p in pairs])) and torch.equal(e2, torch.cat([p[1] for p in pairs]))
    assert float(e2.abs().sum()) > 0 and not torch.equal(e1[:B], e1[B:2 * B])
    # the other bases keep retrieve_explanation's route and its list
    for base_type, n in (("tgn", 2), ("graphmixer", 1)):
        ex = _HostExplainer(base_type)
        out = explain_sides(ex, b, imps, True)
        assert len(out) == n and ex.calls[0] == ("all", True) and torch.equal(out[0], e1)


def test_base_is_tgat_names_both_sides_of_a_mismatch():
    from tempme_amd.train import base_is_tgat
    tgat = TA.build_model("uslegis")
    tgn = TI.build_model("uslegis")
    ex = lambda t: type("E", (), {"base_type": t})()  # noqa: E731
    assert base_is_tgat(ex("tgat"), tgat) is True and base_is_tgat(ex("tgn"), tgn) is False
    with pytest.raises(ValueError, match="(?s)'tgn'.*TGAT"):
        base_is_tgat(ex("tgn"), tgat)
    with pytest.raises(ValueError, match="(?s)'tgat'.*TGN"):
        base_is_tgat(ex("tgat"), tgn)


def test_new_names_are_exported():
    import inspect

    import tempme_amd.train as T
    from tempme_amd import TGAT, evaluate
    for name in ("base_is_tgat", "split_stacked_weights", "explained_contrast", "explain_sides", "prepare_step"):
        assert callable(getattr(T, name)) and name in T.__all__
    assert callable(TGAT.prepare_contrast)
    params = inspect.signature(TGAT.contrast).parameters
    assert "prepared" in params and "stacked_weights" in params
    # the reference's positional signature is unchanged
    assert list(params)[1:12] == ["src_idx_l", "tgt_idx_l", "bgd_idx_l", "cut_time_l", "e_idx_l", "subgraph_src",
                                  "subgraph_tgt", "subgraph_bgd", "test", "if_explain", "exp_weights"]
    assert evaluate.split_stacked_weights is T.split_stacked_weights
