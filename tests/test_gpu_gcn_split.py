"""walk_kernel's event_gcn first layer on bf16 MFMA in the zero-node family (v_mfma_f32_16x16x32_bf16 over pair
steps of two input tiles, both operands split exactly into three bf16 parts, six products per (tile, step), fp32
accumulation from the bias; EncW::g13, half of it resident in LDS) against oracle/encoder_ref.forward (CPU, torch fp32) at the project's
contract rtol=1e-5, atol=1e-6, with tests/test_gpu_lin_split.py's synthetic walks:

* de = 32 with zero node features in table mode (the zero-node instance, the converted one), de = 172 with node
  features in table and plain mode (the two-branch instances, whose first layer stays on fp32 MFMA: dn = 172's
  last tile has four padded rows that the clamped node loads fill with a duplicate), and de = 1;
* M = 1 and 3; 7 events (split form, last unit partial) and 3 x 137 events (persistent form, 514 units);
* null positions and null slots (in the walks);
* lin_event outputs the new layer can get wrong: every one negative (bias -50: the layer multiplies all-zero
  activations and H = relu(b)), |L| up to ~1e4 and |L| ~ 1e-6 (lin_event's weight and bias scaled).

Also: the persistent launch equals the per-group split launches bit for bit in every one of those weight sets,
and the error against the float64 oracle stays within twice the fp32-MFMA parent build's on the same input.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_lin_split import ATOL, BIG, CONFIGS, N, N_EDGES, N_NODES, RTOL, SMALL, _close, _walks

pytestmark = pytest.mark.gpu

# lin_event's (weight scale, bias shift) per weight set
VARIANTS = {"plain": (1.0, 0.0), "neg": (1.0, -50.0), "big": (1e3, 0.0), "tiny": (1e-7, 0.0)}

# max |imp - float64 oracle| of the parent commit's build of the library (fp32-MFMA first layer) on
# budget_case()'s input, measured once on an MI355X with this file's test_error_budget (it prints the figure
# before it asserts); DESIGN section 6p records the run
PARENT_MAX_ERR64 = 5.383e-08


@functools.lru_cache(maxsize=None)
def _model(cfg, variant="plain"):
    import tempme_amd as tm
    de, dn, node_feat = CONFIGS[cfg]
    rng = np.random.RandomState(5)
    e_feat = rng.uniform(0, 1, (N_EDGES + 1, de)).astype(np.float32)
    e_feat[0] = 0
    n_feat = np.zeros((N_NODES + 1, dn), np.float32)
    if node_feat != "zeros":
        n_feat[1:] = rng.uniform(0, 1, (N_NODES, dn))
    dev = torch.device("cuda", 0)

    class Base:
        n_feat_th = torch.from_numpy(n_feat)
        e_feat_th = torch.from_numpy(e_feat)
        node_raw_features = torch.nn.Embedding.from_pretrained(n_feat_th, padding_idx=0, freeze=True)
        edge_raw_features = torch.nn.Embedding.from_pretrained(e_feat_th, padding_idx=0, freeze=True)

    torch.manual_seed(7)
    ex = tm.TempME(Base(), "tgn", "synthetic", 40, 64, device=dev,
                   null_model={k: 1 / 12 for k in range(1, 13)}).to(dev).eval()
    scale, shift = VARIANTS[variant]
    prm = dict(ex.named_parameters())
    with torch.no_grad():
        prm["event_conv.lin_event.weight"].mul_(scale)
        prm["event_conv.lin_event.bias"].mul_(scale).add_(shift)
    sd = {k: v.detach().cpu().clone() for k, v in ex.state_dict().items()}
    return ex, sd, torch.from_numpy(n_feat), torch.from_numpy(e_feat)


def _launch(cfg, variant, walks, table, M, groups=None):
    ex, _, _, _ = _model(cfg, variant)
    dev = torch.device("cuda", 0)
    if groups is not None:
        walks = tuple(a[groups] for a in walks)
    G, B, W = walks[1].shape[:3]
    etab = None
    if table:
        etab = ex.dropin_edge_table()
        assert etab is not None, "no table mode for these dims"
    node6, eid3, ts3, cat, cut, cnt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in walks)
    out = ex.encoder_fwd(node6, eid3, ts3, cat, cut, cnt, G, B, W, M=M, etab=etab)
    torch.cuda.synchronize()
    assert ex._node_zero == (CONFIGS[cfg][2] == "zeros")
    return out.cpu().numpy().reshape(G, B, W)


@functools.lru_cache(maxsize=None)
def _oracle(cfg, variant, G, B, M, double=False):
    from oracle import encoder_ref as er
    _, sd, nf, ef = _model(cfg, variant)
    if double:
        sd = {k: v.double() for k, v in sd.items()}
    node6, eid3, ts3, cat, cut, cnt = _walks(G, B, M)
    out = [er.forward(sd, nf, ef, node6[g], eid3[g], ts3[g], cat[g], cut[g], cnt[g].astype(np.float64)).numpy()[..., 0]
           for g in range(G)]
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _lin_event_range(cfg, variant, G, B, M):
    """min and max of lin_event's output over the walks' valid positions and real features (CPU, fp32)."""
    from oracle import encoder_ref as er
    _, sd, _, ef = _model(cfg, variant)
    node6, eid3, ts3, cat, cut, cnt = _walks(G, B, M)
    t = torch.from_numpy(ts3.reshape(-1, 3))
    tf = er.time_encode(sd, (t[:, 2:3] - t).reshape(1, -1)).reshape(-1, 3, sd["time_encoder.phase"].numel())
    ev = torch.cat([ef[torch.from_numpy(eid3.reshape(-1, 3)).long()], torch.from_numpy(cnt.reshape(-1, 3, 3)), tf], -1)
    lev = torch.nn.functional.linear(ev, sd["event_conv.lin_event.weight"], sd["event_conv.lin_event.bias"])
    return float(lev.min()), float(lev.max()), float(lev.abs().median())


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("cfg,table", [("de32", True), ("de172", True), ("de172", False), ("de1", False)])
def test_split_form_vs_oracle(cfg, table, M):
    """8.75 units, the split form (last unit partial)."""
    G, B = SMALL
    _close(_launch(cfg, "plain", _walks(G, B, M), table, M), _oracle(cfg, "plain", G, B, M))


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("variant", ["plain", "neg", "big", "tiny"])
def test_persistent_form_vs_oracle_and_split_form(variant, M):
    """514 units in one call (the persistent zero-node instance), equal bit for bit to the same rows as three
    split-form calls in every weight set, and against the oracle at the contract with the plain weights.  The
    other weight sets meet the oracle in test_lin_event_extremes_vs_oracle; here their distance to it is printed,
    not asserted: over these 8220 x M walks the fp32 oracle is no contract-grade reference for the "big" set (its
    sigmoid inputs are sums of terms ~1e3), the fp32-MFMA parent build of the library is 2.97 (M = 1) and 13.6
    (M = 3) contract bounds away from it there."""
    G, B = BIG
    w = _walks(G, B, M)
    assert (G * B * N + 15) // 16 == 514 and (B * N + 15) // 16 * M <= 3 * 512
    imp = _launch("de32", variant, w, True, M)
    ref = _oracle("de32", variant, G, B, M)
    if variant == "plain":
        _close(imp, ref)
    else:
        d = np.abs(imp - ref)
        print("%s M=%d: max |diff| %.3g, worst diff / bound %.3g" % (variant, M, d.max(), (d / (ATOL + RTOL * np.abs(ref))).max()))
    parts = np.concatenate([_launch("de32", variant, w, True, M, groups=slice(g, g + 1)) for g in range(G)])
    assert np.array_equal(parts.view(np.uint32), imp.view(np.uint32))


def test_variants_reach_what_they_are_for():
    """The weight sets give lin_event the outputs they are meant to (CPU): all negative; up to ~1e4; ~1e-6."""
    G, B = SMALL
    lo, hi, med = _lin_event_range("de32", "plain", G, B, 3)
    print("plain: lin_event in [%.3g, %.3g], median |L| %.3g" % (lo, hi, med))
    assert lo < 0 < hi
    lo, hi, med = _lin_event_range("de32", "neg", G, B, 3)
    print("neg: lin_event in [%.3g, %.3g]" % (lo, hi))
    assert hi < 0
    lo, hi, med = _lin_event_range("de32", "big", G, B, 3)
    print("big: lin_event in [%.3g, %.3g], median |L| %.3g" % (lo, hi, med))
    assert 3e3 <= max(-lo, hi) <= 3e4
    lo, hi, med = _lin_event_range("de32", "tiny", G, B, 3)
    print("tiny: lin_event in [%.3g, %.3g], median |L| %.3g" % (lo, hi, med))
    assert max(-lo, hi) <= 3e-6 and 1e-8 <= med


@pytest.mark.parametrize("cfg,table", [("de32", True), ("de172", True), ("de172", False)])
@pytest.mark.parametrize("variant", ["neg", "big", "tiny"])
def test_lin_event_extremes_vs_oracle(cfg, table, variant):
    """Split form, M = 3: all-zero activations, large and tiny lin_event outputs, in the zero-node instance and
    (dn = 172 with node features: the last tile's four padded rows) the two-branch ones."""
    G, B = SMALL
    _close(_launch(cfg, variant, _walks(G, B, 3), table, 3), _oracle(cfg, variant, G, B, 3))


def budget_case():
    return "de32", "plain", SMALL, 3


def test_error_budget():
    """The bf16-split first layer is no worse than the fp32 one against the float64 oracle: at most twice the
    parent build's measured maximum error on this input (the factor covers the summation order inside one bf16
    MFMA, which a CPU model of the split does not know)."""
    cfg, variant, (G, B), M = budget_case()
    imp = _launch(cfg, variant, _walks(G, B, M), True, M).astype(np.float64)
    err = np.abs(imp - _oracle(cfg, variant, G, B, M, True).astype(np.float64)).max()
    print("max |imp - float64 oracle| = %.4g (fp32-MFMA parent: %s)" % (err, PARENT_MAX_ERR64))
    assert err <= 2 * PARENT_MAX_ERR64
