"""Base TGAT without a GPU: parameter layout, seeded initialisation and refused options of
tempme_amd.tgat.TGAT against what the reference produced (tests/golden/tgat_uslegis.npz), and the
reference's own fp32-vs-fp64 distances that the GPU tests' tolerances are derived from."""
import numpy as np
import pytest
import torch

import tgat_inputs as TA
import tgn_inputs as TI


@pytest.mark.parametrize("case", TA.CASES)
def test_state_dict_keys_and_shapes(case):
    g = TA.golden()
    sd = TA.build_model(case, perturb=False).state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f"{case}_sd_names"]]
    assert [",".join(str(int(x)) for x in v.shape) for v in sd.values()] == [str(s) for s in g[f"{case}_sd_shapes"]]


@pytest.mark.parametrize("case", TA.CASES)
def test_seeded_init_reproduces_reference(case):
    """torch.manual_seed(s); TGAT(...) draws the reference's weights: per tensor (sum, sum |x|, sum x^2) in
    fp64 equal the reference's (the same values in the same order, so equal to summation rounding)."""
    g = TA.golden()
    sd = TA.build_model(case, perturb=False).state_dict()
    got = np.array([[v.double().sum().item(), v.double().abs().sum().item(), (v.double() ** 2).sum().item()]
                    for v in sd.values()])
    np.testing.assert_allclose(got, g[f"{case}_sd_stats"], rtol=1e-12, atol=1e-12)


def test_unsupported_options_raise():
    from tempme_amd.tgat import TGAT
    nf, ef = TI.feats("uslegis")
    ok = dict(num_layers=2, n_head=3)
    for bad in (dict(attn_mode="map"), dict(use_time="pos"), dict(use_time="empty"), dict(attn_agg_method="lstm"),
                dict(attn_agg_method="mean"), dict(num_layers=3), dict(num_layers=1), dict(n_head=5)):
        with pytest.raises(NotImplementedError):
            TGAT(nf, ef, 20, **{**ok, **bad})
    with pytest.raises(NotImplementedError):
        TGAT(nf, ef, 20)                               # the reference's default num_layers=3
    m = TGAT(nf, ef, 20, **ok)
    m.train()                                          # drop_out 0.1: the dropout path is not built
    d = TI.load_batch()
    with pytest.raises(NotImplementedError):
        TA.contrast(m, d)


def test_state_dict_round_trip():
    a, b = TA.build_model("synth"), TA.build_model("uslegis", perturb=False)
    c = TA.build_model("synth", perturb=False)
    c.load_state_dict(a.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), c.state_dict().values()))
    with pytest.raises(RuntimeError):
        b.load_state_dict(a.state_dict())              # other dims: shapes differ


@pytest.mark.parametrize("case", TA.CASES)
def test_reference_fp32_envelope(case, record_property):
    """The reference's own fp32 results against an fp64 evaluation of the same model, from the fixture:
    logits (the GPU parity tolerance is 10 x this, never below the TGN test's 2e-5) and the six
    explanation-weight gradients (the GPU gradient tolerance is 10 x the distance of the same hop).
    Measured when the fixture was made: logits 2.2e-6 (uslegis) / 1.5e-6 (synth); gradients hop-1
    1.1e-5 / 3.0e-7, hop-2 9.2e-7 / 7.9e-9."""
    g = TA.golden()
    env = float(np.abs(g[f"{case}_ori"].astype(np.float64) - g[f"{case}_ori64"]).max())
    record_property("logit_envelope", env)
    assert 0 < env < 5e-6
    assert TA.logit_atol(g, case) == 10 * max(env, 2e-6)
    for h in (0, 1):
        dist = max(float(np.abs(g[f"{case}_grad32_{s}{h}"] - g[f"{case}_grad64_{s}{h}"]).max()) for s in TA.SIDES)
        scale = max(float(np.abs(g[f"{case}_grad64_{s}{h}"]).max()) for s in TA.SIDES)
        record_property(f"grad_hop{h + 1}_distance", dist)
        print(case, "hop", h + 1, "gradient distance", dist, "scale", scale)
        assert 0 < dist < 1e-4 * scale
