"""Shared inputs of the nonzero-phase tests (test_time_phase_cpu.py, test_gpu_time_phase.py and the
phase_sigma legs of the training tests): a seeded perturbation of TimeEncode's phase, the way to write it
into an explainer so that the weight pack follows, the oracle on the committed Enron walks, and a model of
a contracted time argument (one rounding of t * w + phase instead of the reference's two).

Why: the constructor leaves phase at zero and every golden was made from it, and with phase == 0 a fused
multiply-add of (t, w, 0) IS the rounded product, so a kernel that contracts the argument, reads phase at a
wrong index, or keeps a stale pack after phase changed passes every zero-phase test."""
import contextlib

import numpy as np
import torch

import enron_inputs as EI
from oracle import encoder_ref as er

RTOL, ATOL = 1e-5, 1e-6
SIGMA = 0.5
N_DEG, N_EVENTS = 20, 32          # the first 32 events of the N = 20 Enron goldens


def perturbed_phase(d, sigma=SIGMA, seed=5):
    return np.random.RandomState(seed).normal(0, sigma, d).astype(np.float32)


def set_phase(ex, ph):
    """Write ``ph`` into the explainer's TimeEncode phase in place, under no_grad, which bumps the
    parameter's ``_version``.  NOT ``phase.data.copy_``: a write through ``.data`` leaves ``_version``
    unchanged, and packed_weights() keys on (data_ptr, _version), so after a first call the kernels would
    go on reading the stale pack."""
    p = ex.time_encoder.phase
    with torch.no_grad():
        p.copy_(torch.as_tensor(np.asarray(ph), dtype=p.dtype).to(p.device))


def with_phase(sd, ph):
    """A copy of the oracle's state dict carrying phase ``ph`` (in the dict's own dtype)."""
    out = dict(sd)
    old = sd["time_encoder.phase"]
    out["time_encoder.phase"] = torch.as_tensor(np.asarray(ph, dtype=np.float32)).to(old.dtype).reshape(old.shape)
    return out


def single_rounding(sd, t):
    """oracle.encoder_ref.time_encode with the argument rounded ONCE: product and sum in fp64 (the product
    of two fp32 values is exact there), one rounding to fp32 -- what a fused multiply-add computes.  Models
    the defect for the CPU conditions only; no GPU test compares against it."""
    w, ph = sd["time_encoder.basis_freq"], sd["time_encoder.phase"]
    m = t.float().double().unsqueeze(-1) * w.float().double() + ph.float().double()
    return torch.cos(m.float().to(w.dtype))


@contextlib.contextmanager
def oracle_time_encode(fn, module=er):
    """Run the oracle (or another restatement module with a ``time_encode(sd, t)``) with ``fn`` in its place."""
    old = module.time_encode
    module.time_encode = fn
    try:
        yield
    finally:
        module.time_encode = old


def enron_walks(z):
    return EI.walks(z, N_DEG, N_EVENTS)


def enron_reference(sd, g, d, variant="base", dtype=torch.float32):
    """The oracle on the golden walks ``d``: per side (imp [B, W, 1], hop-1 [B, N], hop-2 [B, N^2]) in
    ``dtype`` (fp32 forms the comparison target, fp64 measures the oracle's own error).  The time argument is
    formed in fp32 with two roundings in both."""
    kw = EI.VARIANTS[variant]
    sd = {k: v.to(dtype) for k, v in sd.items()}
    nf, ef = torch.from_numpy(g["n_feat"]), torch.from_numpy(g["e_feat"])
    out = {}
    for s in EI.SIDES:
        x = d[s]
        imp = er.forward(sd, nf, ef, x["node"], x["eid"], x["ts"], x["cat"], d["ts_cut"], x["cnt"],
                         temporal=kw.get("use_temporal_guidance", True))
        e0, e1 = er.edge_importance(sd, ef, imp, x["eid"], x["ts"], x["sub_node"], x["sub_eid"],
                                    dependency=kw.get("use_dependency_aware_sampling", True))
        out[s] = (imp.double().numpy(), e0.double().numpy(), e1.double().numpy())
    return out


ENHANCE_TSCALE = 2e6


def enhance_inputs(G, B, W, seed=3):
    """enhance_train_ref.seeded_inputs (the smallest shapes of test_gpu_enhance*.py) with its timestamps
    (integers below 60) scaled into the Enron range: walk times up to 1e8 and cut times up to 1.2e8, every
    one still exact in fp32.  At the original scale a single-rounding time argument moves the pooled
    encoder's outputs by 0.06 of their tolerance; at this one by hundreds of it (test_time_phase_cpu.py)."""
    import enhance_train_ref as TR
    d = TR.seeded_inputs(seed, G, B, W)
    d["ts"], d["cut"] = d["ts"] * ENHANCE_TSCALE, d["cut"] * ENHANCE_TSCALE
    assert np.array_equal(d["ts"].astype(np.float32), d["ts"]) and np.array_equal(d["cut"].astype(np.float32), d["cut"])
    return d


def enhance_sides(d, seed=17):
    """The three groups of ``d`` (G = 3) as enhance_predict_agg's (walks, edge_identify) per side, and seeded
    base embeddings [B, node_dim]."""
    rng = np.random.default_rng(seed)
    gats = [torch.from_numpy(rng.normal(0, 1, (d["B"], d["n_feat"].shape[1])).astype(np.float32)) for _ in range(3)]
    sides = [((d["node"][g], d["eid"][g], d["ts"][g], d["cat"][g]), d["cnt"][g]) for g in range(3)]
    return sides, gats


def enhance_explainer(d, device=torch.device("cpu")):
    """The seeded explainer of test_gpu_enhance_train.build on ``d``'s tables, with the perturbed phase."""
    import tempme_amd as tm
    from enhance_inputs import Base
    torch.manual_seed(7)
    ex = tm.TempME(Base(d["n_feat"], d["e_feat"]), "tgn", "uslegis_sampled", 40, 64, device=device,
                   null_model={k: 1.0 / 12 for k in range(1, 13)}).to(device)
    ex.set_node_degree(d["deg"])
    set_phase(ex, perturbed_phase(ex.time_encoder.phase.numel()))
    return ex


def tol(ref):
    return ATOL + RTOL * np.abs(ref)
