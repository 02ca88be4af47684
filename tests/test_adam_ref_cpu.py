"""tests/adam_ref.py (the fp64 yardstick of the FusedAdam kernel tests) against torch.optim.Adam on fp64 CPU tensors:
six steps, with and without weight decay, with and without a gradient scale (torch is fed ``g * grad_scale``)."""
import numpy as np
import pytest
import torch

from adam_ref import adam_ref, f32

LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_ref_equals_torch_adam_fp64(wd, grad_scale):
    rng = np.random.default_rng(11)
    n = 257
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n) for _ in range(6)]
    # torch gets the hyper-parameters the C ABI would (fp32-rounded), as adam_ref rounds its own
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=f32(LR), betas=(f32(B1), f32(B2)), eps=f32(EPS), weight_decay=f32(wd),
                           foreach=False)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads):
        tp.grad = torch.from_numpy(g * f32(grad_scale))
        opt.step()
        p, m, v = adam_ref(p, g, m, v, t, LR, B1, B2, EPS, wd, grad_scale)
        st = opt.state[tp]
        for name, got, want in (("p", p, tp.detach().numpy()), ("m", m, st["exp_avg"].numpy()),
                                ("v", v, st["exp_avg_sq"].numpy())):
            err = np.abs(got - want).max() / np.abs(want).max()
            assert err <= 1e-12, (t, name, err)
    assert float(opt.state[tp]["step"]) == 6.0


def test_adam_ref_leaves_its_inputs_alone():
    a = [np.full(3, x) for x in (1.0, 2.0, 3.0, 4.0)]
    b = [x.copy() for x in a]
    adam_ref(*a, 0, LR, B1, B2, EPS, 1e-2, 0.5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
