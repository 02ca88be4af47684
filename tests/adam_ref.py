"""fp64 restatement of one ``tm_adam_step`` call over a flat buffer (csrc/optim.hip; the formula quoted at its top is
torch/optim/adam.py ``_single_tensor_adam`` with amsgrad and maximize off):

    g = grad * grad_scale (+ weight_decay * p)
    m = lerp(m, g, 1 - beta1)            v = v * beta2 + (1 - beta2) * g * g
    p = p - step_size * m / (sqrt(v) / sqrt(bc2) + eps),  step_size = lr / bc1,  bc_i = 1 - beta_i^t,  t = t_before + 1

The hyper-parameters are rounded to fp32 first, as the C ABI receives them (``float lr, beta1, ...``); everything after
that is fp64.  tests/test_adam_ref_cpu.py holds it against torch.optim.Adam on fp64 CPU tensors."""
import numpy as np


def f32(x):
    """The fp32 value the C ABI receives for a Python float, as fp64."""
    return float(np.float32(x))


def adam_ref(p, g, m, v, t_before, lr, beta1, beta2, eps, weight_decay, grad_scale):
    """One step over flat fp64 arrays; returns the new (p, m, v), the inputs untouched."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    lr, beta1, beta2, eps, weight_decay, grad_scale = (f32(x) for x in (lr, beta1, beta2, eps, weight_decay,
                                                                        grad_scale))
    t = float(t_before) + 1.0
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    g = g * grad_scale
    if weight_decay != 0.0:
        g = g + weight_decay * p
    m = m + (1.0 - beta1) * (g - m)
    v = v * beta2 + (1.0 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v
