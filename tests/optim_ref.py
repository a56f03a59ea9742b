"""A float64 restatement of one guarded optimizer step (include/hybridflux.h,
hf_adam_flat_ex): clip by the global L2 norm, decoupled weight decay, Adam,
the skip of a step whose gradient norm is not finite.  Plain torch float64
expressions on whatever device the arrays are on; no engine.

The coefficient values are arguments: with the exact ones (c1 = 1 - b1, c2 = 1
- b2 in float64) it is clip_grad_norm_ + torch.optim.AdamW
(test_optim_ref_cpu.py); with the kernel's documented float32-valued ones
(kernel_coefficients) it is the kernel's mathematics, from which the kernel
differs by float32 rounding alone.
"""
import math

import numpy as np
import torch


def kernel_coefficients(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=float("inf")):
    """The values the kernel computes with, as Python floats: every by-value
    argument rounded to float32, c1 = float32(1) - float32(b1) and c2 likewise."""
    f = np.float32
    b1, b2 = f(betas[0]), f(betas[1])
    return dict(b1=float(b1), b2=float(b2), c1=float(f(1) - b1), c2=float(f(1) - b2), lr=float(f(lr)),
                wd=float(f(weight_decay)), eps=float(f(eps)), max_norm=float(f(max_norm)))


def _f64(a):
    return torch.as_tensor(a).to(torch.float64)


def grad_norm(g):
    """sqrt(sum g^2) with the squares and the sum in float64 (a Python float)."""
    g = _f64(g)
    return float(torch.sqrt(torch.sum(g * g)))


def step(p, m, v, g, t, *, b1, b2, c1, c2, lr, wd, eps, max_norm, skip_nonfinite=False):
    """Step t + 1 from the state (p, m, v) after t steps, on the gradient g.
    Returns (p, m, v, t, stats) as float64 tensors and stats = (norm, coef,
    skipped); a skipped step returns its inputs."""
    p, m, v, g = _f64(p), _f64(m), _f64(v), _f64(g)
    norm = grad_norm(g)
    if skip_nonfinite and not math.isfinite(norm):
        return p, m, v, t, (norm, 0.0, 1)
    c = max_norm / (norm + 1e-6) if not (math.isinf(max_norm) and math.isinf(norm)) else float("nan")
    coef = c if c < 1.0 else 1.0
    if coef != 1.0:
        g = g * coef
    if wd != 0.0:
        p = p * (1.0 - lr * wd)
    t = t + 1
    m = b1 * m + c1 * g
    v = b2 * v + c2 * g * g
    bc1 = 1.0 - b1 ** t
    bc2s = math.sqrt(1.0 - b2 ** t)
    p = p - (lr / bc1) * m / (torch.sqrt(v) / bc2s + eps)
    return p, m, v, t, (norm, coef, 0)
