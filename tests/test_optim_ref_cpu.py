"""tests/optim_ref.py against torch's own tools: with exact coefficients (c = 1 - b
in float64) six of its steps equal clip_grad_norm_ + torch.optim.AdamW run in
float64 on the CPU, to 1e-12 relative on p, m and v.  Clipping active (a
threshold well below every norm), inactive (above every norm) and absent,
weight decay zero and not.  No GPU, no engine."""
import numpy as np
import pytest
import torch

import optim_ref as R

STEPS = 6
SHAPES = ((7, 5), (5,), (3, 4, 2))


def _data(seed=0):
    g = np.random.default_rng(seed)
    ps = [g.standard_normal(s) for s in SHAPES]
    gs = [[g.standard_normal(s) * 10.0 ** (k % 3 - 1) for s in SHAPES] for k in range(STEPS)]
    return ps, gs


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("max_norm", [None, 1e6, 0.05], ids=["absent", "inactive", "active"])
def test_ref_equals_clip_grad_norm_and_adamw(max_norm, wd):
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    ps, gs = _data()
    params = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in ps]
    opt = torch.optim.AdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p = np.concatenate([a.ravel() for a in ps])
    m, v, t = np.zeros_like(p), np.zeros_like(p), 0
    coefs = []
    for k in range(STEPS):
        for q, g in zip(params, gs[k]):
            q.grad = torch.tensor(g, dtype=torch.float64)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        p, m, v, t, stats = R.step(p, m, v, np.concatenate([g.ravel() for g in gs[k]]), t, b1=b1, b2=b2, c1=1 - b1,
                                   c2=1 - b2, lr=lr, wd=wd, eps=eps,
                                   max_norm=float("inf") if max_norm is None else max_norm)
        coefs.append(stats[1])
        want = {"p": torch.cat([q.detach().reshape(-1) for q in params]),
                "m": torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in params]),
                "v": torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params])}
        for name, got in (("p", p), ("m", m), ("v", v)):
            err = (got - want[name]).abs().max().item()
            assert err <= 1e-12 * want[name].abs().max().item(), (name, k, err)
    assert t == STEPS
    if max_norm == 0.05:
        assert all(c < 0.5 for c in coefs)  # clipping was active at every step
    else:
        assert all(c == 1.0 for c in coefs)


def test_ref_skips_a_nonfinite_step_and_only_with_the_option():
    p, m, v = np.ones(4), np.full(4, 0.5), np.full(4, 0.25)
    kw = R.kernel_coefficients(1e-3, weight_decay=0.1, max_norm=1.0)
    for bad in (np.inf, -np.inf, np.nan):
        g = np.array([0.1, bad, 0.2, 0.3])
        p2, m2, v2, t2, stats = R.step(p, m, v, g, 3, skip_nonfinite=True, **kw)
        assert t2 == 3 and stats[2] == 1 and stats[1] == 0.0 and not np.isfinite(stats[0])
        for a, b in ((p2, p), (m2, m), (v2, v)):
            assert np.array_equal(a.numpy(), b)
        p3, _, _, t3, stats = R.step(p, m, v, g, 3, **kw)
        assert t3 == 4 and stats[2] == 0 and not torch.isfinite(p3).all()


def test_kernel_coefficients_are_float32_values():
    kw = R.kernel_coefficients(1e-3, (0.9, 0.999), 1e-8, 0.01, 0.5)
    for k, x in kw.items():
        assert float(np.float32(x)) == x, k
    assert kw["c1"] == float(np.float32(1) - np.float32(0.9))
    assert kw["c2"] == float(np.float32(1) - np.float32(0.999))
    assert R.kernel_coefficients(1e-3)["max_norm"] == float("inf")


def test_grad_norm_keeps_small_beside_large_and_does_not_overflow():
    n = 1 << 20
    g = np.full(n, 1e-4, dtype=np.float32)
    g[0] = 1e4
    exact = np.sqrt(float(np.float32(1e4)) ** 2 + (n - 1) * float(np.float32(1e-4)) ** 2)
    assert abs(R.grad_norm(g) - exact) <= 1e-12 * exact
    assert R.grad_norm(np.full(4, 1e30, dtype=np.float32)) == pytest.approx(2.0 * float(np.float32(1e30)), rel=1e-15)
