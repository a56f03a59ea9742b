"""The restatement of PINN's K-step loss that the GPU tests measure against
(tests/pinn_unroll_ref.py), checked without a GPU: against the reference
trainer's own values at K = 1, its gather formulas against float64 autograd, its
state loss against the one PureGNN's unrolled tests restate, and that the
comparison would catch a lost neighbour term."""
import math

import numpy as np
import pytest
import torch

import pinn_unroll_ref as R
from conftest import close, golden

DT, NU = 5e-3, 1e-3


def test_k1_reproduces_the_reference_trainer():
    """K = 1, w = (1,1,1), l = (0.1, 0.1, 0.01) on the fixture's first prediction: the
    reference's own loss values (rtol 1e-5) and dL/dpred (2e-5 max|ref| + 1e-9), the
    gates of test_gpu_pinn_training.py for these arrays."""
    from test_gpu_pinn_training import fixture_batch, grad_close
    fx = golden("pinn_train.npz")
    dx, dt, nu = float(fx["dx"]), float(fx["dt"]), float(fx["nu"])
    st, sn = (t.double() for t in fixture_batch(fx, 0))
    pred = torch.from_numpy(fx["first_pred"]).double().requires_grad_(True)
    w = [float(v) for v in fx["weights"]]
    assert tuple(w) == (1.0,) + R.REF_LAMBDA
    t = R.step_terms(pred, st, sn, (w[0],) * 3, w[1:], dx, dt, nu, R.poisson_matrix(32, 32 * dx), K=1)
    t[0].backward()
    got = np.array([float(v.detach()) for v in t])
    want = np.asarray(fx["first_losses"], np.float64) * np.array([1.0] + w)  # the fixture's terms are unweighted
    close(got, want, 0.0, 1e-5, what="losses")
    grad_close(pred.grad, fx["first_grad_pred"], "grad_pred")


def slot_case(nx, B=2, seed=7):
    g = torch.Generator().manual_seed(seed + nx)
    s = torch.stack([1 + 0.1 * torch.randn(B, nx, generator=g, dtype=torch.float64),
                     0.1 * torch.randn(B, nx, generator=g, dtype=torch.float64),
                     0.1 * torch.randn(B, nx, generator=g, dtype=torch.float64)], dim=1)
    pnext = s + 0.02 * torch.randn(B, 3, nx, generator=g, dtype=torch.float64)
    return pnext, s


def slot_autograd(pnext, s, lam, phys_scale, dx):
    """float64 autograd of phys_scale (l_c sum r_c^2 + l_m sum r_m^2 + l_p sum r_p^2) in the state slot."""
    nx = s.shape[-1]
    s = s.clone().requires_grad_(True)
    r_c, r_m, r_p = R.residuals(pnext, s, dx, DT, NU, R.poisson_matrix(nx, nx * dx))
    (phys_scale * (lam[0] * (r_c ** 2).sum() + lam[1] * (r_m ** 2).sum() + lam[2] * (r_p ** 2).sum())).backward()
    return s.grad.numpy()


@pytest.mark.parametrize("nx", [1, 2, 3, 5, 16])
def test_gather_formulas_equal_autograd(nx):
    """d term / d (n, u, E) by the header's gather formulas against float64 autograd of
    the restatement, to 1e-12 relative; r_p adds nothing (it does not depend on the
    state slot).  nx = 1, 2: the neighbour indices coincide and stay separate terms."""
    pnext, s = slot_case(nx)
    dx, lam, ps = 2 * math.pi / nx, (0.3, 0.7, 0.05), 1.0 / (3 * 2 * nx)
    want = slot_autograd(pnext, s, lam, ps, dx)
    got = R.state_slot_grad_np(pnext.numpy(), s.numpy(), lam, ps, dx, DT, NU)
    assert np.abs(want).max() > 0
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("nx", [2, 5])
def test_lost_neighbour_term_is_detected(nx):
    """The mutant without the j+1 neighbour terms misses the same comparison by orders of magnitude."""
    pnext, s = slot_case(nx)
    dx, lam, ps = 2 * math.pi / nx, (0.3, 0.7, 0.05), 1.0 / (3 * 2 * nx)
    want = slot_autograd(pnext, s, lam, ps, dx)
    bad = R.state_slot_grad_np(pnext.numpy(), s.numpy(), lam, ps, dx, DT, NU, drop_jp1=True)
    assert np.abs(bad - want).max() > 1e-6 * np.abs(want).max()


@pytest.mark.parametrize("lam", [None, (0.0, 0.0, 0.0)])
def test_zero_lambda_is_the_shared_state_loss(lam):
    """With l = 0 (or no residual terms) L is the state loss that
    test_gpu_pure_unrolled_training.py restates, on the same states."""
    torch.manual_seed(3)
    B, K, nx = 3, 3, 8
    W = 0.1 * torch.randn(3 * nx, 3 * nx, dtype=torch.float64)
    net = lambda s: s + torch.tanh(s.reshape(B, -1) @ W).reshape(s.shape)  # noqa: E731
    traj = torch.randn(B, K + 1, 3, nx, dtype=torch.float64)
    w = (0.5, 2.0, 1.0)
    L, states, terms = R.unrolled_loss(net, traj, w, lam, 2 * math.pi / nx, DT, NU)
    want = R.state_mse_unrolled(states, traj, w)
    assert abs(float(L) - float(want)) <= 1e-15 * abs(float(want))
    assert torch.equal(terms[:, 0], terms[:, 1]) and not terms[:, 2:].any()
    assert abs(float(terms[:, 0].sum()) - float(L)) <= 1e-15 * abs(float(L))


def test_pushforward_cuts_the_state_slot():
    """through=False: step 2's residuals send nothing into step 1's network call, so the
    gradient is the sum of the K one-step gradients on the detached states."""
    torch.manual_seed(4)
    B, K, nx = 2, 2, 5
    dx = 2 * math.pi / nx
    W = (0.1 * torch.randn(3 * nx, 3 * nx, dtype=torch.float64)).requires_grad_(True)
    net = lambda s: s + torch.tanh(s.reshape(B, -1) @ W).reshape(s.shape)  # noqa: E731
    traj = torch.randn(B, K + 1, 3, nx, dtype=torch.float64)
    L, states, _ = R.unrolled_loss(net, traj, lam=R.REF_LAMBDA, dx=dx, dt=DT, nu=NU, through=False)
    (g,) = torch.autograd.grad(L, W)
    Pm = R.poisson_matrix(nx, nx * dx)
    want = torch.zeros_like(W)
    for k in range(K):
        s = traj[:, 0] if k == 0 else states[k - 1]
        t = R.step_terms(net(s), s, traj[:, k + 1], (1.0, 1.0, 1.0), R.REF_LAMBDA, dx, DT, NU, Pm, K)
        want = want + torch.autograd.grad(t[0], W)[0]
    assert (g - want).abs().max() <= 1e-13 * want.abs().max()
