"""Plain torch restatement of PINN's K-step loss (include/hybridflux.h,
hf_pinn_unroll_loss / hf_pinn_unroll_adjoint), shared by
test_pinn_unroll_ref_cpu.py and test_gpu_pinn_unrolled_training.py.  Not a test.

    L = (1/K) sum_{k=1..K} [ mean_{b,ch,i} w_ch (s^_k - s*_k)^2
          + l_c mean r_c^2 + l_m mean r_m^2 + l_p mean r_p^2 ]
    s^_0 = traj[:, 0],  s^_k = s^_{k-1} + net(s^_{k-1}),  s*_k = traj[:, k]

with the residuals at p = s^_k, (n, u, E) = s^_{k-1}, written with torch.roll
and a dense circulant P from hf_poisson_coeffs (a host helper), in whatever
dtype the inputs have; gradients come from autograd.  state_slot_grad_np is the
numpy restatement of the header's gather formulas for d term / d (n, u, E)."""
from ctypes import c_void_p

import numpy as np
import torch

REF_LAMBDA = (0.1, 0.1, 0.01)  # PINN_LOSS_WEIGHTS[1:], train_pinn.py:142-145


_COLUMNS = {}


def poisson_column(nx, length):
    """First column of the engine's spectral Poisson operator (hf_poisson_coeffs; the
    host forms it in O(nx^2), so each (nx, length) is asked for once).  A fresh copy."""
    from hybridflux._lib import check, lib
    key = (int(nx), float(length))
    if key not in _COLUMNS:
        pc = np.empty(lib().hf_poisson_plan_len(nx), dtype=np.float64)
        check(lib().hf_poisson_coeffs(nx, float(length), pc.ctypes.data_as(c_void_p)))
        _COLUMNS[key] = pc[:nx].copy()
    return _COLUMNS[key].copy()


_LAST_MATRIX = {}


def poisson_matrix(nx, length, dtype=torch.float64):
    """The dense circulant: (P f)[i] = sum_j col[(i - j) mod nx] f[j].  The last one
    built is kept (one entry: 6144^2 float64 values are 302 MB and seconds to index)
    and shared by the calls that follow for the same operator; callers leave it
    unchanged."""
    key = (int(nx), float(length), dtype)
    if key not in _LAST_MATRIX:
        i = torch.arange(nx)
        _LAST_MATRIX.clear()
        _LAST_MATRIX[key] = torch.as_tensor(poisson_column(nx, length), dtype=dtype)[(i[:, None] - i[None, :]) % nx]
    return _LAST_MATRIX[key]


def _up(f):
    return torch.roll(f, -1, -1)  # f[i+1]


def _dn(f):
    return torch.roll(f, 1, -1)   # f[i-1]


def residuals(p, s, dx, dt, nu, Pm):
    """(r_c, r_m, r_p) [B,nx] each, of prediction p and state slot s, both [B,3,nx]."""
    n, u, E = s[:, 0], s[:, 1], s[:, 2]
    pn, pu, pE = p[:, 0], p[:, 1], p[:, 2]
    r_c = (pn - n) / dt + (_up(n * u) - _dn(n * u)) / (2 * dx)
    r_m = (pu - u) / dt + u * (_up(u) - _dn(u)) / (2 * dx) + E - nu * (_up(u) - 2 * u + _dn(u)) / dx ** 2
    keep = torch.ones(p.shape[-1], dtype=p.dtype)
    keep[0] = 0.0
    X = -(pn @ Pm.T) * keep  # solve_poisson_torch (train_pinn.py:64-75): X[0] = 0
    return r_c, r_m, pE - X


def step_terms(p, s, tgt, w, lam, dx, dt, nu, Pm, K=1):
    """One step's (total, data, cont, mom, pois), each with its weight and the 1/K of L.
    lam None: the state loss alone (s is not used)."""
    wt = torch.as_tensor(w, dtype=p.dtype)[None, :, None]
    data = (wt * (p - tgt) ** 2).mean() / K
    zero = torch.zeros((), dtype=p.dtype)
    if lam is None:
        return data, data, zero, zero, zero
    r_c, r_m, r_p = residuals(p, s, dx, dt, nu, Pm)
    cont, mom, pois = lam[0] * (r_c ** 2).mean() / K, lam[1] * (r_m ** 2).mean() / K, lam[2] * (r_p ** 2).mean() / K
    return data + cont + mom + pois, data, cont, mom, pois


def unrolled_loss(net, traj, w=(1.0, 1.0, 1.0), lam=None, dx=None, dt=None, nu=None, through=True, length=None):
    """(L, states [K,B,3,nx] detached, terms [K,5] detached) for net: state [B,3,nx]
    -> state + net(state) (differentiable) and traj [B,K+1,3,nx] in the dtype to
    compute in.  through=False detaches the state between steps: both the
    network's input and the residuals' state slot."""
    B, K1, _, nx = traj.shape
    K = K1 - 1
    Pm = poisson_matrix(nx, nx * dx if length is None else length, traj.dtype) if lam is not None else None
    s, L, states, rows = traj[:, 0], 0.0, [], []
    for k in range(1, K1):
        p = net(s)
        t = step_terms(p, s, traj[:, k], w, lam, dx, dt, nu, Pm, K)
        L = L + t[0]
        states.append(p.detach())
        rows.append(torch.stack([v.detach() for v in t]))
        s = p if through else p.detach()
    return L, torch.stack(states), torch.stack(rows)


def state_mse_unrolled(states, traj, w):
    """The L that test_gpu_pure_unrolled_training.py restates, from given states [K,B,3,nx]."""
    K = states.shape[0]
    wt = torch.as_tensor(w, dtype=states.dtype)[None, :, None]
    L = 0.0
    for j in range(1, K + 1):
        L = L + (wt * (states[j - 1] - traj[:, j]) ** 2).mean() / K
    return L


def state_slot_grad_np(pnext, s, lam, phys_scale, dx, dt, nu, drop_jp1=False):
    """The header's gather formulas in numpy float64: d [phys_scale (l_c sum r_c^2 +
    l_m sum r_m^2)] / d (n, u, E) for the residuals at p' = pnext, (n, u, E) = s,
    both [B,3,nx].  drop_jp1: the mutant that loses the j+1 neighbour terms."""
    pnext, s = np.asarray(pnext, np.float64), np.asarray(s, np.float64)
    n, u, E = s[:, 0], s[:, 1], s[:, 2]
    up, dn = (lambda f: np.roll(f, -1, -1)), (lambda f: np.roll(f, 1, -1))
    r_c = (pnext[:, 0] - n) / dt + (up(n * u) - dn(n * u)) / (2 * dx)
    r_m = (pnext[:, 1] - u) / dt + u * (up(u) - dn(u)) / (2 * dx) + E - nu * (up(u) - 2 * u + dn(u)) / dx ** 2
    q_c, q_m = 2 * phys_scale * lam[0] * r_c, 2 * phys_scale * lam[1] * r_m
    k1 = 0.0 if drop_jp1 else 1.0
    dqc = dn(q_c) - k1 * up(q_c)
    g_n = -q_c / dt + u * dqc / (2 * dx)
    g_u = n * dqc / (2 * dx) + q_m * (-1 / dt + (up(u) - dn(u)) / (2 * dx) + 2 * nu / dx ** 2) \
        + dn(q_m) * (dn(u) / (2 * dx) - nu / dx ** 2) + k1 * up(q_m) * (-up(u) / (2 * dx) - nu / dx ** 2)
    return np.stack([g_n, g_u, q_m], axis=1)
