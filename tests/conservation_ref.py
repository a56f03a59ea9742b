"""Plain torch restatement of the three K-step losses with the energy and charge
terms (include/hybridflux.h, hf_unroll_update_ex / hf_pure_unroll_update_ex /
hf_pinn_unroll_loss_ex and their adjoints), shared by
test_conservation_ref_cpu.py and test_gpu_conservation.py.  Not a test.

    L = (1/K) sum_{k=1..K} [ base_k + mean_b ( lam_e (e(s^_k)_b - eref_kb)^2
                                              + lam_q (q(s^_k)_b - qref_kb)^2 ) ]
    e(s)_b = 0.5 (sum_i u_i^2 + sum_i E_i^2) / nx,   q(s)_b = (sum_i n_i) / nx

base_k is the channel-weighted state MSE of step k (FluxGNN, PureGNN) or PINN's
term with its residuals (pinn_unroll_ref.step_terms); s^_k comes from a `step`
closure, one per model: flux_step (the hybrid solver step around FluxGNN),
pure_step (PureGNN's residual rollout), pinn_step (PINN's).  Everything runs in
the dtype of the inputs; gradients come from autograd."""
import numpy as np
import torch

import pinn_unroll_ref as R
from oracle import hybrid_oracle as O


def moments(s):
    """(e [..], q [..]) of states [..., 3, nx]: the oracle's energy and charge metrics."""
    nx = s.shape[-1]
    return 0.5 * ((s[..., 1, :] ** 2).sum(-1) + (s[..., 2, :] ** 2).sum(-1)) / nx, s[..., 0, :].sum(-1) / nx


def moments_np(s):
    """moments in numpy float64, [..., 2]."""
    e, q = moments(torch.as_tensor(np.asarray(s), dtype=torch.float64))
    return torch.stack([e, q], dim=-1).numpy()


def cons_terms(s, ref, lam, K):
    """(energy, charge) values of one step: s [B,3,nx], ref [B,2], each with its lam and the 1/(K B) of L."""
    e, q = moments(s)
    B = s.shape[0]
    return lam[0] * ((e - ref[:, 0]) ** 2).sum() / (K * B), lam[1] * ((q - ref[:, 1]) ** 2).sum() / (K * B)


def cons_coef(s, ref, lam, K):
    """The header's (ce, cq) [B,2] of one step, float64."""
    s = torch.as_tensor(np.asarray(s), dtype=torch.float64)
    ref = torch.as_tensor(np.asarray(ref), dtype=torch.float64)
    e, q = moments(s)
    B, _, nx = s.shape
    return torch.stack([2 * lam[0] * (e - ref[:, 0]) / (K * B * nx), 2 * lam[1] * (q - ref[:, 1]) / (K * B * nx)], 1).numpy()


def seed_np(s, coef, hybrid=False):
    """What the adjoints add to the seed of s [B,3,nx]: (cq, ce u, ce E); hybrid: no cq."""
    s = np.asarray(s, np.float64)
    c = np.asarray(coef, np.float64)
    g = np.empty_like(s)
    g[:, 0] = 0.0 if hybrid else c[:, 1, None]
    g[:, 1] = c[:, 0, None] * s[:, 1]
    g[:, 2] = c[:, 0, None] * s[:, 2]
    return g


def state_mse(p, s, tgt, w, K):
    wt = torch.as_tensor(w, dtype=p.dtype)[None, :, None]
    v = (wt * (p - tgt) ** 2).mean() / K
    return v, v


def unrolled_loss(step, traj, w=(1.0, 1.0, 1.0), lam=(0.0, 0.0), ref=None, through=True, base=state_mse):
    """(L, states [K,B,3,nx] detached, rows [K, base's values + 2] detached) of the
    rollout s^_k = step(s^_{k-1}) from traj[:, 0] against traj[:, 1:] [B,K+1,3,nx];
    ref [B,K,2] = (eref, qref) per IC and step (None with lam = (0, 0)).  base(p, s,
    target, w, K) -> (the step's term, its components...); a row is (total, the
    components..., energy, charge)."""
    B, K1, _, nx = traj.shape
    K = K1 - 1
    s, L, states, rows = traj[:, 0], 0.0, [], []
    zero = torch.zeros((), dtype=traj.dtype)
    for k in range(1, K1):
        p = step(s)
        t = base(p, s, traj[:, k], w, K)
        en, ch = cons_terms(p, ref[:, k - 1], lam, K) if ref is not None else (zero, zero)
        tot = t[0] + en + ch
        L = L + tot
        states.append(p.detach())
        rows.append(torch.stack([v.detach() for v in (tot, *t[1:], en, ch)]))
        s = p if through else p.detach()
    return L, torch.stack(states), torch.stack(rows)


# ------------------------------------------------------------------ the three models
def poisson_t(n, k):
    """Differentiable spectral solve (src/baseline_solver.py:59-68) in n's dtype."""
    rh = torch.fft.fft(n - 1.0, dim=-1)
    keep = k != 0
    Eh = torch.zeros_like(rh)
    Eh[..., keep] = 1j * rh[..., keep] / k[keep]
    return torch.fft.ifft(Eh, dim=-1).real


def hybrid_step_t(st, fe, c, dt, k):
    """src/hybrid_solver.py:45-63 from the edge fluxes fe [B,2nx]."""
    nx = st.shape[-1]
    n, u, E = st[:, 0], st[:, 1], st[:, 2]
    F = 0.5 * (fe[:, :nx] + fe[:, nx:])
    n1 = n - c * (F - torch.roll(F, 1, -1))
    Fu = 0.5 * u * u
    u1 = u - c * (Fu - torch.roll(Fu, 1, -1)) + dt * E
    return torch.stack([n1, u1, poisson_t(n1, k)], dim=1)


def flux_step(p, G, B, dtype):
    """s -> the hybrid step of s with FluxGNN parameters p (c = f32(dt/dx), dt = f32(dt), the kernels' scalars)."""
    nx = G.nx
    c, dt = float(np.float32(G.dt / G.dx)), float(np.float32(G.dt))
    k = torch.as_tensor(G.k, dtype=dtype)
    x = torch.as_tensor(G.x.astype(np.float32), dtype=dtype)
    ei = O.chain_edges(nx, B)

    def step(st):
        nf = torch.stack([st[:, 0], st[:, 1], st[:, 2], x.expand(B, nx)], dim=-1).reshape(B * nx, 4)
        return hybrid_step_t(st, O.flux_gnn_forward(p, nf, ei).reshape(B, 2 * nx), c, dt, k)
    return step


def pure_step(p, G, B, dtype):
    """s -> s + PureGNN([n, u, E, x])^T (evaluate_multi_ic.py:53-64)."""
    nx = G.nx
    x = torch.as_tensor(G.x.astype(np.float32), dtype=dtype)
    ei = O.chain_edges(nx, B)

    def step(st):
        nf = torch.stack([st[:, 0], st[:, 1], st[:, 2], x.expand(B, nx)], dim=-1).reshape(B * nx, 4)
        return st + O.pure_gnn_forward(p, nf, ei).view(B, nx, 3).permute(0, 2, 1)
    return step


def pinn_step(p):
    """s -> s + net(s) (evaluate_multi_ic.py:70-83; oracle.pinn_forward)."""
    return lambda s: O.pinn_forward(p, s)


def pinn_base(lam_phys, dx, dt, nu, nx, dtype):
    """PINN's base term with the residuals: (total, data, cont, mom, pois) of pinn_unroll_ref.step_terms."""
    Pm = R.poisson_matrix(nx, nx * dx, dtype) if lam_phys is not None else None
    return lambda p, s, tgt, w, K: R.step_terms(p, s, tgt, w, lam_phys, dx, dt, nu, Pm, K)


def params(sd, dtype):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(True) for k, v in sd.items()}


def loss_and_grads(make_step, sd, traj, w, lam, ref, dtype, through=True, base=state_mse):
    """(loss, {name: grad float64}, states, rows) of one model in `dtype`: make_step(p) -> step."""
    p = params(sd, dtype)
    tr = torch.as_tensor(np.asarray(traj), dtype=dtype)
    rf = None if ref is None else torch.as_tensor(np.asarray(ref), dtype=dtype)
    L, states, rows = unrolled_loss(make_step(p), tr, w, lam, rf, through, base)
    L.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in p.items()}
    return float(L.detach()), grads, states.double().numpy(), rows.double().numpy()


def offset_ref(traj, rel=0.1):
    """A [B,K,2] float64 reference about `rel` away from the targets' own moments (below them
    for the even ICs, above for the odd ones), so that no residual is a small difference of
    large numbers."""
    m = moments_np(np.asarray(traj)[:, 1:])  # [B,K,2]
    sign = np.where(np.arange(m.shape[0]) % 2 == 0, -1.0, 1.0)[:, None, None]
    return m * (1.0 + rel * sign)
