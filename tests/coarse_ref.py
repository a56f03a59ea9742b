"""A numpy restatement of the coarse-graining of a fine classical rollout
(include/hybridflux.h, hf_coarsen_traj / hf_run_coarse), and the case table
the CPU and GPU tests share.

Definition, for `r` fine cells per coarse cell and `S` fine steps per coarse
step (r a power of two):

  traj_c[b, t, ch, j] = f32(tree / r),  tree the ADJACENT PAIRWISE float64 sum
      of the r float32 cells r j .. r j + r - 1 of fine row S t: level 1 adds
      cells (2m, 2m+1), level 2 adds those sums pairwise, and so on;
  flux_c[b, t, j]     = f32(acc / S),   acc the float64 sum, in ascending
      substep order from 0.0, of the fine F at cell r j + r - 1 (the right face
      of coarse cell j) over fine steps S t .. S t + S - 1; a float64 division.

The fine trajectories come from oracle.hybrid_oracle.classical_run.
"""
import numpy as np

from oracle import hybrid_oracle as O

# (nx coarse, r, S): the CPU identity's cases; all stay finite for T_c <= 3, seeds 0-2
IDENTITY_CASES = [(16, 16, 4), (64, 16, 16), (64, 4, 4), (64, 1, 4), (4, 64, 3), (32, 2, 1)]
IDENTITY_TC = 3
IDENTITY_SEEDS = (0, 1, 2)


def tree_sum(x, r):
    """Adjacent pairwise float64 sum of each run of r cells of the last axis."""
    v = np.asarray(x).astype(np.float64)
    assert r >= 1 and r & (r - 1) == 0 and v.shape[-1] % r == 0
    m = r
    while m > 1:
        v = v[..., 0::2] + v[..., 1::2]
        m //= 2
    return v


def box_mean(x, r):
    """f32(tree / r) of float32 cells [..., nx_f] -> [..., nx_f / r]."""
    return (tree_sum(np.asarray(x, np.float32), r) / float(r)).astype(np.float32)


def coarsen(traj_f, flux_f, r, S):
    """traj_f [..., T_f+1, 3, nx_f], flux_f [..., T_f, nx_f] or None ->
    (traj_c [..., T_c+1, 3, nx_f/r], flux_c [..., T_c, nx_f/r] or None)."""
    traj_f = np.asarray(traj_f, np.float32)
    T_f = traj_f.shape[-3] - 1
    assert S >= 1 and T_f % S == 0
    traj_c = box_mean(traj_f[..., ::S, :, :], r)
    if flux_f is None:
        return traj_c, None
    F = np.asarray(flux_f, np.float32)[..., r - 1::r].astype(np.float64)  # the coarse cells' right faces
    T_c = T_f // S
    acc = np.zeros(F.shape[:-2] + (T_c, F.shape[-1]), dtype=np.float64)
    for s in range(S):  # ascending substep order
        acc = acc + F[..., s::S, :]
    return traj_c, (acc / float(S)).astype(np.float32)


def grids(nx, r, S, dt=5e-3, nu=1e-3, length=2 * np.pi, poisson="spectral"):
    """(coarse, fine) oracle grids: nx cells at dt, r nx cells at dt / S."""
    return (O.Grid(nx, length, dt, nu, poisson=poisson), O.Grid(nx * r, length, dt / S, nu, poisson=poisson))


def fine_ics(grid_f, seeds):
    return np.stack([O.initial_condition(grid_f, s) for s in seeds]) if len(seeds) else \
        np.zeros((0, 3, grid_f.nx), np.float32)


def fine_run(grid_f, ics_f, T_c, S):
    """The oracle's fine rollout: (traj_f [B, T_c S + 1, 3, nx_f], flux_f [B, T_c S, nx_f])."""
    if T_c == 0:
        return ics_f[:, None].astype(np.float32), np.zeros((ics_f.shape[0], 0, grid_f.nx), np.float32)
    return O.classical_run(grid_f, ics_f, T_c * S)


def fine_reference(nx, r, S, T_c, seeds, E="filtered", **kw):
    """The coarse-grained oracle rollout: dict(traj, flux, fine_traj, fine_flux,
    coarse, fine).  E = "solve" overwrites the E rows with the oracle's Poisson
    solve of the coarse density on the coarse grid."""
    gc, gf = grids(nx, r, S, **kw)
    ics = fine_ics(gf, list(seeds))
    tf, ff = fine_run(gf, ics, T_c, S)
    tc, fc = coarsen(tf, ff, r, S)
    if E == "solve":
        tc = tc.copy()
        tc[..., 2, :] = O.solve_poisson(gc, tc[..., 0, :])
    elif E != "filtered":
        raise ValueError(E)
    return {"traj": tc, "flux": fc, "fine_traj": tf, "fine_flux": ff, "coarse": gc, "fine": gf}


def continuity_bound(fine_traj, fine_flux, gf, S):
    """(3 S + 4) 2^-24 (max|n| + 2 c_f max|F|): per fine step the product's, the
    difference's and the update's roundings (3 S of them, each at most one
    float32 ulp of a term bounded by max|n| or c_f max|F|... 2 c_f max|F| for
    the difference), the final casts of n-bar (2) and of F-bar (2, scaled by c),
    and S f32(c_f) against f32(c) (within the same ulps)."""
    c_f = gf.dt / gf.dx
    return (3 * S + 4) * 2.0 ** -24 * (np.abs(fine_traj[..., 0, :]).max() + 2 * c_f * np.abs(fine_flux).max())


def continuity_residual(traj_c, flux_c, gc):
    """max |n-bar_{t+1} - (n-bar_t - f32(dt/dx) (F-bar_j - F-bar_{j-1}))| in float64."""
    c = float(np.float32(gc.dt / gc.dx))
    n = traj_c[..., 0, :].astype(np.float64)
    F = flux_c.astype(np.float64)
    pred = n[..., :-1, :] - c * (F - np.roll(F, 1, axis=-1))
    return np.abs(n[..., 1:, :] - pred).max()
