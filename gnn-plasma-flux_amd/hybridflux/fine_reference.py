"""The fine reference: the classical solver on `refine` x the cells with
`substeps` x smaller steps, coarse-grained onto the training grid as it runs.

The reference's README claims "Hybrid model matches fine-step baseline on
coarse grid" and "Can take larger time steps (2-5x) while maintaining
accuracy", but its data generator and its evaluation scripts run the classical
solver on the training grid at the training step (scripts/training/
generate_data.py:12-54, scripts/evaluation/evaluate_multi_ic.py:21-94), so
FluxGNN learns, and is scored against, the first-order upwind flux n*u of the
solver it is meant to beat.  FineReference produces the data and the score
behind those claims:

  states  the box average of the fine states over `refine` cells, every
          `substeps` fine steps;
  flux    the fine face flux at the coarse faces averaged over those substeps:
          the flux a coarse finite-volume step needs to be exact,
              nbar_j' = nbar_j - (dt/dx) (Fbar_j - Fbar_{j-1}),
          which holds to rounding (include/hybridflux.h, hf_coarsen_traj).

One launch per rollout where the fine grid has nx_f <= 64 or nx_f in {256, 512,
1024} (hf_run_coarse: the fine states never leave registers); any other nx_f
is sequenced in chunks, same bits.

E of the coarse states, the `E` option:
  "solve"     (default) E = engine.poisson(coarse grid, nbar): what the hybrid
              step itself computes from nbar, so the coarse states are
              self-consistent inputs and targets for it.  One strided
              hf_poisson_ex call over all B (T+1) rows.
  "filtered"  the box average of the fine E.
The two differ at nx = 64 (CPU oracle, seeds 0-3, 10 coarse steps, substeps =
refine, max |E| = 0.78) by at most 9.3e-3 at refine = 2, 9.6e-3 at 4 and 4.8e-2
at 16: the fine E carries the modes above the coarse Nyquist, which alias into
the box average, and the box filter's own transfer function.  With refine = 1
the fine grid is the coarse grid and E is already its solve: nothing is
recomputed.

Stability (CPU oracle, the reference's ICs, nu = 1e-3, dt = 5e-3, substeps =
refine, seeds 0-3): nx_f = 64 and 128 stay finite through 60 coarse steps;
nx_f = 256 first goes non-finite at coarse step 50, 53, 36, 45 (one per seed),
nx_f = 512 at 52, 33, 26, 28 and nx_f = 1024 at 41, 34, 25, 28; nx_f = 256 with
nu = 5e-3 stays finite through 60.
"""
import contextlib
import io
import math

import torch

from . import engine
from .baseline_solver import BaselineSolver


def first_nonfinite(traj):
    """(ic, step) of the first non-finite row of a trajectory [B,T1,3,nx] (the
    smallest step, then the smallest IC at it), or None.  One reduction and
    one host copy."""
    bad = ~torch.isfinite(traj).all(dim=3).all(dim=2)  # [B,T1]
    if not bool(bad.any()):
        return None
    step = int(bad.any(dim=0).to(torch.int8).argmax())
    ic = int(bad[:, step].to(torch.int8).argmax())
    return ic, step


class FineReference:
    def __init__(self, nx=64, refine=1, substeps=1, length=2 * math.pi, dt=5e-3, nu=1e-3, device="cuda",
                 poisson="spectral", E="solve"):
        refine, substeps = int(refine), int(substeps)
        if refine < 1 or refine > 64 or refine & (refine - 1):
            raise ValueError(f"refine must be a power of two in 1..64, got {refine}")
        if substeps < 1:
            raise ValueError(f"substeps must be >= 1, got {substeps}")
        if E not in ("solve", "filtered"):
            raise ValueError(f"E must be 'solve' or 'filtered', got {E!r}")
        self.nx, self.refine, self.substeps, self.E = int(nx), refine, substeps, E
        self.length, self.dt, self.nu = length, dt, nu
        self.coarse = BaselineSolver(nx=self.nx, length=length, dt=dt, nu=nu, device=device, poisson=poisson)
        with contextlib.redirect_stdout(io.StringIO()):  # the fine grid's dt/dx warning is not the caller's concern
            self.fine = BaselineSolver(nx=self.nx * refine, length=length, dt=dt / substeps, nu=nu, device=device,
                                       poisson=poisson)
        self.device = self.coarse.device

    @property
    def identity(self):
        """refine = substeps = 1: the fine reference IS the classical solver of the training grid."""
        return self.refine == 1 and self.substeps == 1

    def initial_conditions(self, seeds, device_rng=False):
        """Fine ICs [B,3,nx*refine] (device tensor): BaselineSolver.initial_conditions
        of the fine grid with the same seeds, so the per-cell 0.05 randn noise
        on u is fine-grid noise."""
        return self.fine.initial_conditions(seeds, as_tensor=True, device_rng=device_rng)

    def _solve_E(self, traj):
        if self.E == "solve" and self.refine > 1:
            engine.poisson_traj(self.coarse.grid, traj)
        return traj

    def restrict(self, states_fine):
        """Fine states [B,3,nx*refine] -> coarse states [B,3,nx] (box average; E per the E option)."""
        s = self.fine._upload(states_fine)
        if self.refine == 1:
            return s
        tc, _ = engine.coarsen_traj(s[:, None].contiguous(), None, self.refine, 1)
        return self._solve_E(tc)[:, 0]

    def run_batch(self, fine_states0, n_steps, traj=True, flux=False, final=False):
        """n_steps COARSE steps from fine states -> dict(traj [B,T+1,3,nx] | None,
        flux [B,T,nx] | None, final_fine [B,3,nx*refine] | None)."""
        s0 = self.fine._upload(fine_states0)
        if self.identity:  # the classical rollout itself: hf_run's launches and bits
            r = self.coarse.run_batch(s0, n_steps, traj=traj, flux=flux)
            return {"traj": r["traj"], "flux": r["flux"], "final_fine": r["final"] if final else None}
        r = engine.run_coarse(self.fine.grid, s0, n_steps, self.refine, self.substeps, traj=traj, flux=flux, final=final)
        if r["traj"] is not None:
            self._solve_E(r["traj"])
        return r
