"""Training-data generation on the MI355X.

Replaces scripts/training/generate_data.py:12-54, which runs
BaselineSolver.run one IC at a time on the CPU, with ONE batched classical
rollout (hf_run, model=NULL) over every IC.  The output file has the
reference's keys, dtypes and ordering:

  state_t    [N*steps, 3, nx] f32   states 0..steps-1 of IC 0, then IC 1, ...
  flux_t     [N*steps, nx]    f32   F_n = n*u of each of those steps
  state_next [N*steps, 3, nx] f32   states 1..steps
  x          [nx]             f32   cell centres
  dt, dx, nu                        scalars (float64, as np.savez stores Python floats)

ICs are BaselineSolver.initial_condition(seed=ic) for ic = 0..N-1, exactly as
the reference seeds them (generate_data.py:24).

refine / substeps above 1 (both default 1: the path above, same launches, same
bits) generate the data from a FINE reference instead (fine_reference.py): the
classical solver on refine x the cells with substeps x smaller steps, box-
averaged onto the nx-cell grid every `substeps` fine steps.  Keys, shapes and
dtypes stay as above, on the coarse grid: flux_t is then the fine face flux at
the coarse faces averaged over the substeps (the flux a coarse finite-volume
step needs to be exact), dt, dx, x are the coarse grid's, and E follows
fine_E ("solve": the coarse grid's Poisson solve of the averaged density,
"filtered": the averaged fine E; at nx = 64 they differ by up to 1e-2 at refine
<= 4 and 5e-2 at refine = 16, fine_reference.py).  The ICs
are drawn ON THE FINE GRID with the same seeds, so the per-cell 0.05 randn
noise on u is fine-grid noise.

Limits: fine classical rollouts of these ICs do not stay finite for long.
CPU oracle, nu = 1e-3, dt = 5e-3, seeds 0-3, substeps = refine: nx*refine = 64
and 128 stay finite through 60 coarse steps; 256 first goes non-finite at
coarse step 50, 53, 36, 45 (one per seed), 512 at 52, 33, 26, 28 and 1024 at
41, 34, 25, 28; 256 with nu = 5e-3 stays finite through 60.  With
refine or substeps above 1 the generators therefore check the result once and
raise a ValueError naming the first IC and coarse step that is not finite
instead of writing NaNs into a dataset.
"""
import os

import numpy as np

from .baseline_solver import BaselineSolver
from .fine_reference import FineReference, first_nonfinite


def _fine_rollout(nx, seeds, steps, dt, nu, device, device_rng, refine, substeps, fine_E, flux):
    """FineReference.run_batch from fine ICs of `seeds`, checked once for non-finite rows."""
    ref = FineReference(nx=nx, refine=refine, substeps=substeps, dt=dt, nu=nu, device=device, E=fine_E)
    r = ref.run_batch(ref.initial_conditions(seeds, device_rng=device_rng), steps, traj=True, flux=flux)
    bad = first_nonfinite(r["traj"])
    if bad is not None:
        raise ValueError(f"the fine reference (nx = {nx} x refine = {refine}, substeps = {substeps}, nu = {nu}) is not "
                         f"finite at IC {bad[0]} (seed {seeds[bad[0]]}), coarse step {bad[1]}: fine classical "
                         "rollouts of these ICs blow up (datagen's docstring has the limits); use fewer steps, a "
                         "smaller refine or a larger nu")
    return r


def generate_dataset(nx=64, num_initial_conditions=20, steps_per_ic=30, dt=5e-3, t_end=1.0, nu=1e-3,
                     out_path="data/dataset.npz", device="cuda", seeds=None, device_rng=False, refine=1, substeps=1,
                     fine_E="solve"):
    """Returns (state_t, flux_t, state_next, x, dt, dx, nu) like the reference and
    writes them to `out_path` (skipped when out_path is None).  device_rng=True
    draws the ICs on the device too (BaselineSolver.initial_conditions).
    refine / substeps above 1: the data of the fine reference (module
    docstring; ValueError when it does not stay finite)."""
    solver = BaselineSolver(nx=nx, dt=dt, t_end=t_end, nu=nu, device=device)
    seeds = list(range(num_initial_conditions)) if seeds is None else list(seeds)
    if refine != 1 or substeps != 1:
        r = _fine_rollout(nx, seeds, steps_per_ic, dt, nu, device, device_rng, refine, substeps, fine_E, flux=True)
    else:
        ics = solver.initial_conditions(seeds, as_tensor=True, device_rng=device_rng)
        r = solver.run_batch(ics, steps_per_ic, traj=True, flux=True)
    traj = r["traj"].cpu().numpy()                     # [N, steps+1, 3, nx]
    N = traj.shape[0]
    state_t = traj[:, :-1].reshape(N * steps_per_ic, 3, nx)
    state_next = traj[:, 1:].reshape(N * steps_per_ic, 3, nx)
    flux_t = r["flux"].cpu().numpy().reshape(N * steps_per_ic, nx)
    x = solver.x.astype(np.float32)
    if out_path is not None:
        d = os.path.dirname(out_path)
        if d:
            os.makedirs(d, exist_ok=True)
        np.savez(out_path, state_t=state_t, flux_t=flux_t, state_next=state_next, x=x, dt=dt, dx=solver.dx, nu=nu)
    return state_t, flux_t, state_next, x, dt, solver.dx, nu


def generate_trajectories(nx=64, num_initial_conditions=20, steps_per_ic=30, dt=5e-3, t_end=1.0, nu=1e-3,
                          device="cuda", seeds=None, device_rng=False, refine=1, substeps=1, fine_E="solve"):
    """The classical trajectories themselves, [N, steps+1, 3, nx] float32 (numpy):
    the array generate_dataset computes and flattens into (state_t, state_next)
    pairs, kept whole for multi-step windows (training.WindowDataset).  Same
    ICs, same batched rollout; x, dx are BaselineSolver(nx=nx).x / .dx.
    device_rng=True draws the ICs on the device too.  refine / substeps above
    1: the fine reference's coarse trajectories (module docstring; ValueError
    when they do not stay finite)."""
    seeds = list(range(num_initial_conditions)) if seeds is None else list(seeds)
    if refine != 1 or substeps != 1:
        return _fine_rollout(nx, seeds, steps_per_ic, dt, nu, device, device_rng, refine, substeps, fine_E,
                             flux=False)["traj"].cpu().numpy()
    solver = BaselineSolver(nx=nx, dt=dt, t_end=t_end, nu=nu, device=device)
    ics = solver.initial_conditions(seeds, as_tensor=True, device_rng=device_rng)
    return solver.run_batch(ics, steps_per_ic, traj=True)["traj"].cpu().numpy()
