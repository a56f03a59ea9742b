"""Batched, device-side counterparts of the reference's rollout scoring
(SURVEY.md 8f rank 1).  The reference scores one IC at a time on host numpy
trajectories; here B rollouts are scored on the MI355X from the metric
series the rollout kernels write (hf_traj_metrics / hf_traj_mse /
hf_rollout_summary), so a sharded multi-GPU job can gather them.

  compute_metrics(states_pred, states_true)   scripts/evaluation/evaluate_all.py:118-159
  multi_ic_mse(solver, states0, n_steps)      scripts/evaluation/evaluate_multi_ic.py:21-94
  long_rollout(solver, states0, n_steps)      scripts/evaluation/evaluate_long_rollout.py:18-81
  compare_models(models, states0, n_steps)    scripts/evaluation/evaluate_multi_ic.py:97-136
  compare_to_fine(solver, fine_ref, ...)      no counterpart: the score against a fine reference

`solver` is a HybridSolver, a HybridEnsemble (every result then carries a
leading model axis) or a ModelRollout, the adapter that gives the
comparison models (PureGNN, PINN: evaluate_multi_ic.py:45-83) the same
compare_batch / run_batch, scored inside their one-launch rollouts.
"""
import torch

from . import engine
from .baselines import PureGNN
from .hybrid_solver import HybridEnsemble, HybridSolver

SUMMARY_FIELDS = ("exploded_at", "actual_steps", "final_energy_drift", "final_charge_drift", "final_mse",
                  "mean_mse", "final_energy_drift_true", "final_charge_drift_true")


def summary_dict(summary):
    """[B, HF_NUM_SUMMARY] -> {field: [B] tensor} (or [M, B, .] -> [M, B], a model
    set's); exploded_at is -1 where nothing exploded."""
    return {k: summary[..., i] for i, k in enumerate(SUMMARY_FIELDS)}


def compute_metrics(states_pred, states_true):
    """evaluate_all.compute_metrics for B rollouts at once: states_* [B,T+1,3,nx]
    device tensors -> dict of device tensors with the reference's keys, each
    with a leading IC axis ([B,T+1] series, [B] scalars)."""
    mp = engine.traj_metrics(states_pred)
    mt = engine.traj_metrics(states_true)
    mse = engine.traj_mse(states_pred, states_true)
    summ, drift = engine.rollout_summary(mp, mse, mt, drift=True)
    return {
        "mse_n": mse[..., 0], "mse_u": mse[..., 1], "mse_E": mse[..., 2],
        "mse_total": (mse[..., 0] + mse[..., 1]) + mse[..., 2],
        "energy_drift_pred": drift[..., 0], "energy_drift_true": drift[..., 2],
        "charge_drift_pred": drift[..., 1], "charge_drift_true": drift[..., 3],
        "final_mse": summ[:, 4], "mean_mse": summ[:, 5],
        # evaluate_all.py:157-158 read index -1 (= T); the summary's fields 2, 3 stop
        # at the last finite step, which is T unless the rollout exploded
        "final_energy_drift": drift[:, -1, 0], "final_charge_drift": drift[:, -1, 1],
    }


class ModelRollout:
    """A PureGNN or PINN with the batched scoring API of HybridSolver:
    compare_batch and run_batch on the scored rollouts (PureGNN.rollout /
    PINN.rollout with metrics= / compare=), so multi_ic_mse, long_rollout,
    compare_models and rollout.gather_rollout take it unchanged.  `baseline` is
    the BaselineSolver whose grid gives the classical twin its dt, nu and
    Poisson mode; x (PureGNN's node coordinate) defaults to that grid's cell
    centres (evaluate_multi_ic.py:49)."""

    def __init__(self, model, baseline, x=None):
        self.model, self.baseline = model, baseline
        self.x = baseline.grid.x if x is None else x
        self._takes_x = isinstance(model, PureGNN)  # PureGNN.rollout(states0, n_steps, x, ...)

    @property
    def grid(self):
        return self.baseline.grid

    def _rollout(self, states0, n_steps, **kw):
        s0 = self.baseline._upload(states0)
        if self._takes_x:
            return self.model.rollout(s0, n_steps, self.x, **kw)
        return self.model.rollout(s0, n_steps, **kw)

    def compare_batch(self, states0, n_steps, metrics=True):
        """dict(final, mse [B,T+1,3], metrics, metrics_classical): HybridSolver.compare_batch's."""
        r = self._rollout(states0, n_steps, traj=False, metrics=metrics, compare=self.baseline)
        return {k: r[k] for k in ("final", "mse", "metrics", "metrics_classical")}

    def run_batch(self, states0, n_steps, traj=True, flux=False, metrics=False):
        """dict(final, traj, flux (always None), metrics): HybridSolver.run_batch's."""
        if flux:
            raise ValueError("ModelRollout.run_batch: these models predict the state change, not a face flux")
        r = self._rollout(states0, n_steps, traj=traj, metrics=metrics)
        return {"final": r["final"], "traj": r["traj"], "flux": None, "metrics": r.get("metrics")}


def ensemble_groups(models):
    """Which entries of `models` (name -> solver) compare_models rolls out
    together: lists of names, in `models`' order, of HybridSolvers that agree
    on HybridEnsemble.SIGNATURE (nx, grid constants, Poisson mode, precision,
    device, graph radius: a 12-model sweep over three radii is three launches).
    Groups of one, ModelRollouts and anything else are left out: they
    run on their own."""
    groups = {}
    for k, m in models.items():
        if isinstance(m, HybridSolver):
            groups.setdefault(HybridEnsemble.signature(m), []).append(k)
    return [g for g in groups.values() if len(g) > 1]


def compare_models(models, states0, n_steps, grouped=True):
    """evaluate_multi_ic.py:97-136 on the device: every model of `models` (name
    -> HybridSolver or ModelRollout) rolled out from the same ICs and scored
    against the classical solver.  Returns {name: {mean_mse, std_mse (python
    floats, np.mean / np.std over the ICs as :128-136), mse_per_ic (list)}};
    the one host synchronisation is the copy of all per-IC numbers at the end.
    grouped: the HybridSolvers that can share a launch (ensemble_groups) run as
    one HybridEnsemble each, everything else one by one; grouped=False runs
    every model on its own.  The numbers are the same, bit for bit."""
    names = list(models)
    if not names:
        return {}
    rows = {}
    for g in ensemble_groups(models) if grouped else []:
        per_model = multi_ic_mse(HybridEnsemble([models[k] for k in g]), states0, n_steps)[0]  # [len(g), B]
        rows.update(zip(g, per_model))
    for k in names:
        if k not in rows:
            rows[k] = multi_ic_mse(models[k], states0, n_steps)[0]
    per_ic = torch.stack([rows[k] for k in names])  # [M, B], device
    host = per_ic.to(torch.float64).cpu().numpy()
    return {k: {"mean_mse": float(host[i].mean()) if host.shape[1] else float("nan"),
                "std_mse": float(host[i].std()) if host.shape[1] else float("nan"),
                "mse_per_ic": [float(v) for v in host[i]]}
            for i, k in enumerate(names)}


def multi_ic_mse(solver, states0, n_steps):
    """evaluate_model_on_ic('hybrid', ...) for B ICs in one launch: the hybrid
    rollout and the classical BaselineSolver twin from the same states, scored
    per step.  Returns (mean MSE per IC [B] (the reference's return value),
    the compare_batch result, summary dict); with a HybridEnsemble every
    tensor has a leading model axis ([M,B] mean MSE)."""
    r = solver.compare_batch(states0, n_steps, metrics=True)
    summ, _ = engine.rollout_summary(r["metrics"], r["mse"], r["metrics_classical"])
    d = summary_dict(summ)
    return d["mean_mse"], r, d


def compare_to_fine(solver, fine_ref, fine_states0, n_steps):
    """A solver scored against the FINE reference instead of its same-dt/dx
    classical twin (the reference README's "matches fine-step baseline on
    coarse grid"): `solver` (anything with run_batch(states [B,3,nx], n_steps,
    traj=True): HybridSolver, ModelRollout, BaselineSolver) is rolled out from
    fine_ref.restrict(fine_states0), the FineReference from fine_states0, and
    the two coarse trajectories are scored with traj_mse / traj_metrics.
    Returns compare_batch's dict (final, mse [B,T+1,3], metrics,
    metrics_classical = the fine reference's), so summary_dict and everything
    downstream take it unchanged.  The solver's nx, length and dt must be the
    reference's coarse ones (ValueError); a HybridEnsemble is not supported."""
    if isinstance(solver, HybridEnsemble):
        raise ValueError("compare_to_fine: a HybridEnsemble is not supported; score its solvers one by one")
    g, c = solver.grid, fine_ref.coarse.grid
    for k in ("nx", "length", "dt"):
        if getattr(g, k) != getattr(c, k):
            raise ValueError(f"compare_to_fine: the solver's {k} = {getattr(g, k)} is not the fine reference's coarse "
                             f"{k} = {getattr(c, k)}")
    r = solver.run_batch(fine_ref.restrict(fine_states0), n_steps, traj=True)
    ref = fine_ref.run_batch(fine_states0, n_steps, traj=True)["traj"]
    return {"final": r["final"], "mse": engine.traj_mse(r["traj"], ref), "metrics": engine.traj_metrics(r["traj"]),
            "metrics_classical": engine.traj_metrics(ref)}


def long_rollout(solver, states0, n_steps, drift=True):
    """evaluate_long_rollout for B ICs: one rollout, explosion tracking and the
    energy drift series on the device.  Returns the summary dict plus
    'energy_drift_pred' [B,T+1] (valid up to actual_steps, as the reference
    stops recording there)."""
    r = solver.run_batch(states0, n_steps, traj=False, metrics=True)
    summ, dr = engine.rollout_summary(r["metrics"], drift=drift)
    d = summary_dict(summ)
    d["exploded"] = d["exploded_at"] >= 0
    if dr is not None:
        d["energy_drift_pred"] = dr[..., 0]
    d["metrics"] = r["metrics"]
    return d
