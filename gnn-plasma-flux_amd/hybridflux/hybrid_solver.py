"""HybridSolver with the reference's API (src/hybrid_solver.py:11-73).

One step = FluxGNN edge fluxes on the periodic chain -> F = (F_fwd + F_bwd)/2
-> continuity n' = n - dt/dx (F - F_left) -> Burgers u' (no viscosity) + dt E
-> spectral Poisson E'.  On the MI355X the whole step is ONE kernel per IC
wave (chain_rollout_kernel, chain_common.h), and `run` is ONE persistent
kernel for the whole rollout when nx is 16/32/48/64; other nx use the
windowed / super-window chain kernel + the FV/Poisson kernel per step
(fv_poisson.hip).  Nothing crosses PCIe inside a rollout.

`step`/`run` keep the reference's numpy [3,nx] shapes; `step_batch`/`run_batch`
take [B,3,nx] device tensors (batched independent ICs) and return device
tensors.  `radius` is a label: stored and unused, exactly as in the reference
(src/hybrid_solver.py:32), where the stencil radius only names the checkpoint
and the graph is always the ±1 chain.  `graph_radius` is the real one, opt-in:
graph_radius=R (1..3, default 1) runs FluxGNN on the radius-R chain graph
(graph_constructor.chain_edge_index(radius=R): mean over the 2R neighbours) in
the same fused f32 kernels, the solver reading that graph's first 2*nx fluxes.
HybridSolver(path, 3, graph_radius=3) is the intended call for a checkpoint
trained with train_model(..., graph_radius=3).
"""
import math
import os

import numpy as np
import torch

from . import engine
from .baseline_solver import BaselineSolver
from .config import MODEL_CONFIG
from .flux_gnn import FluxGNN


def load_state_dict(model_path):
    """Checkpoint -> state dict without executing anything from the file:
    .pt/.pth via torch.load(weights_only=True), .npz via numpy (no pickle), or
    an in-memory mapping."""
    if isinstance(model_path, dict):
        return {k: torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v
                for k, v in model_path.items()}
    path = os.fspath(model_path)
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as d:
            return {k: torch.from_numpy(d[k].copy()) for k in d.files}
    return torch.load(path, map_location="cpu", weights_only=True)


class HybridSolver:
    def __init__(self, model_path, radius, nx=64, length=2 * math.pi, dt=5e-3, t_end=1.0, device="cuda",
                 precision="f32", poisson="spectral", num_layers=None, graph_radius=1):
        """precision: chain-kernel arithmetic, "f32" (default, exact float32
        MFMA), "f16x3" (float32-accurate split-fp16 MFMA, ~5x the matrix rate)
        or "bf16" (bf16 weights/activations, BASELINE config 4).
        poisson: "spectral" (default, the reference's operator) or
        "tridiagonal" (opt-in, NOT the reference's: the north star's
        cyclic-reduction solve fused into the same step kernels; engine.Grid).
        num_layers: the checkpoint's update layers (default MODEL_CONFIG's, the
        reference's only depth).
        graph_radius: the stencil radius the model's graph really has (1..3;
        nx >= 2*graph_radius + 1; beyond 1 precision must be "f32").  `radius`
        stays the checkpoint label it is in the reference."""
        self.graph_radius = int(graph_radius)
        if not 1 <= self.graph_radius <= 3:
            raise ValueError(f"graph_radius must be 1, 2 or 3, got {graph_radius!r}")
        if self.graph_radius > 1 and precision != "f32":
            raise ValueError(f"graph_radius > 1 runs on the f32 core only, got precision {precision!r}")
        if self.graph_radius > 1 and nx < 2 * self.graph_radius + 1:
            raise ValueError(f"graph_radius {self.graph_radius} needs nx >= {2 * self.graph_radius + 1}, got {nx}")
        self.device = torch.device(device)
        self.baseline = BaselineSolver(nx=nx, length=length, dt=dt, t_end=t_end, device=self.device,
                                       poisson=poisson)
        model = FluxGNN(input_dim=MODEL_CONFIG["input_dim"], hidden_dim=MODEL_CONFIG["hidden_dim"],
                        num_layers=MODEL_CONFIG["num_layers"] if num_layers is None else int(num_layers),
                        precision=precision)
        model.load_state_dict(load_state_dict(model_path))
        self.model = model.to(self.device)
        self.model.eval()
        self.radius = radius

    @property
    def grid(self):
        return self.baseline.grid

    def _dm(self):
        return self.model.device_model(self.device, self.graph_radius)

    def _upload(self, states):
        return self.baseline._upload(states)

    # reference-shaped API --------------------------------------------------------
    def step(self, state):
        out, _, _ = engine.step(self._dm(), self.grid, self._upload(state)[None])
        return out[0].cpu().numpy()

    def run(self, state0, n_steps=40):
        r = engine.run(self._dm(), self.grid, self._upload(state0)[None], n_steps, traj=True)
        return r["traj"][0].cpu().numpy()

    # batched device API ------------------------------------------------------------
    def step_batch(self, states, return_flux=False, metrics=False):
        """states [B,3,nx] -> next states (device).  With return_flux/metrics returns
        (states, F [B,nx], metrics [B,4])."""
        out, F, M = engine.step(self._dm(), self.grid, self._upload(states), flux_face=return_flux,
                                metrics=metrics)
        return (out, F, M) if (return_flux or metrics) else out

    def compare_batch(self, states0, n_steps, metrics=True, out=None, ws=None):
        """Roll B ICs out with this solver AND with the classical BaselineSolver
        (same dt, nu = 1e-3 as BaselineSolver's default) in one launch and score
        them per step.  Returns dict(final, mse [B,T+1,3] for (n,u,E),
        metrics, metrics_classical).  mse.sum(-1).mean(-1) is the per-IC number
        of scripts/evaluation/evaluate_multi_ic.py:88-94."""
        return engine.run_compare(self._dm(), self.grid, self._upload(states0), n_steps, metrics=metrics, out=out,
                                  ws=ws)

    def run_batch(self, states0, n_steps, traj=True, flux=False, metrics=False, out=None, ws=None):
        """Rollout of B ICs: dict(final [B,3,nx], traj [B,T+1,3,nx] | None,
        flux [B,T,nx] | None, metrics [B,T+1,4] | None), all on the device.
        out (may be states0 itself) and ws (engine.workspace) are optional
        preallocated buffers, so a timed loop allocates nothing."""
        return engine.run(self._dm(), self.grid, self._upload(states0), n_steps, traj=traj, flux=flux,
                          metrics=metrics, out=out, ws=ws)


class HybridEnsemble:
    """M HybridSolvers rolled out together: an ablation sweep's checkpoints, or
    an ensemble's members, as ONE launch at nx 16/32/48/64 (hf_run_set: every
    workgroup picks its model's weights), model after model at any other nx.
    The solvers share nx, the grid constants, the Poisson mode, the precision,
    the device and the graph radius (ValueError names the first mismatch); their
    depths may differ.  run_batch / compare_batch take HybridSolver's arguments and return
    its dicts with a leading model axis, model m's block bit-identical to
    solvers[m]'s own call.  states0 [B,3,nx] is shared by all models;
    [M,B,3,nx] gives each model its own ICs.

    Ensemble statistics are torch reductions over that axis:

        ens = HybridEnsemble.from_checkpoints(paths, radius=1)
        traj = ens.run_batch(states0, 50)["traj"]          # [M,B,T+1,3,nx]
        mean, spread = traj.mean(0), traj.std(0)           # [B,T+1,3,nx] each
    """

    def __init__(self, solvers):
        self.solvers = list(solvers)
        if not self.solvers:
            raise ValueError("HybridEnsemble needs at least one HybridSolver")
        ref = self.signature(self.solvers[0])
        for i, s in enumerate(self.solvers[1:], 1):
            for name, a, b in zip(self.SIGNATURE, ref, self.signature(s)):
                if a != b:
                    raise ValueError(f"HybridEnsemble: solver {i} has {name} = {b!r}, solver 0 has {a!r}; the "
                                     f"members of an ensemble share {', '.join(self.SIGNATURE)}")
        self.device = self.solvers[0].device
        self._set = None

    SIGNATURE = ("nx", "length", "dt", "nu", "poisson", "precision", "device", "graph_radius")

    @staticmethod
    def signature(solver):
        """What two HybridSolvers must share to roll out in one launch (SIGNATURE's fields)."""
        g = solver.grid
        return (g.nx, g.length, g.dt, g.nu, g.poisson, solver.model.precision, str(torch.device(solver.device)),
                getattr(solver, "graph_radius", 1))

    @classmethod
    def from_checkpoints(cls, paths, radius=1, **solver_kw):
        """One HybridSolver per checkpoint path (or state dict), all with solver_kw."""
        return cls([HybridSolver(p, radius, **solver_kw) for p in paths])

    def __len__(self):
        return len(self.solvers)

    def __getitem__(self, i):
        return self.solvers[i]

    @property
    def grid(self):
        return self.solvers[0].grid

    def _model_set(self):
        """The DeviceModelSet of the solvers' current weights (rebuilt when a solver repacked its own)."""
        dms = [s._dm() for s in self.solvers]
        if self._set is None or len(self._set.models) != len(dms) or \
                any(a is not b for a, b in zip(self._set.models, dms)):
            if self._set is not None:
                self._set.close()
            self._set = engine.DeviceModelSet(dms)
        return self._set

    def _states(self, states0):
        s0 = self.solvers[0]._upload(states0)
        nx, M = self.grid.nx, len(self.solvers)
        if s0.dim() not in (3, 4) or tuple(s0.shape[-2:]) != (3, nx) or (s0.dim() == 4 and s0.shape[0] != M):
            raise ValueError(f"states0 must be [B,3,{nx}] (shared by the {M} models) or [{M},B,3,{nx}] (ICs per "
                             f"model), got {tuple(s0.shape)}")
        return s0

    @staticmethod
    def _check_out(s0, out):
        if out is not None and s0.dim() == 3 and isinstance(out, torch.Tensor) and s0.numel() and \
                out.device == s0.device and out.untyped_storage().data_ptr() == s0.untyped_storage().data_ptr():
            raise ValueError("out must not share memory with states0 when the models share their ICs; pass "
                             "states0 as [M,B,3,nx] to roll out in place")

    def run_batch(self, states0, n_steps, traj=True, flux=False, metrics=False, out=None, ws=None):
        """HybridSolver.run_batch for every model: dict(final [M,B,3,nx], traj
        [M,B,T+1,3,nx] | None, flux [M,B,T,nx] | None, metrics [M,B,T+1,4] | None).
        out [M,B,3,nx] may be states0 itself when states0 is [M,B,3,nx]."""
        s0 = self._states(states0)
        self._check_out(s0, out)
        return engine.run_set(self._model_set(), self.grid, s0, n_steps, traj=traj, flux=flux, metrics=metrics,
                              out=out, ws=ws)

    def compare_batch(self, states0, n_steps, metrics=True, out=None, ws=None):
        """HybridSolver.compare_batch for every model: dict(final, mse [M,B,T+1,3],
        metrics, metrics_classical), the classical twin stepped beside each."""
        s0 = self._states(states0)
        self._check_out(s0, out)
        return engine.run_compare_set(self._model_set(), self.grid, s0, n_steps, metrics=metrics, out=out, ws=ws)
