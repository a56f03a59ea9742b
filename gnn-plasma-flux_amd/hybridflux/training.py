"""FluxGNN training on the MI355X (differentiable hybrid step).

Mirrors scripts/training/train_ablation.py (FluxDataset, train_model and the
per-sample ablation loss of :107-200).  FluxGNN's forward and backward run in
the HIP training kernels through FluxGNN's autograd Function (on tagged
chains the chain-layout MFMA GEMMs of train_chain.hip / tgemm.h, on other
graphs the generic kernels of graph.hip); the
loss assembly, the finite-volume update it differentiates through and Adam are
the reference trainer's own torch expressions, executed on the device.

Batching: the reference trains with batch size 1 (DataLoader(batch_size=1),
:85).  `batch_size=1` reproduces that loop step for step; `batch_size=B`
evaluates B samples as one batched graph (B disjoint chains) and averages the
per-sample losses, which for every term equals the mean of the B
single-sample losses — the batched training the survey asks for.

As in the reference, the Poisson / energy terms go through a detached
Poisson solve (there numpy, :138-145; here hf_poisson), so they contribute to
the loss value but not to the gradient; the multi-step rollout energies depend
only on u, which the model does not touch (:174-196).

PureGNN (scripts/training/train_pure_gnn.py:79-151) trains here too, at the
end of this module: state_mse_loss (hf_state_mse), pure_gnn_step and
train_pure_gnn, over PureGNN's own autograd Function (baselines.py,
pure_train.hip).

Both models also train through their rollouts, K steps deep: unrolled_loss /
unrolled_step / train_unrolled for FluxGNN through the hybrid solver
(unroll.hip), pure_unrolled_loss / pure_unrolled_step /
train_pure_gnn_unrolled for PureGNN through state <- state + PureGNN(...)
(pure_unroll.hip).  The two are one driver (_rollout_forward /
_rollout_backward / _RolloutLoss / _rollout_step / _train_windows) over a
_Rollout description of each model.

Every trainer hands the kernels the parameters as one flat buffer and gets the
gradient back as one (flat.py).

PINN (scripts/training/train_pinn.py:64-201) trains at the end of this module:
pinn_forward (PINN.forward itself stays inference only), pinn_physics_loss
(hf_pinn_loss), pinn_step and train_pinn, over pinn_train.hip; and through K
steps of its own rollout, as the two graph models and on their driver:
pinn_unrolled_loss / pinn_unrolled_step / train_pinn_unrolled (pinn_unroll.hip),
with the state loss of the other two and, on request, the physics residuals
evaluated on the model's own previous state.

All three K-step losses take conservation=(lam_e, lam_q): energy and charge
terms on the predicted states, which under a K-step loss carry a gradient (the
reference's never do), formed inside the launches the driver already makes (the
_ex entry points) from per-IC float64 sums; _Cons, _cons_refs and the
workspace_ex hook of _Rollout are all the driver needs for them.

All three K-step trainers take noise=StateNoise(...): every window starts from
its first state plus seeded Gaussian noise drawn on the device
(engine.state_noise, hf_state_noise) against the clean targets; the datasets'
batch(..., noise=, seeds=) is where it is applied.
"""
import json
import os
import time
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import engine
from .baseline_solver import BaselineSolver
from .baselines import PINN, PureGNN
from .config import ABLATION_CONFIGS, MODEL_CONFIG
from .flat import assign_grads, drives_exactly, flat_params, flat_view, split_flat
from .flux_gnn import FluxGNN
from .graph_constructor import build_chain_graph_batch, shared_chain_edge_index


def _mse(a, b):
    return torch.mean((a - b) ** 2)


def _poisson_detached(grid, n):
    """E of densities n [B,nx] without gradient (train_ablation.py:47-57 solve_poisson_np)."""
    return engine.poisson(grid, n.detach())


class _StepLoss(torch.autograd.Function):
    """The loss terms as one HIP pass (hf_ablation_loss_ex): forward returns
    (loss, flux_loss) and keeps d loss / d flux_edge, which backward scales by
    the incoming gradient.  flux_loss is for reporting only.  roll = (K,
    lambda_energy_multi, dt) adds the rollout energy term (K <= 3), which
    carries no gradient."""

    @staticmethod
    def forward(ctx, flux_edge, st, ft, sn, grid, lam, roll):
        K, lam_m, dt = roll
        loss, fl, dfe = engine.ablation_loss_terms(grid, flux_edge, st, ft, sn, tuple(lam) + (lam_m,), K, dt)
        ctx.save_for_backward(dfe)
        ctx.mark_non_differentiable(fl)
        return loss, fl

    @staticmethod
    def backward(ctx, g_loss, g_fl):
        (dfe,) = ctx.saved_tensors
        return dfe * g_loss, None, None, None, None, None, None


def _has_rollout(cfg):
    return cfg["rollout_steps"] > 0 and cfg["lambda_energy_multi"] > 0  # train_ablation.py:172


def _solver_edges(flux, B, nx, graph_radius=1):
    """The [B, 2nx] fluxes the solver reads out of FluxGNN.forward's result on B
    chains: all of it on the ±1 chain; on a radius-R graph the first 2nx of each
    IC's 2*R*nx (graph_constructor.chain_edge_index), the long edges' fluxes
    getting a zero gradient from autograd."""
    if graph_radius == 1:
        return flux.reshape(B, 2 * nx)
    return flux.reshape(B, 2 * graph_radius * nx)[:, :2 * nx].contiguous()


def ablation_loss(model, st, ft, st_next, x, dt, dx, cfg, grid, n0=1.0, fused=True, nf=None, rollout="reuse",
                  graph_radius=1):
    """Loss of train_ablation.py:107-206 for a batch: st, st_next [B,3,nx], ft [B,nx]
    on the device.  Returns (loss, flux_loss); B=1 is the reference formula.
    fused: the terms (:124-170, and the rollout energy term for rollout_steps
    <= 3) in one HIP pass (hf_ablation_loss_ex) instead of the torch
    expressions below (kept as the readable statement of the same arithmetic,
    and for the comparison tests).  nf: the batch's chain node features when
    the caller has them (FluxDataset.batch with x).  rollout (torch form only):
    "reuse" runs no model forward whose result cannot reach the loss
    (_rollout_energies), "literal" the reference's loop of rollout_steps
    forwards (_rollout_energies_literal); the two give the same loss bit for bit.
    graph_radius: the stencil radius of the model's graph (1..3).  Beyond 1 the
    model runs on the radius chain graph (FluxGNN's autograd Function on the
    generic kernels) and the loss reads that graph's first 2nx fluxes per IC."""
    B, _, nx = st.shape
    n_t, u_t = st[:, 0], st[:, 1]
    n_next_true, u_next_true, E_next_true = st_next[:, 0], st_next[:, 1], st_next[:, 2]
    if nf is None:
        nf, ei = build_chain_graph_batch(st, x, radius=graph_radius)
    else:
        ei = shared_chain_edge_index(nx, B, st.device, graph_radius)
    flux_edge = _solver_edges(model(nf, ei), B, nx, graph_radius)
    if fused and n0 == 1.0 and abs(dt / dx - grid.dt / grid.dx) <= 1e-12 * abs(dt / dx):
        lam = (cfg["lambda_state"], cfg["lambda_poisson"], cfg["lambda_charge"], cfg["lambda_energy_one"])
        K = cfg["rollout_steps"] if _has_rollout(cfg) else 0
        in_kernel = K <= engine.LOSS_MAX_ROLLOUT
        roll = (K, cfg["lambda_energy_multi"], dt) if in_kernel else (0, 0.0, dt)
        loss, flux_loss = _StepLoss.apply(flux_edge, st, ft, st_next, grid, lam, roll)
        if not in_kernel:  # later energies need forwards on later states
            loss = _add_rollout_term(loss, cfg, _rollout_energies(model, st, flux_edge, x, dt, dx, cfg, grid,
                                                                  graph_radius))
        return loss, flux_loss
    F_pred = 0.5 * (flux_edge[:, :nx] + flux_edge[:, nx:])                        # :124-126
    flux_loss = _mse(F_pred, ft)                                                   # :129
    loss = flux_loss
    n_next_pred = n_t - (dt / dx) * (F_pred - torch.roll(F_pred, 1, dims=-1))     # :134-135
    if cfg["lambda_state"] > 0:
        loss = loss + cfg["lambda_state"] * _mse(n_next_pred, n_next_true)
    E_next_pred = None
    if cfg["lambda_poisson"] > 0 or cfg["lambda_energy_one"] > 0:
        E_next_pred = _poisson_detached(grid, n_next_pred)
    if cfg["lambda_poisson"] > 0:                                                  # :140-147
        loss = loss + cfg["lambda_poisson"] * _mse(E_next_pred, E_next_true)
    if cfg["lambda_charge"] > 0:                                                   # :150-156
        charge_t = torch.sum(n_t - n0, dim=-1) * dx
        charge_next = torch.sum(n_next_pred - n0, dim=-1) * dx
        loss = loss + cfg["lambda_charge"] * _mse(charge_next, charge_t)
    if cfg["lambda_energy_one"] > 0:                                               # :159-170
        e_p = 0.5 * torch.mean(u_next_true ** 2 + E_next_pred ** 2, dim=-1)
        e_t = 0.5 * torch.mean(u_next_true ** 2 + E_next_true ** 2, dim=-1)
        loss = loss + cfg["lambda_energy_one"] * _mse(e_p, e_t)
    if _has_rollout(cfg):
        if rollout == "literal":
            energies = _rollout_energies_literal(model, st, x, dt, dx, cfg, grid, graph_radius)
        else:
            energies = _rollout_energies(model, st, flux_edge, x, dt, dx, cfg, grid, graph_radius)
        loss = _add_rollout_term(loss, cfg, energies)
    return loss, flux_loss


def _add_rollout_term(loss, cfg, energies):
    """+ lambda_energy_multi * mean((energies - energies[0])^2) (:204-206)."""
    return loss + cfg["lambda_energy_multi"] * torch.mean((energies - energies[0]) ** 2)


def _rollout_energies_literal(model, st, x, dt, dx, cfg, grid, graph_radius=1):
    """The rollout energies [K, B] as the reference's loop computes them
    (:173-204): K model forwards, one per rolled state."""
    B, _, nx = st.shape
    state = st.clone()
    energies = []
    for _ in range(cfg["rollout_steps"]):
        n_r, u_r, E_r = state[:, 0], state[:, 1], state[:, 2]
        energies.append(0.5 * torch.mean(u_r ** 2, dim=-1))                         # :181-182
        nf_r, ei_r = build_chain_graph_batch(state, x, radius=graph_radius)
        fe_r = _solver_edges(model(nf_r, ei_r), B, nx, graph_radius)
        F_r = 0.5 * (fe_r[:, :nx] + fe_r[:, nx:])
        n_next_r = n_r - (dt / dx) * (F_r - torch.roll(F_r, 1, dims=-1))
        F_u = 0.5 * u_r * u_r
        u_next_r = u_r - (dt / dx) * (F_u - torch.roll(F_u, 1, dims=-1)) + dt * E_r
        state = torch.stack([n_next_r, u_next_r, _poisson_detached(grid, n_next_r)], dim=1)
    return torch.stack(energies)                                                   # [K, B]


def _rollout_energies(model, st, flux_edge, x, dt, dx, cfg, grid, graph_radius=1):
    """The same energies [K, B] as _rollout_energies_literal, bit for bit, with
    only the forwards whose results reach them.  The energy of step k is
    0.5 mean(u_k^2) (:181) and u_{k+1} needs E_k (:196), which for k >= 1 is
    the detached Poisson E of the n_k that forward k-1 produced (:191, :198-
    200).  So the energies reach forwards 0 .. K-3 only, forward 0 is the main
    forward (the same model on the same state: its flux_edge is reused), and
    the others run untaped (no_grad: nothing differentiates through them — u
    never depends on the parameters).  For the reference's K = 3: no forward."""
    B, _, nx = st.shape
    K = cfg["rollout_steps"]
    n_r, u_r, E_r = st[:, 0], st[:, 1], st[:, 2]
    fe_r = flux_edge.detach()
    energies = []
    for k in range(K):
        energies.append(0.5 * torch.mean(u_r ** 2, dim=-1))
        if k == K - 1:
            break
        F_u = 0.5 * u_r * u_r
        u_next = u_r - (dt / dx) * (F_u - torch.roll(F_u, 1, dims=-1)) + dt * E_r
        n_next = E_next = None
        if k + 2 <= K - 1:  # E_{k+1} feeds u_{k+2}, the last energy's u at k + 2 = K - 1
            if fe_r is None:
                with torch.no_grad():
                    nf_r, ei_r = build_chain_graph_batch(torch.stack([n_r, u_r, E_r], dim=1), x, radius=graph_radius)
                    fe_r = _solver_edges(model(nf_r, ei_r), B, nx, graph_radius)
            F_r = 0.5 * (fe_r[:, :nx] + fe_r[:, nx:])
            n_next = n_r - (dt / dx) * (F_r - torch.roll(F_r, 1, dims=-1))
            E_next = _poisson_detached(grid, n_next)
        fe_r = None
        n_r, u_r, E_r = n_next, u_next, E_next
    return torch.stack(energies)


def train_flop_per_sample(cfg, nx=64, H=128, L=4, F=4):
    """Algorithmic FLOPs of one sample of the training step with the ablation
    config `cfg` (a dict of ABLATION_CONFIGS or its name): FluxGNN forward +
    backward (P/Q-split readout, as the inference count of SURVEY.md 8d):
    forward 329,216 per cell (input 2FH, layers L*2*2H*H, readout 2*H*2H +
    2 edges * 2H), backward = data gradients (layers L*2*2H*H, readout 2*2H*H)
    + weight gradients (the same GEMM sizes, plus the input layer's 2FH).  The
    rollout energy term ('full', 'rollout_only') adds only the forwards whose
    results reach the loss, none for the reference's rollout_steps = 3
    (_rollout_energies; the reference's own loop runs 3 forwards there, of
    which none is needed), and no backward (the term has no gradient).  The
    loss terms' elementwise FV updates and detached Poisson solves are not counted."""
    if isinstance(cfg, str):
        cfg = ABLATION_CONFIGS[cfg]
    fwd = 2 * F * H + L * 2 * 2 * H * H + 2 * H * 2 * H + 2 * 2 * H
    bwd = (L * 2 * 2 * H * H + 2 * 2 * H * H) * 2 + 2 * F * H
    extra = max(0, cfg["rollout_steps"] - 3) if _has_rollout(cfg) else 0
    return ((fwd + bwd) + extra * fwd) * nx


class StateNoise:
    """Seeded Gaussian noise on a training step's start state (the targets stay
    clean, so the model learns to pull a drifted state back):
    engine.state_noise with sigma = (sigma_n, sigma_u, sigma_E), one
    np.random.RandomState(seed).standard_normal(3 nx) per sample, drawn on the
    device.  zero_mean: the n noise loses its mean, so the charge is kept.  grid
    (an engine.Grid): E is recomputed from the perturbed n with the grid's
    Poisson solve, so the start is a consistent solver state; sigma_E must then
    be 0.  Passed as noise= to WindowDataset.batch, FluxDataset.batch and the
    K-step trainers."""

    def __init__(self, sigma_n, sigma_u, sigma_E=0.0, zero_mean=True, grid=None):
        self.sigma = engine.noise_sigma((sigma_n, sigma_u, sigma_E))
        self.zero_mean, self.grid = bool(zero_mean), grid
        if grid is not None and self.sigma[2] != 0:
            raise ValueError("StateNoise: with a grid E is recomputed from the perturbed n: sigma_E must be 0")

    def with_grid(self, grid):
        """This noise with E recomputed on grid."""
        return StateNoise(*self.sigma, zero_mean=self.zero_mean, grid=grid)

    def apply(self, state, seeds, x=None):
        """state [B,3,nx] perturbed with one seed per sample (a new tensor);
        with x [nx] also the node features [B*nx,4] of the perturbed state."""
        return engine.state_noise(state, seeds, self.sigma, self.zero_mean, self.grid, x)


def _noise_seeds(noise, seeds):
    if noise is not None and seeds is None:
        raise ValueError("noise needs seeds: one integer in [0, 2**32) per sample of the batch")
    if noise is None and seeds is not None:
        raise ValueError("seeds given without noise")


class FluxDataset:
    """Device-resident (state_t, flux_t, state_next) triples (train_ablation.py:27-44)."""

    def __init__(self, state_t, flux_t, state_next, device="cuda"):
        assert state_t.shape == state_next.shape and state_t.shape[0] == flux_t.shape[0]
        as_t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=device)  # noqa: E731
        self.state_t, self.flux_t, self.state_next = as_t(state_t), as_t(flux_t), as_t(state_next)
        self.N, self.C, self.nx = self.state_t.shape

    def __len__(self):
        return self.N

    def check_indices(self, idx):
        """IndexError unless every index lies in [-N, N) (torch indexing's
        range; one host sync)."""
        idx = torch.as_tensor(idx)
        if idx.numel() and (int(idx.min()) < -self.N or int(idx.max()) >= self.N):
            raise IndexError(f"sample index out of range for a dataset of {self.N} samples")

    def batch(self, idx, x=None, check=True, noise=None, seeds=None):
        """(state_t, flux_t, state_next)[idx]; with x (the grid positions [nx])
        also the batch's chain node features, all four from one HIP pass
        (engine.chain_batch): (st, ft, sn, node_features).  Indices outside
        [-N, N) raise IndexError as the reference's dataset indexing does
        (check_indices: a host sync); check=False skips that for indices the
        caller has already checked (train_steps checks a pass's order once),
        and then the device gather clamps an out-of-range index to [0, N)
        instead of raising (include/hybridflux.h hf_chain_batch_gather).
        noise (a StateNoise) with seeds (one per sample of the batch): state_t
        is perturbed and the node features are rebuilt from it; flux_t and
        state_next stay clean."""
        _noise_seeds(noise, seeds)
        if check:
            self.check_indices(idx)
        if x is None:
            st, ft, sn = self.state_t[idx], self.flux_t[idx], self.state_next[idx]
            return (st if noise is None else noise.apply(st.contiguous(), seeds)), ft, sn
        st, ft, sn, nf = engine.chain_batch(idx, self.state_t, self.flux_t, self.state_next, x)
        if noise is not None:
            x32 = torch.as_tensor(x, dtype=torch.float32, device=st.device).reshape(-1).contiguous()
            st, nf = noise.apply(st, seeds, x=x32)
        return st, ft, sn, nf


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam (weight decay 0, no amsgrad: the reference trainer's
    optimizer, train_ablation.py:82, :208-209) for a model whose parameters
    share one buffer (FluxGNN.flatten_parameters_): the update of every
    parameter in one HIP launch (hf_adam_flat) with the step count on the
    device, so it is capturable (GraphedStep) and needs no host sync.  The
    gradients are read as one buffer when they are (the chain training
    backward returns them as pieces of one), otherwise concatenated first.

    The keyword options guard the step on the device (hf_adam_flat_ex; two
    launches, still no host sync, still capturable): max_grad_norm clips the
    gradient by its global L2 norm (torch.nn.utils.clip_grad_norm_'s
    arithmetic), weight_decay is torch.optim.AdamW's decoupled decay, and
    skip_nonfinite leaves parameters, moments and step count untouched when
    the gradient norm is inf or NaN.  lr may be a one-element float32 tensor:
    it is moved to the parameters' device once and the kernel reads it there,
    so a torch.optim.lr_scheduler (which fills a tensor lr in place) also
    drives a captured step.  With clipping or skipping on, last_stats is the
    device tensor [4] = (norm before clipping, coefficient applied, skipped
    0/1, skipped steps so far) of the most recent step (state["stats"], saved
    and loaded with the rest); otherwise it is None.  With the three options
    at their defaults and a float lr the step is the one hf_adam_flat launch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, weight_decay=0.0, max_grad_norm=None,
                 skip_nonfinite=False):
        if not float(weight_decay) >= 0.0:
            raise ValueError(f"FlatAdam: weight_decay must be >= 0, got {weight_decay}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"FlatAdam: max_grad_norm must be > 0 (None: no clipping), got {max_grad_norm}")
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("FlatAdam: a tensor lr must hold one value")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=float(weight_decay),
                                      max_grad_norm=None if max_grad_norm is None else float(max_grad_norm),
                                      skip_nonfinite=bool(skip_nonfinite)))
        self._ws = {}
        for group in self.param_groups:
            ps = group["params"]
            flat = flat_view(ps, ps[0].device)
            if flat is None:
                raise ValueError("FlatAdam: the parameters must share one float32 buffer in order "
                                 "(call model.flatten_parameters_() first)")
            st = self.state[ps[0]]  # (the buffer itself is found again each step: state_dict() stays plain)
            st["exp_avg"] = torch.zeros_like(flat)
            st["exp_avg_sq"] = torch.zeros_like(flat)
            st["step"] = torch.zeros(1, dtype=torch.float32, device=flat.device)
            # the kernel's done-counter: 4 zero bytes (float32 so that load_state_dict's cast keeps them 0)
            st["done"] = torch.zeros(1, dtype=torch.float32, device=flat.device)
            if self._needs_norm(group):
                st["stats"] = torch.zeros(engine.OPT_NUM_STATS, dtype=torch.float32, device=flat.device)
            if isinstance(group["lr"], torch.Tensor):
                group["lr"] = self._device_lr(group["lr"], flat.device)

    @staticmethod
    def _needs_norm(group):
        return group.get("max_grad_norm") is not None or bool(group.get("skip_nonfinite"))

    @staticmethod
    def _device_lr(lr, dev):
        """A tensor lr as float32 on dev: the tensor itself when it already is."""
        if lr.device == dev and lr.dtype == torch.float32 and lr.is_contiguous() and not lr.requires_grad:
            return lr
        return lr.detach().to(device=dev, dtype=torch.float32).contiguous()

    @property
    def guarded(self):
        """Some group clips or skips: its steps write last_stats."""
        return any(self._needs_norm(g) for g in self.param_groups)

    @property
    def last_stats(self):
        """The most recent step's statistics [4] on the device (of the first
        group that keeps them; it is overwritten by the next step), or None."""
        for group in self.param_groups:
            st = self.state[group["params"][0]]
            if "stats" in st:
                return st["stats"]
        return None

    def load_state_dict(self, state_dict):
        """torch's, except that a tensor lr keeps its address (a captured step
        reads it there): the loaded value is copied into it."""
        held = [g["lr"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, lr in zip(self.param_groups, held):
            if isinstance(lr, torch.Tensor):
                new = group["lr"]
                lr.copy_(new.reshape(lr.shape) if isinstance(new, torch.Tensor) else torch.as_tensor(float(new)))
                group["lr"] = lr

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            ps = group["params"]
            st = self.state[ps[0]]
            flat = flat_view(ps, ps[0].device)
            if flat is None:
                raise RuntimeError("FlatAdam: the parameters no longer share one buffer (moved or re-created?)")
            if any(p.grad is None for p in ps):
                raise RuntimeError("FlatAdam: every parameter needs a gradient")
            norm = self._needs_norm(group)
            if norm and "stats" not in st:  # (options switched on later, or a plain optimizer's state loaded)
                st["stats"] = torch.zeros(engine.OPT_NUM_STATS, dtype=torch.float32, device=flat.device)
            for k in ("exp_avg", "exp_avg_sq", "step", "done") + (("stats",) if "stats" in st else ()):
                if st[k].device != flat.device or st[k].dtype != torch.float32 or not st[k].is_contiguous():
                    # (a state_dict loaded elsewhere)
                    st[k] = st[k].to(device=flat.device, dtype=torch.float32).contiguous()
            g = flat_view([p.grad for p in ps], ps[0].device)
            if g is None:
                g = torch.cat([p.grad.reshape(-1) for p in ps])
            b1, b2 = group["betas"]
            lr, wd = group["lr"], group.get("weight_decay", 0.0)
            if isinstance(lr, torch.Tensor):
                lr = group["lr"] = self._device_lr(lr, flat.device)
            if not norm and wd == 0.0 and not isinstance(lr, torch.Tensor):
                engine.adam_flat(flat, g, st["exp_avg"], st["exp_avg_sq"], st["step"], st["done"], lr, b1, b2,
                                 group["eps"])
            else:
                ws = None
                if norm:
                    ws = self._ws.get(gi)
                    if ws is None or ws.device != flat.device:
                        ws = self._ws[gi] = engine.adam_flat_workspace(flat.numel(), flat.device)
                max_norm = group.get("max_grad_norm")
                engine.adam_flat_ex(flat, g, st["exp_avg"], st["exp_avg_sq"], st["step"], st["done"], lr, b1, b2,
                                    group["eps"], wd, float("inf") if max_norm is None else max_norm,
                                    bool(group.get("skip_nonfinite")), ws, st["stats"] if norm else None)
            # the kernel wrote the parameters behind autograd's back: bump their
            # version counters as an in-place torch update would, so that a packed
            # inference copy (FluxGNN.device_model keys on _version) is rebuilt
            torch.autograd.graph.increment_version(ps)
        return loss


class _StepStats:
    """The statistics of a guarded optimizer's steps over one epoch: each step's
    last_stats is copied on the device (note) and all are read in the epoch's one
    host sync (read), which appends the epoch's grad_norm_max and skipped_steps to
    the trainer's history.  Off -- no key, nothing copied or read -- for any other
    optimizer."""

    def __init__(self, opt, history):
        self.opt = opt if isinstance(opt, FlatAdam) and opt.guarded else None
        self.history, self.rows, self.weights, self.weight = history, [], [], 0
        if self.opt is not None:
            history.update(grad_norm_max=[], skipped_steps=[])

    def __bool__(self):
        return self.opt is not None

    def note(self, weight=1):
        """After a step over `weight` samples."""
        if self.opt is not None:
            self.rows.append(self.opt.last_stats.clone())
            self.weights.append(weight)

    def read(self):
        """Per step of the epoch whether it was applied; `weight` becomes the
        samples of those steps.  grad_norm_max is taken over the applied steps."""
        rows = torch.stack(self.rows).tolist() if self.rows else []
        applied = [r[2] == 0.0 for r in rows]
        norms = [r[0] for r, a in zip(rows, applied) if a]
        self.history["grad_norm_max"].append(max(norms, key=lambda v: (v != v, v)) if norms else 0.0)  # (a NaN wins)
        self.history["skipped_steps"].append(len(rows) - sum(applied))
        self.weight = sum(w for w, a in zip(self.weights, applied) if a)
        self.rows, self.weights = [], []
        return applied


def _guarded_optimizer(params, lr, weight_decay, max_grad_norm, skip_nonfinite, scheduler, device):
    """The trainers' FlatAdam and its scheduler (None without one): with a
    scheduler -- a callable opt -> torch.optim.lr_scheduler.LRScheduler -- lr is a
    device tensor, which the scheduler's steps rewrite in place."""
    if scheduler is not None:
        lr = torch.full((), float(lr), dtype=torch.float32, device=device)
    opt = FlatAdam(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                   skip_nonfinite=skip_nonfinite)
    return opt, (scheduler(opt) if scheduler is not None else None)


def direct_step(model, opt, st, ft, sn, nf, x, dt, dx, cfg, grid, graph_radius=1):
    """One step of the reference trainer's loop (ablation_loss ->
    loss.backward() -> optimizer.step(), train_ablation.py:107-210) without
    autograd where it reduces to three HIP passes and the optimizer launch:
    FluxGNN with flat parameters (flatten_parameters_), FlatAdam over exactly
    those parameters, the one-pass loss (rollout_steps <= 3), and the batch's
    chain node features nf (FluxDataset.batch with x).  The forward
    (hf_graph_forward_train), the loss and its flux gradient
    (hf_ablation_loss_ex), the backward (hf_graph_backward) with that gradient
    as the incoming one -- autograd's seed is 1 and _StepLoss.backward's
    product dfe * 1 is dfe exactly -- and FlatAdam on the gradient buffer: the
    same parameters bit for bit as the autograd step, without its seed fill,
    gradient product and bookkeeping launches.  Parameter hooks are not run.
    Returns (loss, flux_loss) detached, or None when the case does not apply
    (the caller then takes the autograd step).  It declines a graph_radius
    beyond 1: the radius graph goes through ablation_loss's autograd step."""
    if graph_radius != 1:
        return None
    if type(model) is not FluxGNN or not isinstance(opt, FlatAdam) or nf is None or not torch.is_grad_enabled():
        return None
    params = list(model.parameters())
    if not drives_exactly(opt, params):
        return None
    dev = st.device
    flat = flat_view(params, dev)
    K = cfg["rollout_steps"] if _has_rollout(cfg) else 0
    if flat is None or K > engine.LOSS_MAX_ROLLOUT or abs(dt / dx - grid.dt / grid.dx) > 1e-12 * abs(dt / dx):
        return None
    B, _, nx = st.shape
    dims = (model.input_dim, model.hidden_dim, model.num_layers)
    flux, tape, nf_d, ei_d, chain_nx = engine.graph_forward_train(flat, dims, nf.detach(),
                                                                  shared_chain_edge_index(nx, B, dev))
    lam = (cfg["lambda_state"], cfg["lambda_poisson"], cfg["lambda_charge"], cfg["lambda_energy_one"],
           cfg["lambda_energy_multi"])
    loss, flux_loss, dfe = engine.ablation_loss_terms(grid, flux.reshape(B, 2 * nx), st, ft, sn, lam, K, dt)
    gp, _ = engine.graph_backward(flat, dims, nf_d, ei_d, chain_nx, tape, dfe.reshape(-1), False)
    assign_grads(params, gp)
    opt.step()
    return loss.detach(), flux_loss.detach()


class GraphedStep:
    """One optimizer step of the reference trainer's loop (ablation_loss ->
    backward -> optimizer step, train_ablation.py:107-210) on a fixed batch
    size, captured once as a HIP graph (torch.cuda.graph) and replayed per
    batch: the step's ~100 small launches (loss terms, FV updates, Poisson,
    FluxGNN forward/backward kernels, Adam) become one graph launch.  The
    batch indices are a static device tensor gathered inside the graph.  The
    optimizer must be capturable (torch.optim.Adam(..., capturable=True)).
    The warmup steps that precede the capture are ordinary eager steps on the
    first batches, so a pass makes exactly the eager loop's updates."""

    def __init__(self, model, opt, data, batch_size, x, dt, dx, cfg, grid, direct=True, graph_radius=1):
        self.args = (model, opt, data, x, dt, dx, cfg, grid)
        self.graph_radius = graph_radius
        self.direct = direct  # direct_step where it applies
        dev = data.state_t.device
        self.idx = torch.zeros(batch_size, dtype=torch.long, device=dev)
        self.graph = None
        self.out = None

    def _body(self):
        model, opt, data, x, dt, dx, cfg, grid = self.args
        st, ft, sn, nf = data.batch(self.idx, x, check=False)  # (train_steps checked the order)
        if self.direct:
            r = direct_step(model, opt, st, ft, sn, nf, x, dt, dx, cfg, grid, self.graph_radius)
            if r is not None:
                return r
        loss, flux_loss = ablation_loss(model, st, ft, sn, x, dt, dx, cfg, grid, nf=nf, graph_radius=self.graph_radius)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.detach(), flux_loss.detach()

    def capture(self):
        self.args[1].zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._body()

    def __call__(self, idx):
        """Step on batch idx (a device index tensor of the captured size):
        (loss, flux_loss) as fresh device scalars."""
        self.idx.copy_(idx)
        if self.graph is None:
            return self._body()
        self.graph.replay()
        # the replayed optimizer step changed the parameters without a host-side
        # in-place op: bump their versions (FluxGNN.device_model keys on them)
        torch.autograd.graph.increment_version(list(self.args[0].parameters()))
        return self.out[0].clone(), self.out[1].clone()


def train_steps(model, opt, data, order, batch_size, x, dt, dx, cfg, grid, graphed=None, warmup=3, direct=True,
                stats=None, graph_radius=1):
    """One pass over `order` (sample indices) in batches; returns (sum of
    losses, sum of flux losses) weighted by batch size, and the step count.
    graphed: a GraphedStep of this batch size (created by the caller and kept
    across passes); its first `warmup` steps run eagerly on a side stream, then
    it is captured and every further full batch replays the graph.  direct:
    eager steps take direct_step where it applies (the same parameters bit for
    bit as the autograd step).  stats: the trainer's _StepStats; with a guarded
    FlatAdam the sums then run over the steps that were applied (stats.weight
    samples).  graph_radius: ablation_loss's (a GraphedStep carries its own)."""
    tot, tot_flux, steps = 0.0, 0.0, 0
    losses = []
    data.check_indices(order)  # once per pass; the steps gather with check=False
    for b0 in range(0, len(order), batch_size):
        idx = order[b0:b0 + batch_size]
        if graphed is not None and len(idx) == batch_size:
            if graphed.graph is None and getattr(graphed, "_warm", 0) >= warmup:
                torch.cuda.synchronize()
                graphed.capture()
            if graphed.graph is None:
                graphed._warm = getattr(graphed, "_warm", 0) + 1
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    loss, flux_loss = graphed(idx)
                torch.cuda.current_stream().wait_stream(side)
            else:
                loss, flux_loss = graphed(idx)
        else:
            st, ft, sn, nf = data.batch(idx, x, check=False)
            r = direct_step(model, opt, st, ft, sn, nf, x, dt, dx, cfg, grid, graph_radius) if direct else None
            if r is not None:
                loss, flux_loss = r
            else:
                loss, flux_loss = ablation_loss(model, st, ft, sn, x, dt, dx, cfg, grid, nf=nf,
                                                graph_radius=graph_radius)
                opt.zero_grad()
                loss.backward()
                opt.step()
                loss, flux_loss = loss.detach(), flux_loss.detach()
        losses.append((loss, flux_loss, len(idx)))
        if stats is not None:
            stats.note(len(idx))
        steps += 1
    if stats:
        losses = [row for row, a in zip(losses, stats.read()) if a]
    for l, f, n in losses:  # one host sync per pass, not per step
        tot += float(l) * n
        tot_flux += float(f) * n
    return tot, tot_flux, steps


def train_model(state_t, flux_t, state_next, x, dt, dx, nu, config_name, stencil_radius, epochs=20, lr=1e-3,
                device="cuda", batch_size=1, seed=None, save_dir="checkpoints", log=print, weight_decay=0.0,
                max_grad_norm=None, skip_nonfinite=False, scheduler=None, graph_radius=1):
    """scripts/training/train_ablation.py:64-237 on the MI355X.  Returns
    (model, history) and writes checkpoints/hybrid_<config>_r<radius>.pt and
    history_<config>_r<radius>.json like the reference (save_dir=None skips).
    weight_decay, max_grad_norm, skip_nonfinite: FlatAdam's guard options;
    scheduler: a callable opt -> torch.optim.lr_scheduler.LRScheduler, stepped
    once per epoch.  With max_grad_norm or skip_nonfinite the history gains
    grad_norm_max and skipped_steps per epoch, and the epoch's losses are means
    over the samples of the steps that were applied.
    stencil_radius names the checkpoint, as in the reference, whose graph is
    always the ±1 chain.  graph_radius (1..3) is the real one: beyond 1 the
    model trains on the radius chain graph (ablation_loss), to be rolled out by
    HybridSolver(path, stencil_radius, graph_radius=graph_radius).  The
    checkpoint's name, keys and shapes do not depend on it."""
    cfg = ABLATION_CONFIGS[config_name]
    if int(graph_radius) != graph_radius or not 1 <= graph_radius <= 3:
        raise ValueError(f"graph_radius must be 1, 2 or 3, got {graph_radius!r}")
    engine.require_device(torch.empty(0, device=device), "device")
    if seed is not None:
        torch.manual_seed(seed)
    data = FluxDataset(state_t, flux_t, state_next, device)
    grid = BaselineSolver(nx=data.nx, dt=dt, nu=nu, device=device).grid
    x_dev = torch.as_tensor(np.asarray(x, dtype=np.float32), device=device)
    model = FluxGNN(MODEL_CONFIG["input_dim"], MODEL_CONFIG["hidden_dim"], MODEL_CONFIG["num_layers"]).to(device)
    model.flatten_parameters_()  # one parameter buffer: no per-step concat in the training forward
    # torch.optim.Adam's update (:82), one launch per step
    opt, sched = _guarded_optimizer(model.parameters(), lr, weight_decay, max_grad_norm, skip_nonfinite, scheduler,
                                    device)
    gen = torch.Generator().manual_seed(0 if seed is None else seed)
    history = {"epoch": [], "loss": [], "flux_loss": [], "seconds": []}
    stats = _StepStats(opt, history)
    model.train()
    for epoch in range(1, epochs + 1):
        order = torch.randperm(len(data), generator=gen).to(device)
        t0 = time.perf_counter()
        tot, tot_flux, _ = train_steps(model, opt, data, order, batch_size, x_dev, dt, dx, cfg, grid, stats=stats,
                                       graph_radius=int(graph_radius))
        count = stats.weight if stats else len(data)
        torch.cuda.synchronize(device)
        if sched is not None:
            sched.step()
        history["epoch"].append(epoch)
        history["loss"].append(tot / count if count else float("nan"))
        history["flux_loss"].append(tot_flux / count if count else float("nan"))
        history["seconds"].append(time.perf_counter() - t0)
        if log:
            log(f"[Epoch {epoch}/{epochs}] Loss: {history['loss'][-1]:.6e}, Flux: {history['flux_loss'][-1]:.6e}")
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        # (cloned: one storage per tensor, as the reference's checkpoints, not views of the flat buffer)
        torch.save({k: v.clone() for k, v in model.state_dict().items()}, os.path.join(save_dir, f"hybrid_{config_name}_r{stencil_radius}.pt"))
        with open(os.path.join(save_dir, f"history_{config_name}_r{stencil_radius}.json"), "w") as f:
            json.dump(history, f, indent=2)
    return model, history


# ----------------------------------------------------------------- PureGNN
class _StateMSE(torch.autograd.Function):
    """The PureGNN trainer's loss and its gradient as one HIP pass (hf_state_mse)."""

    @staticmethod
    def forward(ctx, delta, state_t, state_next):
        loss, gd = engine.state_mse(delta, state_t, state_next)
        ctx.save_for_backward(gd)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (gd,) = ctx.saved_tensors
        return gd * g, None, None


def state_mse_loss(delta, state_t, state_next):
    """mean((state_t^T + delta - state_next^T)^2) for delta [B*nx,3] and states
    [B,3,nx]: the reference's batch loss (train_pure_gnn.py:134-141, the mean
    over samples of per-sample means, every sample having 3 nx values),
    differentiable in delta."""
    return _StateMSE.apply(delta, state_t, state_next)


def pure_gnn_features(state_t, x):
    """[B,3,nx] states and x [nx] -> node features [B*nx,4] = [n, u, E, x]
    (train_pure_gnn.py:125-128, batched)."""
    B, _, nx = state_t.shape
    return torch.cat([state_t.permute(0, 2, 1).reshape(B * nx, 3), x.repeat(B).unsqueeze(1)], dim=1)


def pure_gnn_step(model, opt, state_t, state_next, x):
    """One optimizer step of the reference's loop (train_pure_gnn.py:112-145) on
    a batch [B,3,nx]: ONE forward and backward over the batch's B disjoint
    chains (a tagged chain_edge_index) instead of B per-sample graph calls, the
    fused loss, opt.step().  Returns the detached loss (no host sync)."""
    from .graph_constructor import chain_edge_index
    B, _, nx = state_t.shape
    delta = model(pure_gnn_features(state_t, x), chain_edge_index(nx, B, state_t.device))
    loss = state_mse_loss(delta, state_t, state_next)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach()


def pure_gnn_train_flop_per_sample(nx=64, H=128, L=4, F=4):
    """Algorithmic FLOPs of one sample of the PureGNN training step (P/Q-split
    messages, as train_flop_per_sample counts FluxGNN's): forward GEMMs once
    (input 2FH, layers L*2*H*2H, output_mlp 2HH + 2*3H per cell), backward data
    gradients once (the same layer and output_mlp sizes; none into the node
    features) and weight gradients once (the same, plus the input layer's
    2FH).  tanh, the message sums and the loss are not counted."""
    gemm = L * 2 * H * 2 * H + 2 * H * H + 2 * 3 * H
    return (2 * F * H + gemm + gemm + gemm + 2 * F * H) * nx


def _stage_states(state_t, state_next, device):
    """state_t / state_next of a one-step trainer as float32 [N,3,nx] on the device."""
    st_all = torch.as_tensor(np.asarray(state_t, dtype=np.float32), device=device)
    sn_all = torch.as_tensor(np.asarray(state_next, dtype=np.float32), device=device)
    if st_all.dim() != 3 or st_all.shape[1] != 3 or sn_all.shape != st_all.shape or st_all.shape[0] < 1:
        raise ValueError(f"state_t / state_next must be [N,3,nx] with N >= 1, got {tuple(st_all.shape)}, "
                         f"{tuple(sn_all.shape)}")
    return st_all, sn_all


def train_pure_gnn(state_t, state_next, x, epochs=50, lr=1e-3, batch_size=32, hidden_dim=None, num_layers=None,
                   device="cuda", order=None, seed=None, log=None, weight_decay=0.0, max_grad_norm=None,
                   skip_nonfinite=False, scheduler=None):
    """scripts/training/train_pure_gnn.py:79-151 on the MI355X: PureGNN(4,
    hidden_dim, num_layers) (default MODEL_CONFIG's, :94-98), Adam(lr), batches
    of batch_size samples in a shuffled order (the last one may be partial),
    the epoch's history entry the mean of its batch losses (:147-150).  Each
    batch is one batched step (pure_gnn_step).  order: per epoch an explicit
    sample order (a sequence of `epochs` index sequences) instead of the
    shuffle.  Returns (model, {'loss': [...]}).  weight_decay, max_grad_norm,
    skip_nonfinite, scheduler: as train_model's (the mean then runs over the
    batches whose step was applied)."""
    engine.require_device(torch.empty(0, device=device), "device")
    if seed is not None:
        torch.manual_seed(seed)
    st_all, sn_all = _stage_states(state_t, state_next, device)
    n = st_all.shape[0]
    x_dev = torch.as_tensor(np.asarray(x, dtype=np.float32), device=device)
    model = PureGNN(MODEL_CONFIG["input_dim"], hidden_dim or MODEL_CONFIG["hidden_dim"],
                    MODEL_CONFIG["num_layers"] if num_layers is None else num_layers).to(device)
    model.flatten_parameters_()
    opt, sched = _guarded_optimizer(model.parameters(), lr, weight_decay, max_grad_norm, skip_nonfinite, scheduler,
                                    device)
    gen = torch.Generator().manual_seed(0 if seed is None else seed)
    history = {"loss": []}
    stats = _StepStats(opt, history)
    model.train()
    for epoch in range(epochs):
        perm = torch.randperm(n, generator=gen) if order is None else torch.as_tensor(order[epoch], dtype=torch.int64)
        if perm.numel() and (int(perm.min()) < -n or int(perm.max()) >= n):
            raise IndexError(f"sample index out of range for a dataset of {n} samples")
        perm = perm.to(device)
        total, nb, each = torch.zeros((), device=device), 0, []
        for k in range(0, perm.numel(), batch_size):
            idx = perm[k:k + batch_size]
            loss = pure_gnn_step(model, opt, st_all[idx], sn_all[idx], x_dev)
            if stats:
                each.append(loss)
                stats.note()
            else:
                total += loss
            nb += 1
        if stats:
            history["loss"].append(_applied_mean(each, stats.read()))
        else:
            history["loss"].append(float(total) / max(nb, 1))
        if sched is not None:
            sched.step()
        if log:
            log(f"Epoch {epoch + 1}/{epochs}, Loss: {history['loss'][-1]:.6f}")
    return model, history


def _applied_mean(values, applied):
    """The mean of the device values (scalars or vectors of one size) of the
    steps that were applied, read in one transfer; NaN when none was."""
    rows = torch.stack(values).tolist() if values else []
    rows = [r for r, a in zip(rows, applied) if a]
    if not rows:
        return float("nan")
    if isinstance(rows[0], list):
        return [sum(col) / len(rows) for col in zip(*rows)]
    return sum(rows) / len(rows)


# -------------------------------------------------------- unrolled training
# Both rollout models differentiated through K steps of the loop they are
# scored on, so that the loss sees the feedback the one-step losses above never
# do.  FluxGNN through K hybrid solver steps (include/hybridflux.h,
# hf_unroll_update / hf_unroll_adjoint): n -> E -> u -> node features, as the
# evaluation rollouts run it.  PureGNN through K steps of its own rollout state
# <- state + PureGNN([n, u, E, x]) (evaluate_multi_ic.py:53-64;
# hf_pure_unroll_update / hf_pure_unroll_adjoint).  One driver runs both; a
# _Rollout says where they differ.
def _flux_adjoint(grid, tr, pred, k, weights, scale, direct, gnf, keep, coef=None):
    g_fe, direct = engine.unroll_adjoint(grid, tr[0] if k == 0 else pred[k - 1], pred[k], tr[k + 1], weights, scale,
                                         direct, gnf, want_direct=keep, cons_coef=coef)
    return g_fe.reshape(-1), direct


def _pure_update(grid, *args, **kwargs):
    return engine.pure_unroll_update(*args, **kwargs)


def _pure_adjoint(grid, tr, pred, k, weights, scale, gd, gnf, keep, coef=None):
    # dL/ds_{k+1} transposed is dL/ddelta_k: the seed of s_{k+1}, what reached s_{k+2} (the
    # residual update is the identity in the state) and step k+1's feature gradient
    gd = engine.pure_unroll_adjoint(pred[k], tr[k + 1], weights, scale, gd, gnf, cons_coef=coef)
    return gd, gd


class _Rollout(NamedTuple):
    """Where K-step training of one model differs from the other's."""
    model_cls: type
    loss_name: str       # the public loss function, for the TypeError
    input_dim: Optional[int]  # the rollout's node features need this width (None: the kernels check)
    features: Callable   # (state [B,3,nx], x) -> node features of the first step
    forward: Callable    # engine.*_forward_train
    backward: Callable   # engine.*_backward
    workspace: Callable  # (B, nx, dev) -> scratch of update
    update: Callable     # (grid, model output, state, x, target, weights, scale, want_nf=, out=, loss=, ws=); with
    #                      the conservation terms also cons=, cons_scale=, cons_ref=, cons_coef= (the _ex call)
    adjoint: Callable    # (grid, tr, pred, k, weights, scale, carry, gnf, keep, coef=) -> (the model backward's
    #                      incoming gradient, carry): step k's, from step k+1's carry and feature gradient
    log_label: str
    checkpoint: str      # <checkpoint>_K<K>.pt
    history: str         # <history>_K<K>.json
    graph: bool = True   # False (PINN): no edge index and no x, the model maps the flattened state to the next
    #                      state itself (forward(..., out=pred[k])), `grid` carries the loss's own constants
    terms: int = 1       # values of a step's loss row, the first one the step's term of L
    direct_ok: Optional[Callable] = None  # (model, opt) -> the direct step applies (default: FlatAdam on exactly
    #                                       the model's parameters, grad enabled)
    workspace_ex: Optional[Callable] = None  # the conservation terms' one hook: (B, nx, dev) -> scratch of the _ex
    #                                          update; its loss row is `terms` values (at least 2) + (energy, charge)


_FLUX = _Rollout(FluxGNN, "unrolled_loss", None, lambda st, x: build_chain_graph_batch(st, x)[0],
                 engine.graph_forward_train, engine.graph_backward, engine.unroll_workspace, engine.unroll_update,
                 _flux_adjoint, "Unrolled loss", "hybrid_unrolled", "history_unrolled",
                 workspace_ex=engine.unroll_workspace_ex)
_PURE = _Rollout(PureGNN, "pure_unrolled_loss", 4, pure_gnn_features,
                 engine.pure_gnn_forward_train, engine.pure_gnn_backward, engine.pure_unroll_workspace, _pure_update,
                 _pure_adjoint, "PureGNN unrolled loss", "pure_gnn_unrolled", "history_pure_gnn_unrolled",
                 workspace_ex=engine.pure_unroll_workspace_ex)


class _Cons(NamedTuple):
    """The energy and charge terms of a K-step loss: lam = (lam_e, lam_q), ref "target", "start" or [B,K,2] float64."""
    lam: tuple
    ref: object


def _conservation(conservation, conservation_ref, trainer=False):
    """The public conservation / conservation_ref arguments as a _Cons (None: no terms)."""
    if conservation is None:
        if not (isinstance(conservation_ref, str) and conservation_ref == "target"):
            raise ValueError("conservation_ref belongs to the energy and charge terms: pass conservation with it")
        return None
    lam = tuple(float(v) for v in conservation)
    if len(lam) != 2 or not all(v >= 0 for v in lam):
        raise ValueError("conservation must be (lam_e, lam_q), both >= 0")
    if isinstance(conservation_ref, str):
        if conservation_ref not in ("target", "start"):
            raise ValueError(f'conservation_ref must be "target", "start" or a [B,K,2] tensor, got {conservation_ref!r}')
    elif trainer:
        raise ValueError('a trainer takes conservation_ref "target" or "start"')
    elif not isinstance(conservation_ref, torch.Tensor):
        raise ValueError('conservation_ref must be "target", "start" or a float64 [B,K,2] tensor')
    return _Cons(lam, conservation_ref)


def _cons_refs(cons, tr):
    """The steps' references [K,B,2] float64 (step k's rows contiguous) for the
    window tr [K+1,B,3,nx]: one hf_state_moments launch over the whole window,
    every step's reference a view of its output -- "target": (e, q) of s*_k,
    "start": of s*_0 for every step; a [B,K,2] tensor: as given."""
    K, B = tr.shape[0] - 1, tr.shape[1]
    if isinstance(cons.ref, str):
        mom = engine.state_moments(tr)
        return mom[1:] if cons.ref == "target" else mom[:1].expand(K, B, 2)
    ref = cons.ref
    if ref.dtype != torch.float64 or tuple(ref.shape) != (B, K, 2) or ref.device != tr.device:
        raise ValueError(f"conservation_ref must be float64 [{B},{K},2] on {tr.device}, got {tuple(ref.shape)} "
                         f"{ref.dtype}")
    return ref.detach().transpose(0, 1).contiguous()


def _rollout_forward(m, flat, dims, traj, x, grid, weights, cons=None):
    """The K taped forwards and updates.  Returns (loss [] , rec): rec holds
    what the backward needs and the predicted states `pred` [K,B,3,nx].  cons
    (a _Cons): the updates are the _ex calls, which add the energy and charge
    terms and leave the adjoints' coefficients in rec["coef"] [K,B,2]."""
    B, K1, _, nx = traj.shape
    K = K1 - 1
    dev = traj.device
    tr = traj.detach().to(torch.float32).transpose(0, 1).contiguous()  # [K+1,B,3,nx]: a step's rows contiguous
    ei = shared_chain_edge_index(nx, B, dev) if m.graph else None
    scale = 1.0 / (K * 3 * B * nx)
    pred = torch.empty(K, B, 3, nx, device=dev)
    if cons is None:
        terms = torch.empty(K, device=dev) if m.terms == 1 else torch.empty(K, m.terms, device=dev)
        ws = m.workspace(B, nx, dev)
        refs = coef = None
    else:
        terms = torch.empty(K, max(m.terms, 2) + 2, device=dev)
        ws = m.workspace_ex(B, nx, dev)
        refs, coef = _cons_refs(cons, tr), torch.empty(K, B, 2, device=dev)
    st = tr[0]
    nf = m.features(st, x)
    forward, update = m.forward, m.update
    tapes, nfs, chain_nx = [], [], 0
    for k in range(K):
        if m.graph:
            y, tape, nf_d, ei_d, chain_nx = forward(flat, dims, nf, ei)
        else:
            y, tape, nf_d, ei_d, chain_nx = forward(flat, dims, nf, ei, out=pred[k])
        ckw = {} if cons is None else dict(cons=cons.lam, cons_scale=1.0 / (K * B), cons_ref=refs[k], cons_coef=coef[k])
        _, nf, _ = update(grid, y, st, x, tr[k + 1], weights, scale, want_nf=k + 1 < K, out=pred[k],
                          loss=terms[k:k + 1] if terms.dim() == 1 else terms[k], ws=ws, **ckw)
        tapes.append(tape)
        nfs.append(nf_d)
        st = pred[k]
    rec = dict(tr=tr, pred=pred, tapes=tapes, nfs=nfs, ei=ei_d, chain_nx=chain_nx, scale=scale, K=K, terms=terms,
               coef=coef)
    return (terms.sum() if terms.dim() == 1 else terms[:, 0].sum()), rec


def _rollout_backward(m, flat, dims, rec, grid, weights, through_state):
    """The K adjoint / model-backward pairs, last step first; the parameter
    gradients of the steps are added in that order (K-1, K-2, ..., 0).
    Returns d loss / d params as one flat buffer."""
    tr, pred, K, scale = rec["tr"], rec["pred"], rec["K"], rec["scale"]
    nfs, ei, chain_nx, tapes = rec["nfs"], rec["ei"], rec["chain_nx"], rec["tapes"]
    adjoint, backward, coef = m.adjoint, m.backward, rec["coef"]
    total, carry, gnf = None, None, None
    for k in range(K - 1, -1, -1):
        keep = through_state and k > 0  # step k's state gradient feeds step k-1
        ckw = {} if coef is None else dict(coef=coef[k])
        g, carry = adjoint(grid, tr, pred, k, weights, scale, carry if through_state else None, gnf, keep, **ckw)
        gp, gnf = backward(flat, dims, nfs[k], ei, chain_nx, tapes[k], g, keep)
        total = gp if total is None else total.add_(gp)
    return total


def _rollout_check(m, model, traj, x, grid):
    """The model, traj and x of a K-step loss; with a grid nx is the grid's,
    without one (PureGNN) any.  Returns x [nx] float32 on traj's device."""
    if type(model) is not m.model_cls:
        raise TypeError(f"{m.loss_name} trains {m.model_cls.__name__}")
    if m.input_dim is not None and model.input_dim != m.input_dim:
        raise ValueError(f"the rollout builds [n,u,E,x] node features: input_dim must be {m.input_dim}")
    engine.require_device(traj, "traj")
    if not m.graph:  # PINN: no x, nx the model's
        if traj.dim() != 4 or traj.shape[0] < 1 or traj.shape[1] < 2 or traj.shape[2] != 3 \
                or 3 * traj.shape[3] != model.input_dim:
            raise ValueError(f"traj must be [B,K+1,3,nx] with B >= 1, K >= 1, 3 nx = {model.input_dim}, got "
                             f"{tuple(traj.shape)}")
        return None
    want = f"[B,K+1,3,{grid.nx}] with B >= 1, K >= 1" if grid is not None else \
        "[B,K+1,3,nx] with B >= 1, K >= 1, nx >= 1"
    if traj.dim() != 4 or traj.shape[1] < 2 or traj.shape[2] != 3 or traj.shape[0] < 1 \
            or (traj.shape[3] != grid.nx if grid is not None else traj.shape[3] < 1):
        raise ValueError(f"traj must be {want}, got {tuple(traj.shape)}")
    x = torch.as_tensor(x, dtype=torch.float32, device=traj.device).reshape(-1).contiguous()
    if x.numel() != traj.shape[3]:
        raise ValueError("x must hold nx positions")
    return x


class _RolloutLoss(torch.autograd.Function):
    """A K-step loss as one Function: forward = K taped model forwards and
    updates, backward = K adjoint / model-backward pairs."""

    @staticmethod
    def forward(ctx, m, traj, x, grid, weights, through_state, dims, cons, *params):
        flat, _ = flat_params(params, traj.device)
        loss, rec = _rollout_forward(m, flat, dims, traj, x, grid, weights, cons)
        ctx.m, ctx.rec, ctx.flat, ctx.grid, ctx.weights, ctx.through, ctx.dims = \
            m, rec, flat, grid, weights, through_state, dims
        ctx.shapes = [q.shape for q in params]
        ctx.param_devices = [q.device for q in params]
        ctx.mark_non_differentiable(rec["pred"], rec["terms"])
        return loss, rec["pred"], rec["terms"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_pred, g_terms):
        gp = _rollout_backward(ctx.m, ctx.flat, ctx.dims, ctx.rec, ctx.grid, ctx.weights, ctx.through)
        ctx.rec = None  # the tapes are consumed
        gp = gp.mul_(g_loss)  # (exact for autograd's seed 1)
        return (None, None, None, None, None, None, None, None, *split_flat(gp, ctx.shapes, ctx.param_devices))


def _rollout_loss(m, model, traj, x, grid, channel_weights, through_state, return_states=False, cons=None):
    x = _rollout_check(m, model, traj, x, grid)
    dims = (model.input_dim, model.hidden_dim, model.num_layers)
    w = tuple(float(v) for v in channel_weights)
    loss, pred, terms = _RolloutLoss.apply(m, traj, x, grid, w, bool(through_state), dims, cons, *model.parameters())
    if not return_states:
        return loss
    return (loss, pred) if terms.dim() == 1 else (loss, pred, terms)


def _rollout_step(m, model, opt, traj, x, grid, channel_weights, through_state, cons=None, terms_out=None):
    """terms_out: a list that receives the step's loss rows [K, terms] (the trainers' energy and charge history)."""
    if m.direct_ok is not None:
        if not m.direct_ok(model, opt):
            return None
    elif type(model) is not m.model_cls or not isinstance(opt, FlatAdam) or not torch.is_grad_enabled():
        return None
    params = list(model.parameters())
    if not drives_exactly(opt, params):
        return None
    flat = flat_view(params, traj.device)
    if flat is None:
        return None
    x = _rollout_check(m, model, traj, x, grid)
    dims = (model.input_dim, model.hidden_dim, model.num_layers)
    w = tuple(float(v) for v in channel_weights)
    loss, rec = _rollout_forward(m, flat, dims, traj, x, grid, w, cons)
    gp = _rollout_backward(m, flat, dims, rec, grid, w, bool(through_state))
    assign_grads(params, gp)
    opt.step()
    if terms_out is not None:
        terms_out.append(rec["terms"])
    return loss.detach()


def _train_windows(m, model, data, x, grid, init, epochs, lr, batch_size, seed, channel_weights, through_state,
                   device, save_dir, log, guard=(0.0, None, False, None), cons=None, noise=None, noise_seed=0):
    """The K-step trainers' loop: Adam(lr) over shuffled batches of batch_size
    windows of data (a WindowDataset), one direct step each (the autograd step
    where that does not apply), one host sync per epoch.  model: the freshly
    initialised host model; init: a state dict to load into it first.  guard:
    (weight_decay, max_grad_norm, skip_nonfinite, scheduler) as train_model's;
    with clipping or skipping on the epoch's loss is the mean over the windows
    of the steps that were applied, and the history gains grad_norm_max and
    skipped_steps.  cons (a _Cons): the energy and charge terms are on, and the
    history gains energy_loss and charge_loss, the epoch's means of the two
    terms' values, weighted as loss.  noise (a StateNoise): every window starts
    from its perturbed first state (WindowDataset.batch); once per epoch one
    seed per sample is drawn from a generator of its own seeded with noise_seed
    (the shuffle's order does not change) and indexed by sample on the device,
    and the history gains noise, the sigmas."""
    K = data.K
    x_dev = torch.as_tensor(np.asarray(x, dtype=np.float32), device=device) if x is not None else None
    if init is not None:
        model.load_state_dict({k: torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v
                               for k, v in init.items()})
    model = model.to(device)
    model.flatten_parameters_()
    opt, sched = _guarded_optimizer(model.parameters(), lr, *guard, device)
    gen = torch.Generator().manual_seed(0 if seed is None else seed)
    history = {"epoch": [], "loss": [], "seconds": []}
    if noise is not None:
        noise_gen = torch.Generator().manual_seed(noise_seed)
        history["noise"] = [float(v) for v in noise.sigma]
    if cons is not None:
        history["energy_loss"], history["charge_loss"] = [], []
    stats = _StepStats(opt, history)
    model.train()
    for epoch in range(1, epochs + 1):
        order = torch.randperm(len(data), generator=gen).to(device)
        if noise is not None:
            seeds = torch.randint(0, 2 ** 32, (len(data),), dtype=torch.int64, generator=noise_gen).to(device)
        t0 = time.perf_counter()
        losses = []
        rows = [] if cons is not None else None  # the steps' loss rows [K, terms]
        for b0 in range(0, len(order), batch_size):
            idx = order[b0:b0 + batch_size]
            win = data.batch(idx) if noise is None else data.batch(idx, noise, seeds[idx])
            loss = _rollout_step(m, model, opt, win, x_dev, grid, channel_weights, through_state, cons, rows)
            if loss is None:
                if cons is None:
                    loss = _rollout_loss(m, model, win, x_dev, grid, channel_weights, through_state)
                else:
                    loss, _, terms = _rollout_loss(m, model, win, x_dev, grid, channel_weights, through_state, True, cons)
                    rows.append(terms)
                opt.zero_grad()
                loss.backward()
                opt.step()
                loss = loss.detach()
            losses.append((loss, win.shape[0]))
            stats.note(win.shape[0])
        count = len(data)
        if rows is not None:
            rows = [(r[:, -2:].sum(0), n) for r, (_, n) in zip(rows, losses)]
        if stats:
            applied = stats.read()
            losses = [row for row, a in zip(losses, applied) if a]
            if rows is not None:
                rows = [row for row, a in zip(rows, applied) if a]
            count = stats.weight
        tot = sum(float(l) * n for l, n in losses)  # one host sync per epoch
        if rows is not None:
            ec = torch.stack([r for r, _ in rows]).tolist() if rows else []
            for j, key in enumerate(("energy_loss", "charge_loss")):
                history[key].append(sum(v[j] * n for v, (_, n) in zip(ec, rows)) / count if count else float("nan"))
        torch.cuda.synchronize(device)
        if sched is not None:
            sched.step()
        history["epoch"].append(epoch)
        history["loss"].append(tot / count if count else float("nan"))
        history["seconds"].append(time.perf_counter() - t0)
        if log:
            log(f"[Epoch {epoch}/{epochs}] {m.log_label} (K = {K}): {history['loss'][-1]:.6e}")
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        # (cloned: one storage per tensor, not views of the flat buffer)
        torch.save({k: v.clone() for k, v in model.state_dict().items()},
                   os.path.join(save_dir, f"{m.checkpoint}_K{K}.pt"))
        with open(os.path.join(save_dir, f"{m.history}_K{K}.json"), "w") as f:
            json.dump(history, f, indent=2)
    return model, history


def _radius_one_only(what, graph_radius):
    if graph_radius != 1:
        raise ValueError(f"{what}: unrolled training runs on the ±1 chain only (graph_radius = 1), got "
                         f"graph_radius = {graph_radius!r}; train a radius graph with train_model(graph_radius=...)")


def unrolled_loss(model, traj, x, grid, channel_weights=(1.0, 1.0, 1.0), through_state=True, return_states=False,
                  conservation=None, conservation_ref="target", graph_radius=1):
    """L = (1/K) sum_{k=1..K} mean_{b,ch,i} w_ch (s^_k - s*_k)^2 of the hybrid
    solver (src/hybrid_solver.py:45-63) unrolled K steps from traj[:, 0], against
    the targets traj[:, 1:] (classical solver states): traj [B,K+1,3,nx] on the
    device, x [nx], grid the engine.Grid of the step (spectral Poisson, nx <=
    6144).  A scalar with autograd into the model's parameters, through every
    step's FluxGNN call and, with through_state, through the state the steps hand
    on (continuity, velocity, the Poisson solve and the next node features).
    through_state=False cuts the state gradient between steps (the pushforward
    form): each step's loss reaches only its own FluxGNN call.  Per unrolled step
    the forward is hf_graph_forward_train + one hf_unroll_update launch, the
    backward one hf_unroll_adjoint launch + hf_graph_backward.  return_states:
    also the predicted states [K,B,3,nx] (no gradient).  conservation = (lam_e, lam_q) adds L_cons = (1/K) sum_k mean_b [ lam_e
    (e(s^_k)_b - eref_kb)^2 + lam_q (q(s^_k)_b - qref_kb)^2 ] with e = 0.5 (sum
    u^2 + sum E^2) / nx and q = sum n / nx (the energy and charge the evaluation
    scores), in float64, inside the same launches (the _ex calls of
    include/hybridflux.h) plus one hf_state_moments launch; conservation_ref:
    "target" (the reference of step k is the classical s*_k), "start" (s*_0 for
    every step: the drift the evaluation reports) or a float64 [B,K,2] tensor of
    (eref, qref).  None (the default): the calls and bits of the loss without the
    terms.  With conservation, return_states also returns the steps' rows
    [K,4] = (total, state, energy, charge).  The charge term has no gradient here
    (the finite-volume update conserves charge identically); its value is reported.
    graph_radius: 1 only (ValueError otherwise): the unrolled kernels know the ±1 chain."""
    _radius_one_only("unrolled_loss", graph_radius)
    return _rollout_loss(_FLUX, model, traj, x, grid, channel_weights, through_state, return_states,
                         _conservation(conservation, conservation_ref))


def unrolled_step(model, opt, traj, x, grid, channel_weights=(1.0, 1.0, 1.0), through_state=True, conservation=None,
                  conservation_ref="target", graph_radius=1):
    """unrolled_loss -> backward -> opt.step() without autograd, after
    direct_step: FluxGNN with flat parameters (flatten_parameters_), FlatAdam
    over exactly those parameters, grad enabled.  The same forwards, adjoints,
    backwards and gradient sum as the autograd step, in the same order, so the
    same parameters bit for bit, without autograd's seed, product and
    bookkeeping launches.  Returns the detached loss, or None when the case does
    not apply (the caller then takes the autograd step).  graph_radius: 1 only
    (ValueError otherwise)."""
    _radius_one_only("unrolled_step", graph_radius)
    return _rollout_step(_FLUX, model, opt, traj, x, grid, channel_weights, through_state,
                         _conservation(conservation, conservation_ref))


def unrolled_train_flop_per_sample(K=4, nx=64, H=128, L=4, F=4):
    """Algorithmic FLOPs of one sample (one K-step window) of the unrolled
    training step, after train_flop_per_sample: K FluxGNN forwards and K
    backwards (data + weight gradients), plus the input layer's data gradient
    2FH per cell for the K - 1 steps whose node features carry a gradient back
    to the previous step.  The hybrid updates, their adjoints and the Poisson
    solves (elementwise and float64 work outside the MFMA GEMMs) are not counted."""
    fwd = 2 * F * H + L * 2 * 2 * H * H + 2 * H * 2 * H + 2 * 2 * H
    bwd = (L * 2 * 2 * H * H + 2 * 2 * H * H) * 2 + 2 * F * H
    return (K * (fwd + bwd) + (K - 1) * 2 * F * H) * nx


class WindowDataset:
    """Device-resident K-step windows of classical trajectories [N,T+1,3,nx]:
    sample ic * (T - K + 1) + t0 is trajectories[ic, t0 : t0 + K + 1], for every
    (ic, t0) with t0 + K <= T."""

    def __init__(self, trajectories, K, device="cuda"):
        self.traj = torch.as_tensor(np.asarray(trajectories, dtype=np.float32), device=device) \
            if not isinstance(trajectories, torch.Tensor) else trajectories.to(device=device, dtype=torch.float32)
        if self.traj.dim() != 4 or self.traj.shape[2] != 3:
            raise ValueError(f"trajectories must be [N,T+1,3,nx], got {tuple(self.traj.shape)}")
        self.N, T1, _, self.nx = self.traj.shape
        self.K, self.T = int(K), T1 - 1
        if self.K < 1 or self.K > self.T:
            raise ValueError(f"need 1 <= K <= T (K = {K}, T = {self.T})")
        self.per_ic = self.T - self.K + 1
        self._steps = torch.arange(self.K + 1, device=self.traj.device)

    def __len__(self):
        return self.N * self.per_ic

    def batch(self, idx, noise=None, seeds=None):
        """Windows [B,K+1,3,nx] of the sample indices idx (each in [0, len)).
        noise (a StateNoise) with seeds (one per window of the batch): the
        window's first state is perturbed; rows 1..K, the targets, stay the
        clean classical states."""
        _noise_seeds(noise, seeds)
        idx = torch.as_tensor(idx, device=self.traj.device).to(torch.long).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError(f"sample index out of range for a dataset of {len(self)} windows")
        ic = torch.div(idx, self.per_ic, rounding_mode="floor")
        t0 = idx - ic * self.per_ic
        win = self.traj[ic[:, None], t0[:, None] + self._steps[None, :]]
        if noise is not None:
            win[:, 0] = noise.apply(win[:, 0].contiguous(), seeds)
        return win


def train_unrolled(trajectories, x, dt, dx, nu, K=4, epochs=10, lr=1e-3, batch_size=32, seed=None, init=None,
                   channel_weights=(1.0, 1.0, 1.0), through_state=True, device="cuda", save_dir="checkpoints",
                   log=print, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False, scheduler=None,
                   conservation=None, conservation_ref="target", graph_radius=1, noise=None, noise_seed=0):
    """Train (or fine-tune) FluxGNN on K-step windows of classical trajectories
    [N,T+1,3,nx] (datagen.generate_trajectories) with the unrolled loss: Adam(lr)
    over shuffled batches of batch_size windows, one unrolled_step each.  init:
    a reference state dict to start from (e.g. a one-step-trained checkpoint).
    Returns (model, history) with history keys epoch, loss (the mean over the
    epoch's windows), seconds, and writes checkpoints/hybrid_unrolled_K<K>.pt
    and history_unrolled_K<K>.json as train_model writes its files (save_dir=None
    skips).  weight_decay, max_grad_norm, skip_nonfinite, scheduler: as
    train_model's -- the guard that keeps one window whose rollout blows up from
    turning every parameter into NaN.  conservation = (lam_e, lam_q),
    conservation_ref "target" or "start": unrolled_loss's energy and charge
    terms; the history then also holds energy_loss and charge_loss.
    graph_radius: 1 only (ValueError otherwise).  noise (a StateNoise with
    sigma_E = 0), noise_seed: every window starts from its first state plus
    seeded Gaussian noise, E recomputed from the perturbed n on the step's grid,
    against the clean targets; one seed per sample and epoch from a generator
    seeded with noise_seed, apart from the shuffle's; the history then also holds
    noise, the sigmas.  None (the default): the calls and bits without it."""
    _radius_one_only("train_unrolled", graph_radius)
    cons = _conservation(conservation, conservation_ref, trainer=True)
    engine.require_device(torch.empty(0, device=device), "device")
    if seed is not None:
        torch.manual_seed(seed)
    data = WindowDataset(trajectories, K, device)
    grid = BaselineSolver(nx=data.nx, dt=dt, nu=nu, device=device).grid
    if abs(dt / dx - grid.dt / grid.dx) > 1e-12 * abs(dt / dx):
        raise ValueError(f"dx = {dx} is not the periodic grid's {grid.dx} for nx = {data.nx}")
    model = FluxGNN(MODEL_CONFIG["input_dim"], MODEL_CONFIG["hidden_dim"], MODEL_CONFIG["num_layers"])
    return _train_windows(_FLUX, model, data, x, grid, init, epochs, lr, batch_size, seed, channel_weights,
                          through_state, device, save_dir, log,
                          (weight_decay, max_grad_norm, skip_nonfinite, scheduler), cons,
                          None if noise is None else noise.with_grid(grid), noise_seed)


def pure_unrolled_loss(model, traj, x, channel_weights=(1.0, 1.0, 1.0), through_state=True, return_states=False,
                       conservation=None, conservation_ref="target"):
    """L = (1/K) sum_{k=1..K} mean_{b,ch,i} w_ch (s^_k - s*_k)^2 of PureGNN's own
    rollout s^_{k+1} = s^_k + PureGNN([n, u, E, x])^T (evaluate_multi_ic.py:53-64)
    unrolled K steps from traj[:, 0], against the targets traj[:, 1:] (classical
    solver states): traj [B,K+1,3,nx] on the device, x [nx]; any nx.  The same
    loss as unrolled_loss.  A scalar with autograd into the model's parameters,
    through every step's PureGNN call and, with through_state, through the state
    the steps hand on (the residual update and the next node features).
    through_state=False cuts the state gradient between steps (the pushforward
    form): each step's loss reaches only its own PureGNN call.  Per unrolled step
    the forward is hf_pure_gnn_forward_train + one hf_pure_unroll_update launch,
    the backward one hf_pure_unroll_adjoint launch + hf_pure_gnn_backward.
    model: a PureGNN with input_dim 4.  return_states: also the predicted states
    [K,B,3,nx] (no gradient).  conservation = (lam_e, lam_q) adds L_cons = (1/K) sum_k mean_b [ lam_e
    (e(s^_k)_b - eref_kb)^2 + lam_q (q(s^_k)_b - qref_kb)^2 ] with e = 0.5 (sum
    u^2 + sum E^2) / nx and q = sum n / nx (the energy and charge the evaluation
    scores), in float64, inside the same launches (the _ex calls of
    include/hybridflux.h) plus one hf_state_moments launch; conservation_ref:
    "target" (the reference of step k is the classical s*_k), "start" (s*_0 for
    every step: the drift the evaluation reports) or a float64 [B,K,2] tensor of
    (eref, qref).  None (the default): the calls and bits of the loss without the
    terms.  With conservation, return_states also returns the steps' rows
    [K,4] = (total, state, energy, charge)."""
    return _rollout_loss(_PURE, model, traj, x, None, channel_weights, through_state, return_states,
                         _conservation(conservation, conservation_ref))


def pure_unrolled_step(model, opt, traj, x, channel_weights=(1.0, 1.0, 1.0), through_state=True, conservation=None,
                       conservation_ref="target"):
    """pure_unrolled_loss -> backward -> opt.step() without autograd, after
    unrolled_step: PureGNN with flat parameters (flatten_parameters_), FlatAdam
    over exactly those parameters, grad enabled.  The same forwards, adjoints,
    backwards and gradient sum as the autograd step, in the same order, so the
    same parameters bit for bit, without autograd's seed, product and
    bookkeeping launches.  Returns the detached loss, or None when the case does
    not apply (the caller then takes the autograd step)."""
    return _rollout_step(_PURE, model, opt, traj, x, None, channel_weights, through_state,
                         _conservation(conservation, conservation_ref))


def pure_unrolled_train_flop_per_sample(K=4, nx=64, H=128, L=4, F=4):
    """Algorithmic FLOPs of one sample (one K-step window) of PureGNN's unrolled
    training step: K times the forward and backward terms of
    pure_gnn_train_flop_per_sample, plus the input layer's data gradient 2FH per
    cell for the K - 1 steps whose node features carry a gradient back to the
    previous step.  The residual updates, their adjoints and the loss
    (elementwise work outside the GEMMs) are not counted."""
    return K * pure_gnn_train_flop_per_sample(nx, H, L, F) + (K - 1) * 2 * F * H * nx


def train_pure_gnn_unrolled(trajectories, x, K=4, epochs=10, lr=1e-3, batch_size=32, hidden_dim=None, num_layers=None,
                            seed=None, init=None, channel_weights=(1.0, 1.0, 1.0), through_state=True, device="cuda",
                            save_dir="checkpoints", log=print, weight_decay=0.0, max_grad_norm=None,
                            skip_nonfinite=False, scheduler=None, conservation=None, conservation_ref="target",
                            noise=None, noise_seed=0):
    """Train (or fine-tune) PureGNN on K-step windows of classical trajectories
    [N,T+1,3,nx] (datagen.generate_trajectories) with the unrolled loss:
    train_unrolled's loop -- Adam(lr) over shuffled batches of batch_size windows
    (WindowDataset), one pure_unrolled_step each, one host sync per epoch -- on
    PureGNN(4, hidden_dim, num_layers) (default MODEL_CONFIG's, as
    train_pure_gnn).  seed also seeds the initial weights; init: a reference
    state dict to start from (e.g. a one-step-trained checkpoint).  Returns
    (model, history) with history keys epoch, loss (the mean over the epoch's
    windows), seconds, and writes checkpoints/pure_gnn_unrolled_K<K>.pt (a state
    dict the reference's PureGNN loads) and history_pure_gnn_unrolled_K<K>.json
    (save_dir=None skips).  weight_decay, max_grad_norm, skip_nonfinite,
    scheduler, conservation, conservation_ref, noise, noise_seed: as
    train_unrolled's, except that the StateNoise is used as given (its own
    sigma_E, or its own grid to recompute E)."""
    cons = _conservation(conservation, conservation_ref, trainer=True)
    engine.require_device(torch.empty(0, device=device), "device")
    if seed is not None:
        torch.manual_seed(seed)
    data = WindowDataset(trajectories, K, device)
    model = PureGNN(MODEL_CONFIG["input_dim"], hidden_dim or MODEL_CONFIG["hidden_dim"],
                    MODEL_CONFIG["num_layers"] if num_layers is None else num_layers)
    return _train_windows(_PURE, model, data, x, None, init, epochs, lr, batch_size, seed, channel_weights,
                          through_state, device, save_dir, log,
                          (weight_decay, max_grad_norm, skip_nonfinite, scheduler), cons, noise, noise_seed)


# --------------------------------------------------------------------- PINN
# scripts/training/train_pinn.py on the engine (pinn_train.hip).  PINN.forward
# stays the inference call (under autograd it raises); training goes through
# pinn_forward below, in the style of direct_step.
PINN_LOSS_WEIGHTS = (1.0, 0.1, 0.1, 0.01)  # (w_data, w_continuity, w_momentum, w_poisson), train_pinn.py:142-145


def _pinn_dims(model):
    return model.input_dim, model.hidden_dim, model.num_layers


class _PinnTrainForward(torch.autograd.Function):
    """state + net(state) with HIP backward kernels (hf_pinn_forward_train /
    hf_pinn_backward; parameter order = state dict), the counterpart of
    baselines._PureTrainForward."""

    @staticmethod
    def forward(ctx, state, dims, *params):
        dev = engine.compute_device(state, "state")
        flat, _ = flat_params(params, dev)
        s = state.detach().to(device=dev, dtype=torch.float32).reshape(-1, dims[0]).contiguous()
        out, tape = engine.pinn_forward_train(flat, dims, s)
        ctx.save_for_backward(flat, tape, s)
        ctx.dims = dims
        ctx.shapes = [q.shape for q in params]
        ctx.param_devices = [q.device for q in params]
        ctx.state_shape, ctx.state_dtype, ctx.state_device = state.shape, state.dtype, state.device
        return out.reshape(state.shape).to(state.device)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        flat, tape, s = ctx.saved_tensors
        gp, gs = engine.pinn_backward(flat, ctx.dims, s, tape, grad_out.reshape(-1, ctx.dims[0]),
                                      ctx.needs_input_grad[0])
        if gs is not None:
            gs = gs.reshape(ctx.state_shape).to(device=ctx.state_device, dtype=ctx.state_dtype)
        return (gs, None, *split_flat(gp, ctx.shapes, ctx.param_devices))


def pinn_forward(model, state):
    """PINN's training forward: state [..., 3, nx] -> state + net(state), the
    same shape, differentiable in the parameters and (when it requires grad)
    the state.  Gradients land on each tensor's own device; after
    model.flatten_parameters_() the kernels read the parameters in place."""
    if state.dim() < 2 or state.shape[-2] * state.shape[-1] != model.input_dim:
        raise ValueError(f"pinn_forward: state must be [..., 3, nx] with 3 nx = {model.input_dim}, got "
                         f"{tuple(state.shape)}")
    return _PinnTrainForward.apply(state, _pinn_dims(model), *model.parameters())


class _PinnLoss(torch.autograd.Function):
    """The PINN trainer's loss and its gradient as one HIP launch (hf_pinn_loss)."""

    @staticmethod
    def forward(ctx, pred, state_t, state_next, consts):
        dev = engine.compute_device(pred, "pred")
        dx, dt, nu, weights, length = consts
        losses, gp = engine.pinn_loss(pred.detach().to(dev), state_t, state_next, dx, dt, nu, weights, length)
        ctx.save_for_backward(gp)
        ctx.home = (pred.device, pred.dtype)
        terms = losses[1:].to(pred.device)
        ctx.mark_non_differentiable(terms)
        return losses[0].to(pred.device), terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        (gp,) = ctx.saved_tensors
        dev, dtype = ctx.home
        return (gp.to(device=dev, dtype=dtype) * g.to(dev)), None, None, None


def pinn_physics_loss(pred, state_t, state_next, dx, dt, nu, weights=PINN_LOSS_WEIGHTS, length=None):
    """The reference trainer's loss (train_pinn.py:163-175 with
    compute_physics_losses, :78-111) of pred = model's prediction from state_t
    against state_next, all [B,3,nx]: (loss, terms), loss = w . (data,
    continuity, momentum, poisson), terms the detached device tensor [4] of
    those.  Differentiable in pred only (the Poisson term included, as in the
    reference).  length: the domain length of the Poisson operator (default
    nx dx, the reference's fftfreq(nx, d=dx))."""
    return _PinnLoss.apply(pred, state_t, state_next, (float(dx), float(dt), float(nu), tuple(weights), length))


def _pinn_direct_ok(model, opt):
    """pinn_step's direct path applies: the optimizer drives exactly the
    model's parameters, no parameter has hooks, anomaly mode is off."""
    if type(model) is not PINN or not torch.is_grad_enabled() or torch.is_anomaly_enabled():
        return False
    params = list(model.parameters())
    if not drives_exactly(opt, params):
        return False
    return not any(getattr(q, "_backward_hooks", None) or getattr(q, "_post_accumulate_grad_hooks", None)
                   for q in params)


def pinn_step(model, opt, state_t, state_next, dx, dt, nu, weights=PINN_LOSS_WEIGHTS, length=None):
    """One optimizer step of the reference's loop (train_pinn.py:156-179) on a
    batch [B,3,nx] without an autograd graph: hf_pinn_forward_train,
    hf_pinn_loss, hf_pinn_backward with the loss's gradient as the incoming
    one, opt.step().  The gradient goes into the parameters' .grad, as pieces
    of one flat buffer (which FlatAdam on a flattened model reads in place).
    Returns the losses [5] = (loss, data, continuity, momentum, poisson) on
    the device; nothing synchronises the host, so with FlatAdam the step can
    be captured (GraphedPinnStep).  Parameter hooks are not run on this path:
    when a parameter has hooks, anomaly mode is on or the optimizer drives
    other parameters, the step is the autograd composition pinn_forward ->
    pinn_physics_loss -> backward() instead (the same arithmetic)."""
    params = list(model.parameters())
    if not _pinn_direct_ok(model, opt):
        pred = pinn_forward(model, state_t)
        loss, terms = pinn_physics_loss(pred, state_t, state_next, dx, dt, nu, weights, length)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return torch.cat([loss.detach().reshape(1), terms])
    dev = engine.compute_device(state_t, "state_t")
    dims = _pinn_dims(model)
    flat, home = flat_params(params, dev)
    st = state_t.detach().to(device=dev, dtype=torch.float32).contiguous()
    s2 = st.reshape(-1, dims[0])
    out, tape = engine.pinn_forward_train(flat, dims, s2)
    losses, gpred = engine.pinn_loss(out.reshape(st.shape), st, state_next, dx, dt, nu, weights, length)
    gp, _ = engine.pinn_backward(flat, dims, s2, tape, gpred.reshape(-1, dims[0]), False)
    assign_grads(params, gp, home)
    opt.step()
    return losses


class GraphedPinnStep(GraphedStep):
    """pinn_step on a fixed batch size, captured once as a HIP graph and
    replayed per batch (GraphedStep for the PINN trainer): the batch is copied
    into static device tensors, the losses [5] come back as a fresh tensor.
    Needs a flattened model and FlatAdam (a capturable optimizer); the steps
    before capture() are ordinary eager steps."""

    def __init__(self, model, opt, batch_shape, dx, dt, nu, weights=PINN_LOSS_WEIGHTS, length=None, device="cuda"):
        self.args = (model, opt, dx, dt, nu, weights, length)
        self.st = torch.zeros(batch_shape, device=device)
        self.sn = torch.zeros(batch_shape, device=device)
        self.graph = None
        self.out = None

    def _body(self):
        model, opt, dx, dt, nu, weights, length = self.args
        return pinn_step(model, opt, self.st, self.sn, dx, dt, nu, weights, length)

    def __call__(self, state_t, state_next):
        self.st.copy_(state_t)
        self.sn.copy_(state_next)
        if self.graph is None:
            return self._body()
        self.graph.replay()
        torch.autograd.graph.increment_version(list(self.args[0].parameters()))
        return self.out.clone()


def pinn_train_flop_per_sample(D=192, H=256, L=4):
    """Algorithmic FLOPs of one sample of the PINN training step: the forward
    GEMMs once (2 (DH + (L-2) HH + HD)), the weight gradients once (the same)
    and the data gradients of every layer but the first (none into the state).
    tanh, the loss and Adam are not counted."""
    fwd = 2 * (D * H + (L - 2) * H * H + H * D)
    return fwd + fwd + (fwd - 2 * D * H)


def train_pinn(state_t, state_next, dx, dt, nu, epochs=50, lr=1e-3, batch_size=32, hidden_dim=256, num_layers=4,
               weights=PINN_LOSS_WEIGHTS, seed=None, init=None, device=None, log=None, weight_decay=0.0,
               max_grad_norm=None, skip_nonfinite=False, scheduler=None):
    """scripts/training/train_pinn.py:114-201 on the MI355X: PINN(3 nx,
    hidden_dim, num_layers), Adam(lr), batches of batch_size samples in a
    shuffled order (the last one may be partial), one pinn_step per batch.
    init: a state dict to start from instead of the seeded initialisation.
    Returns (model, history) with the reference's history keys, each the
    per-epoch mean of its batch values (:187-197), accumulated on the device
    and read once per epoch.  model.state_dict() has the reference PINN's keys
    and shapes.  weight_decay, max_grad_norm, skip_nonfinite, scheduler: as
    train_model's (the means then run over the batches whose step was applied)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    engine.require_device(torch.empty(0, device=device), "device")
    if seed is not None:
        torch.manual_seed(seed)
    st_all, sn_all = _stage_states(state_t, state_next, device)
    n, _, nx = st_all.shape
    model = PINN(3 * nx, hidden_dim, num_layers)
    if init is not None:
        model.load_state_dict({k: torch.as_tensor(v) for k, v in init.items()})
    model = model.to(device).flatten_parameters_()
    opt, sched = _guarded_optimizer(model.parameters(), lr, weight_decay, max_grad_norm, skip_nonfinite, scheduler,
                                    device)
    gen = torch.Generator().manual_seed(0 if seed is None else seed)
    keys = ("loss", "loss_data", "loss_continuity", "loss_momentum", "loss_poisson")
    history = {k: [] for k in keys}
    stats = _StepStats(opt, history)
    model.train()
    for epoch in range(epochs):
        perm = torch.randperm(n, generator=gen).to(device)
        total, nb, each = torch.zeros(5, device=device), 0, []
        for k in range(0, n, batch_size):
            idx = perm[k:k + batch_size]
            losses = pinn_step(model, opt, st_all[idx], sn_all[idx], dx, dt, nu, weights)
            if stats:
                each.append(losses)
                stats.note()
            else:
                total += losses
            nb += 1
        if stats:
            mean = _applied_mean(each, stats.read())
            mean = mean if isinstance(mean, list) else [mean] * 5
        else:
            mean = (total / max(nb, 1)).tolist()  # the epoch's one host read
        if sched is not None:
            sched.step()
        for k, v in zip(keys, mean):
            history[k].append(v)
        if log:
            log(f"Epoch {epoch + 1}/{epochs}, Loss: {mean[0]:.6f} (data={mean[1]:.6f}, cont={mean[2]:.6f}, "
                f"mom={mean[3]:.6f}, pois={mean[4]:.6f})")
    return model, history


# ------------------------------------------------------- PINN, unrolled training
# PINN differentiated through K steps of its own rollout s^_k = s^_{k-1} +
# net(s^_{k-1}) (evaluate_multi_ic.py:70-83; hf_pinn_unroll_loss /
# hf_pinn_unroll_adjoint, pinn_unroll.hip), on the driver of the two graph
# models: the third _Rollout.  The `grid` slot carries the loss's constants.
class _PinnPhys(NamedTuple):
    """The residual terms of PINN's K-step loss: lam = (l_c, l_m, l_p) or None (state loss only)."""
    lam: Optional[tuple]
    dx: Optional[float]
    dt: Optional[float]
    nu: Optional[float]
    length: Optional[float]

    def kw(self, scale):
        # phys_scale = 1 / (K B nx) = 3 loss_scale
        return dict(phys=self.lam, phys_scale=3.0 * scale, dx=self.dx, dt=self.dt, nu=self.nu, length=self.length)


def _pinn_roll_forward(flat, dims, state, ei, out):
    B = state.shape[0]
    s2 = state.reshape(B, dims[0])
    y, tape = engine.pinn_forward_train(flat, dims, s2, out=out.view(B, dims[0]))
    return y, tape, s2, None, 0


def _pinn_roll_update(phys, y, st, x, target, weights, scale, want_nf, out, loss, ws, **cons):
    # the forward wrote s^_k into `out` itself; the next model input is that state
    engine.pinn_unroll_loss(out, target, weights, scale, state=st if phys.lam is not None else None, losses=loss,
                            ws=ws, **phys.kw(scale), **cons)
    return out, out, None


def _pinn_roll_adjoint(phys, tr, pred, k, weights, scale, carry, gstate, keep, coef=None):
    # gstate: hf_pinn_backward's dL/dstate of step k+1, there exactly when the state gradient passes (k < K-1)
    B, _, nx = pred[k].shape
    on = phys.lam is not None
    g = engine.pinn_unroll_adjoint(pred[k], tr[k + 1], weights, scale, state=(tr[0] if k == 0 else pred[k - 1]) if on
                                   else None, pred_next=pred[k + 1] if on and gstate is not None else None,
                                   grad_state_next=None if gstate is None else gstate.view(B, 3, nx), cons_coef=coef,
                                   **phys.kw(scale))
    return g.view(B, 3 * nx), None


def _pinn_roll_backward(flat, dims, state, ei, chain_nx, tape, g, keep):
    return engine.pinn_backward(flat, dims, state, tape, g, keep)


_PINN = _Rollout(PINN, "pinn_unrolled_loss", None, lambda st, x: st, _pinn_roll_forward, _pinn_roll_backward,
                 engine.pinn_unroll_workspace, _pinn_roll_update, _pinn_roll_adjoint, "PINN unrolled loss",
                 "pinn_unrolled", "history_pinn_unrolled", graph=False, terms=5, direct_ok=_pinn_direct_ok,
                 workspace_ex=engine.pinn_unroll_workspace_ex)


def _pinn_phys(physics_weights, dx, dt, nu, length):
    """dx, dt and nu are required exactly when physics_weights is given."""
    given = [v is not None for v in (dx, dt, nu)]
    if physics_weights is None:
        if any(given) or length is not None:
            raise ValueError("dx, dt, nu and length belong to the residual terms: pass physics_weights with them")
        return _PinnPhys(None, None, None, None, None)
    lam = tuple(float(v) for v in physics_weights)
    if len(lam) != 3:
        raise ValueError("physics_weights must be (l_continuity, l_momentum, l_poisson)")
    if not all(given):
        raise ValueError("physics_weights needs dx, dt and nu")
    return _PinnPhys(lam, float(dx), float(dt), float(nu), None if length is None else float(length))


def pinn_unrolled_loss(model, traj, dx=None, dt=None, nu=None, channel_weights=(1.0, 1.0, 1.0), physics_weights=None,
                       through_state=True, return_states=False, length=None, conservation=None,
                       conservation_ref="target"):
    """L = (1/K) sum_{k=1..K} [ mean_{b,ch,i} w_ch (s^_k - s*_k)^2 + l_c mean r_c^2 +
    l_m mean r_m^2 + l_p mean r_p^2 ] of PINN's own rollout s^_k = s^_{k-1} +
    net(s^_{k-1}) (evaluate_multi_ic.py:70-83) unrolled K steps from traj[:, 0]
    against the targets traj[:, 1:]: traj [B,K+1,3,nx] on the device, 3 nx the
    model's input_dim, nx <= 6144.  physics_weights None (the default): the state
    loss of unrolled_loss / pure_unrolled_loss alone.  physics_weights = (l_c,
    l_m, l_p) adds pinn_physics_loss's residuals (train_pinn.py:64-111) at p =
    s^_k and (n, u, E) = s^_{k-1}, the model's own previous state, and needs dx,
    dt, nu (length: the Poisson operator's domain length, default nx dx); at K =
    1 with (0.1, 0.1, 0.01) this is pinn_physics_loss with PINN_LOSS_WEIGHTS.  A
    scalar with autograd into the model's parameters, through every step's
    network call and, with through_state, through the state the steps hand on
    (the network's input and the residuals' state slot).  through_state=False
    cuts both between steps (the pushforward form).  Per unrolled step the
    forward is hf_pinn_forward_train + one hf_pinn_unroll_loss launch, the
    backward one hf_pinn_unroll_adjoint launch + hf_pinn_backward.
    return_states: also the predicted states [K,B,3,nx] and the steps' terms
    [K,5] = (total, data, cont, mom, pois), both without gradient.
    conservation = (lam_e, lam_q) adds L_cons = (1/K) sum_k mean_b [ lam_e
    (e(s^_k)_b - eref_kb)^2 + lam_q (q(s^_k)_b - qref_kb)^2 ] with e = 0.5 (sum
    u^2 + sum E^2) / nx and q = sum n / nx (the energy and charge the evaluation
    scores), in float64, inside the same launches (the _ex calls of
    include/hybridflux.h) plus one hf_state_moments launch; conservation_ref:
    "target" (the reference of step k is the classical s*_k), "start" (s*_0 for
    every step: the drift the evaluation reports) or a float64 [B,K,2] tensor of
    (eref, qref).  None (the default): the calls and bits of the loss without the
    terms.  With conservation the steps' rows are
    [K,7] = (total, data, cont, mom, pois, energy, charge)."""
    return _rollout_loss(_PINN, model, traj, None, _pinn_phys(physics_weights, dx, dt, nu, length), channel_weights,
                         through_state, return_states, _conservation(conservation, conservation_ref))


def pinn_unrolled_step(model, opt, traj, dx=None, dt=None, nu=None, channel_weights=(1.0, 1.0, 1.0),
                       physics_weights=None, through_state=True, length=None, conservation=None,
                       conservation_ref="target"):
    """pinn_unrolled_loss -> backward -> opt.step() without autograd, after
    pure_unrolled_step: where pinn_step's direct path applies (the optimizer
    drives exactly the model's parameters, no parameter hooks, no anomaly mode)
    and the parameters share one buffer (flatten_parameters_).  The same
    forwards, adjoints, backwards and gradient sum as the autograd step, in the
    same order, so the same parameters bit for bit.  Returns the detached loss,
    or None when the case does not apply (the caller then takes the autograd
    step)."""
    return _rollout_step(_PINN, model, opt, traj, None, _pinn_phys(physics_weights, dx, dt, nu, length),
                         channel_weights, through_state, _conservation(conservation, conservation_ref))


def pinn_unrolled_train_flop_per_sample(K=4, D=192, H=256, L=4):
    """Algorithmic FLOPs of one sample (one K-step window) of PINN's unrolled
    training step: K times pinn_train_flop_per_sample, plus the first layer's
    data gradient 2DH for the K - 1 steps that hand a state gradient back.  The
    loss terms and their adjoints are not counted."""
    return K * pinn_train_flop_per_sample(D, H, L) + (K - 1) * 2 * D * H


def train_pinn_unrolled(trajectories, dx, dt, nu, K=4, epochs=10, lr=1e-3, batch_size=32, hidden_dim=256, num_layers=4,
                        physics_weights=None, seed=None, init=None, channel_weights=(1.0, 1.0, 1.0),
                        through_state=True, device="cuda", save_dir="checkpoints", log=print, weight_decay=0.0,
                        max_grad_norm=None, skip_nonfinite=False, scheduler=None, conservation=None,
                        conservation_ref="target", noise=None, noise_seed=0):
    """Train (or fine-tune) PINN(3 nx, hidden_dim, num_layers) on K-step windows
    of classical trajectories [N,T+1,3,nx] with pinn_unrolled_loss:
    train_unrolled's loop -- Adam(lr) over shuffled batches of batch_size windows
    (WindowDataset), one pinn_unrolled_step each, one host sync per epoch.
    physics_weights None: the state loss alone (dx, dt, nu are then not used);
    (l_c, l_m, l_p): with the residual terms.  seed also seeds the initial
    weights; init: a reference state dict to start from (e.g. train_pinn's).
    Returns (model, history) with history keys epoch, loss, seconds, and writes
    checkpoints/pinn_unrolled_K<K>.pt (the reference PINN's keys) and
    history_pinn_unrolled_K<K>.json (save_dir=None skips).  weight_decay,
    max_grad_norm, skip_nonfinite, scheduler, conservation, conservation_ref,
    noise, noise_seed: as train_unrolled's, except that the StateNoise is used as
    given (its own sigma_E, or its own grid to recompute E)."""
    cons = _conservation(conservation, conservation_ref, trainer=True)
    engine.require_device(torch.empty(0, device=device), "device")
    if seed is not None:
        torch.manual_seed(seed)
    data = WindowDataset(trajectories, K, device)
    phys = _pinn_phys(physics_weights, dx, dt, nu, None) if physics_weights is not None else \
        _PinnPhys(None, None, None, None, None)
    model = PINN(3 * data.nx, hidden_dim, num_layers)
    return _train_windows(_PINN, model, data, None, phys, init, epochs, lr, batch_size, seed, channel_weights,
                          through_state, device, save_dir, log,
                          (weight_decay, max_grad_norm, skip_nonfinite, scheduler), cons, noise, noise_seed)
