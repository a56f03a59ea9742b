"""The reference's other rollout models on the MI355X.

PureGNN (scripts/training/train_pure_gnn.py:35-76) and PINN
(scripts/training/train_pinn.py:36-61) with the reference's module trees, so
their checkpoints load with load_state_dict unchanged, and forward()
signatures; inference runs in the HIP kernels of baselines.hip
(hf_pure_gnn_* / hf_pinn_*).  `rollout` batches the per-IC loops of
scripts/evaluation/evaluate_multi_ic.py:45-83 and benchmark_timing.py:100-203
over B initial conditions in one call.  forward() takes the reference's host
(CPU) tensors too (evaluate_multi_ic.py:53-83 calls them with
torch.FloatTensor states): they are staged to the current HIP device and the
result is copied back.

PureGNN is trainable on the engine: under autograd (grad enabled and a
parameter or the node features requiring grad) forward() runs the training
kernels of pure_train.hip instead (hf_pure_gnn_forward_train keeps a tape on
the device, backward() runs hf_pure_gnn_backward), so the reference's
`batch_loss.backward()` (train_pure_gnn.py:144) and its smoke test's call with
grad enabled (examples/smoke_test.py:98-104) work unchanged; gradients land on
each tensor's own device, and after flatten_parameters_() the kernels read the
parameters in place (hybridflux.training.train_pure_gnn, FlatAdam).  Under
torch.no_grad() the inference kernels run as before.

PINN.forward is the inference call and still raises under autograd; PINN
trains through hybridflux.training instead: pinn_forward (the training kernels
of pinn_train.hip under an autograd Function), pinn_physics_loss, pinn_step
and train_pinn (scripts/training/train_pinn.py:114-201), with
PINN.flatten_parameters_() for FlatAdam.
"""
import torch
import torch.nn as nn

from . import engine
from ._lib import HF_NUM_METRICS, check, lib, ptr
from .flat import flat_params, flatten_, split_flat


def _flat(module):
    return torch.cat([p.detach().reshape(-1).to(torch.float32) for p in module.parameters()]).contiguous()


def _no_grad_guard(module, *inputs):
    if torch.is_grad_enabled() and (any(p.requires_grad for p in module.parameters()) or
                                    any(getattr(t, "requires_grad", False) for t in inputs)):
        raise NotImplementedError(f"{type(module).__name__}: inference kernels only; wrap calls in torch.no_grad()")


class _Flat:
    """Flat device copy of a module's parameters, rebuilt when any changes."""

    def __init__(self):
        self.sig, self.buf = None, None

    def get(self, module, device):
        sig = (str(device),) + tuple((p.data_ptr(), p._version) for p in module.parameters())
        if sig != self.sig:
            self.buf = _flat(module).to(device)
            self.sig = sig
        return self.buf


def _score_buffers(B, T, dev, metrics, compare):
    """The series a scored rollout writes (compare_batch's keys): metrics
    [B,T+1,4] when asked, mse [B,T+1,3] and metrics_classical (with metrics)
    when a BaselineSolver to compare with is given; None otherwise."""
    me = torch.empty(B, T + 1, HF_NUM_METRICS, device=dev) if metrics else None
    mse = torch.empty(B, T + 1, 3, device=dev) if compare is not None else None
    mc = torch.empty(B, T + 1, HF_NUM_METRICS, device=dev) if (compare is not None and metrics) else None
    return me, mse, mc


def _score_grid(compare, nx, dev):
    """Grid constants of the classical twin: (plan, pmode, c, dt, nu, dx2).
    Without a solver to compare with no twin runs and they are unused."""
    if compare is None:
        return None, 0, 0.0, 0.0, 0.0, 0.0
    g = compare.grid
    if g.nx != nx:
        raise ValueError(f"compare: the solver's grid has nx = {g.nx}, the states {nx}")
    return g.on(dev)[1], g.pmode, g.c32, g.dt32, g.nu32, g.dx2_32


class _PureTrainForward(torch.autograd.Function):
    """PureGNN.forward with HIP backward kernels (parameter order = state dict);
    the counterpart of flux_gnn._TrainForward."""

    @staticmethod
    def forward(ctx, node_features, edge_index, dims, *params):
        dev = engine.compute_device(node_features, "node_features")
        flat, _ = flat_params(params, dev)
        delta, tape, nf, ei, chain_nx = engine.pure_gnn_forward_train(flat, dims, node_features.detach().to(dev),
                                                                      edge_index)
        ctx.save_for_backward(flat, tape, nf, ei)
        ctx.dims = dims
        ctx.chain_nx = chain_nx
        ctx.shapes = [q.shape for q in params]
        ctx.param_devices = [q.device for q in params]
        ctx.nf_dtype, ctx.nf_device = node_features.dtype, node_features.device
        return delta.to(node_features.device)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_delta):
        flat, tape, nf, ei = ctx.saved_tensors
        gp, gnf = engine.pure_gnn_backward(flat, ctx.dims, nf, ei, ctx.chain_nx, tape, grad_delta,
                                           ctx.needs_input_grad[0])
        gnf = gnf.to(device=ctx.nf_device, dtype=ctx.nf_dtype) if gnf is not None else None
        return (gnf, None, None, *split_flat(gp, ctx.shapes, ctx.param_devices))


class PureGNN(nn.Module):
    """End-to-end GNN predicting the state change per node (train_pure_gnn.py:35-76)."""

    def __init__(self, input_dim=4, hidden_dim=64, num_layers=3):
        super().__init__()
        self.input_dim, self.hidden_dim, self.num_layers = input_dim, hidden_dim, num_layers
        self.input_mlp = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.Tanh())
        self.update_mlps = nn.ModuleList(
            [nn.Sequential(nn.Linear(hidden_dim * 2, hidden_dim), nn.Tanh()) for _ in range(num_layers)])
        self.output_mlp = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.Tanh(), nn.Linear(hidden_dim, 3))
        self._flat = _Flat()

    def forward(self, node_features, edge_index):
        """node_features [N, input_dim], edge_index [2, E] -> delta_state [N, 3]."""
        params = list(self.parameters())
        if torch.is_grad_enabled() and (node_features.requires_grad or any(q.requires_grad for q in params)):
            dims = (self.input_dim, self.hidden_dim, self.num_layers)
            return _PureTrainForward.apply(node_features, edge_index, dims, *params)
        home = node_features.device
        dev = engine.compute_device(node_features, "node_features")
        nf, ei, N, E, chain_nx = engine._graph_inputs(node_features.to(dev), edge_index, self.input_dim)
        delta = torch.empty(N, 3, device=nf.device)
        H = self.hidden_dim
        ws = torch.empty(int(lib().hf_pure_gnn_workspace_bytes(H, N, E)), dtype=torch.uint8, device=nf.device)
        with torch.cuda.device(nf.device):
            check(lib().hf_pure_gnn_forward(ptr(self._flat.get(self, nf.device)), self.input_dim, H,
                                            self.num_layers, ptr(nf), N, ptr(ei), E, chain_nx, ptr(delta), ptr(ws),
                                            engine.stream_of(nf.device)))
        return delta.to(home)

    def flatten_parameters_(self):
        """Re-home every parameter into one contiguous float32 buffer in
        state-dict order (FluxGNN.flatten_parameters_'s contract: the parameters
        keep their identity, FlatAdam can drive them, and the training forward
        hands the kernels that buffer instead of concatenating the parameters
        each step).  .to() / .cuda() afterwards undo it."""
        return flatten_(self)

    def rollout(self, states0, n_steps, x, traj=True, *, metrics=False, compare=None):
        """B ICs [B,3,nx] (device) -> dict(final [B,3,nx], traj [B,T+1,3,nx] or None);
        the loop of evaluate_multi_ic.py:53-64 with node features [n,u,E,x].

        metrics=True and / or compare=<BaselineSolver> run the scored rollout
        (hf_pure_gnn_run_scored) instead: the same final and traj, and the dict
        also holds compare_batch's keys, metrics [B,T+1,4], mse [B,T+1,3]
        against the classical solver stepped from the same ICs on compare's
        grid (dt, nu, Poisson mode) and metrics_classical [B,T+1,4] (None
        where not asked), written by the rollout kernel itself."""
        if self.input_dim != 4:
            raise ValueError("rollout builds [n,u,E,x] node features: input_dim must be 4")
        engine.require_device(states0, "states0")
        s0 = states0.to(torch.float32).contiguous()
        B, _, nx = s0.shape
        xd = torch.as_tensor(x, dtype=torch.float32, device=s0.device).contiguous()
        final = torch.empty_like(s0)
        tr = torch.empty(B, n_steps + 1, 3, nx, device=s0.device) if traj else None
        if metrics or compare is not None:
            T = int(n_steps)
            me, mse, mc = _score_buffers(B, T, s0.device, metrics, compare)
            plan, pmode, c, dt, nu, dx2 = _score_grid(compare, nx, s0.device)
            nb = int(lib().hf_pure_gnn_score_workspace_bytes(self.hidden_dim, B, nx, T))
            ws = torch.empty(nb, dtype=torch.uint8, device=s0.device) if nb > 0 else None
            with torch.no_grad(), torch.cuda.device(s0.device):
                check(lib().hf_pure_gnn_run_scored(ptr(self._flat.get(self, s0.device)), self.hidden_dim,
                                                   self.num_layers, ptr(s0), ptr(final), ptr(xd), ptr(plan), pmode,
                                                   B, nx, T, c, dt, nu, dx2, ptr(tr), ptr(me), ptr(mse), ptr(mc),
                                                   ptr(ws), max(nb, 0), engine.stream_of(s0.device)))
            return {"final": final, "traj": tr, "metrics": me, "mse": mse, "metrics_classical": mc}
        nb = int(lib().hf_pure_gnn_run_workspace_bytes(self.hidden_dim, B, nx, int(n_steps)))
        ws = torch.empty(nb, dtype=torch.uint8, device=s0.device) if nb > 0 else None
        with torch.no_grad(), torch.cuda.device(s0.device):
            check(lib().hf_pure_gnn_run(ptr(self._flat.get(self, s0.device)), self.hidden_dim, self.num_layers,
                                        ptr(s0), ptr(final), ptr(xd), B, nx, int(n_steps),
                                        ptr(tr) if tr is not None else None, ptr(ws) if ws is not None else None,
                                        engine.stream_of(s0.device)))
        return {"final": final, "traj": tr}


class PINN(nn.Module):
    """MLP on the flattened state predicting the next state (train_pinn.py:36-61)."""

    def __init__(self, input_dim=3 * 64, hidden_dim=256, num_layers=4):
        super().__init__()
        layers = [nn.Linear(input_dim, hidden_dim), nn.Tanh()]
        for _ in range(num_layers - 2):
            layers += [nn.Linear(hidden_dim, hidden_dim), nn.Tanh()]
        layers.append(nn.Linear(hidden_dim, input_dim))
        self.net = nn.Sequential(*layers)
        self.input_dim, self.hidden_dim, self.num_layers = input_dim, hidden_dim, num_layers
        self._flat = _Flat()

    def forward(self, state):
        """state [..., 3, nx] -> state + delta, same shape."""
        _no_grad_guard(self, state)
        dev = engine.compute_device(state, "state")
        s = state.to(device=dev, dtype=torch.float32).contiguous()
        flat = s.reshape(-1, self.input_dim)
        out = torch.empty_like(flat)
        B = flat.shape[0]
        nb = int(lib().hf_pinn_workspace_bytes(self.input_dim, self.hidden_dim, B))
        ws = torch.empty(nb, dtype=torch.uint8, device=s.device) if nb > 0 else None
        with torch.cuda.device(s.device):
            check(lib().hf_pinn_forward(ptr(self._flat.get(self, s.device)), self.input_dim, self.hidden_dim,
                                        self.num_layers, ptr(flat), ptr(out), B, ptr(ws) if ws is not None else None,
                                        engine.stream_of(s.device)))
        return out.reshape(state.shape).to(state.device)

    def flatten_parameters_(self):
        """Re-home every parameter into one contiguous float32 buffer in
        state-dict order (PureGNN.flatten_parameters_'s contract: the
        parameters keep their identity, FlatAdam can drive them, and
        hybridflux.training.pinn_forward / pinn_step hand the kernels that
        buffer instead of concatenating the parameters each step).  .to() /
        .cuda() afterwards undo it."""
        return flatten_(self)

    def rollout(self, states0, n_steps, traj=True, *, metrics=False, compare=None):
        """B ICs [B,3,nx] -> dict(final, traj [B,T+1,3,nx] or None) (evaluate_multi_ic.py:75-81).
        metrics / compare: the scored rollout (hf_pinn_run_scored), as PureGNN.rollout."""
        engine.require_device(states0, "states0")
        s0 = states0.to(torch.float32).contiguous()
        B = s0.shape[0]
        if s0[0].numel() != self.input_dim:
            raise ValueError(f"states0 must hold {self.input_dim} values per IC")
        final = torch.empty_like(s0)
        tr = torch.empty((B, n_steps + 1) + tuple(s0.shape[1:]), device=s0.device) if traj else None
        if metrics or compare is not None:
            T = int(n_steps)
            me, mse, mc = _score_buffers(B, T, s0.device, metrics, compare)
            plan, pmode, c, dt, nu, dx2 = _score_grid(compare, self.input_dim // 3, s0.device)
            nb = int(lib().hf_pinn_score_workspace_bytes(self.input_dim, self.hidden_dim, B, T))
            ws = torch.empty(nb, dtype=torch.uint8, device=s0.device) if nb > 0 else None
            with torch.no_grad(), torch.cuda.device(s0.device):
                check(lib().hf_pinn_run_scored(ptr(self._flat.get(self, s0.device)), self.input_dim, self.hidden_dim,
                                               self.num_layers, ptr(s0), ptr(final), ptr(plan), pmode, B, T, c, dt,
                                               nu, dx2, ptr(tr), ptr(me), ptr(mse), ptr(mc), ptr(ws), max(nb, 0),
                                               engine.stream_of(s0.device)))
            return {"final": final, "traj": tr, "metrics": me, "mse": mse, "metrics_classical": mc}
        nb = int(lib().hf_pinn_workspace_bytes(self.input_dim, self.hidden_dim, B))
        ws = torch.empty(nb, dtype=torch.uint8, device=s0.device) if nb > 0 else None
        with torch.no_grad(), torch.cuda.device(s0.device):
            check(lib().hf_pinn_run(ptr(self._flat.get(self, s0.device)), self.input_dim, self.hidden_dim,
                                    self.num_layers, ptr(s0), ptr(final), B, int(n_steps),
                                    ptr(tr) if tr is not None else None, ptr(ws) if ws is not None else None,
                                    engine.stream_of(s0.device)))
        return {"final": final, "traj": tr}
