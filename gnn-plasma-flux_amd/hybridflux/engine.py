"""Device-side engine: owns the libhybridflux model handles and per-grid
device constants, and launches the hot path on torch's current HIP stream.

Everything here takes and returns torch tensors that already live on a HIP
device; the reference-shaped numpy API (HybridSolver / BaselineSolver) sits
on top of it.  Scalars follow the reference's rounding: the Python floats
dt/dx, dt, nu and dx**2 are rounded to float32 once on the host, exactly as
numpy does when it mixes them with float32 arrays (src/hybrid_solver.py:52,
56-57; src/baseline_solver.py:86,91,94).
"""
import math
from ctypes import c_void_p

import numpy as np
import torch

from . import _lib
from ._lib import HF_NUM_METRICS, HF_OP_COMPARE, HF_OP_RUN, HF_OP_STEP, check, lib, ptr

LOSS_MAX_ROLLOUT = 3  # hf_ablation_loss_ex forms the rollout energy term for rollout_steps <= 3

PARAM_ORDER_DOC = "input_mlp.0.{weight,bias}, update_mlps.<l>.0.{weight,bias}, edge_mlp.0.*, edge_mlp.2.*"


def require_device(t, what="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(
            f"hybridflux: {what} must be a torch tensor on a HIP (cuda) device; this engine has no CPU "
            f"path (got {type(t).__name__}{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)})")
    return t


def compute_device(t, what="tensor"):
    """The HIP device a drop-in call computes on: t's own device when t is a
    device tensor; for a host tensor (the reference's CPU call pattern,
    examples/smoke_test.py:50-56) the current HIP device, to which the
    caller's inputs are staged and from which results are copied back.  No HIP
    device visible: raises (the kernels are the only implementation)."""
    if isinstance(t, torch.Tensor) and t.is_cuda:
        return t.device
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"hybridflux: {what} must be a torch tensor, got {type(t).__name__}")
    if not torch.cuda.is_available():
        raise RuntimeError(f"hybridflux: {what} is a host tensor and no HIP device is visible; this engine has "
                           "no CPU path (host tensors are staged to the current HIP device, and there is none)")
    return torch.device("cuda", torch.cuda.current_device())


def stream_of(device):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def flatten_params(sd, layers):
    """Reference state dict (src/flux_gnn.py:17-38 keys) -> flat float32 array in
    the order include/hybridflux.h documents for hf_model_create."""
    def arr(k):
        v = sd[k]
        if isinstance(v, torch.Tensor):
            v = v.detach().to("cpu", torch.float32).numpy()
        return np.ascontiguousarray(np.asarray(v, dtype=np.float32)).reshape(-1)

    parts = [arr("input_mlp.0.weight"), arr("input_mlp.0.bias")]
    for l in range(layers):
        parts += [arr(f"update_mlps.{l}.0.weight"), arr(f"update_mlps.{l}.0.bias")]
    parts += [arr("edge_mlp.0.weight"), arr("edge_mlp.0.bias"), arr("edge_mlp.2.weight"), arr("edge_mlp.2.bias")]
    return np.ascontiguousarray(np.concatenate(parts))


def dims_of(sd):
    w_in = sd["input_mlp.0.weight"]
    hidden, in_dim = int(w_in.shape[0]), int(w_in.shape[1])
    layers = sum(1 for k in sd if k.startswith("update_mlps.") and k.endswith(".0.weight"))
    return in_dim, hidden, layers


PRECISIONS = {"f32": _lib.HF_WDTYPE_F32, "bf16": _lib.HF_WDTYPE_BF16, "f16x3": _lib.HF_WDTYPE_F16X3}


class DeviceModel:
    """A packed, read-only copy of FluxGNN weights on one device (hf_model_t).

    precision selects the chain kernels' matrix-core arithmetic:
      "f32"   v_mfma_f32_16x16x4_f32, exact float32 (parity reference)
      "f16x3" fp16 hi+lo split of weights and activations, 3 products on
              v_mfma_f32_16x16x32_f16, f32 accumulate: float32-level accuracy
              while every GEMM input stays within the fp16 range (|value| <
              65504; the physical states of this model are O(1), ~1e3x inside
              it); past it the split overflows and the flux is reported
              non-finite where f32 would still be finite (tests: test_f16x3_range)
      "bf16"  bf16 weights and activations, f32 accumulate (BASELINE config 4)
    The generic-graph path always computes in float32.

    radius (1..3) is the stencil radius of the fused chain kernels
    (hf_model_create_ex): the update layers' mean runs over the 2*radius
    neighbours of the radius chain graph (graph_constructor.chain_edge_index),
    "f32" only beyond 1.  The generic-graph path takes its graph from the
    caller and ignores it."""

    def __init__(self, state_dict, device, precision="f32", radius=1):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self.precision = precision
        self.radius = int(radius)
        self.in_dim, self.hidden, self.layers = dims_of(state_dict)
        self.device = torch.device(device)
        flat = flatten_params(state_dict, self.layers)
        want = lib().hf_model_param_count(self.in_dim, self.hidden, self.layers)
        if flat.size != want:
            raise ValueError(f"state dict has {flat.size} parameters, expected {want}")
        self.handle = c_void_p()
        with torch.cuda.device(self.device):
            check(lib().hf_model_create_ex(flat.ctypes.data_as(c_void_p), self.in_dim, self.hidden,
                                           self.layers, PRECISIONS[precision], self.radius, self.handle))

    @property
    def chain_ok(self):
        return self.in_dim == 4 and self.hidden == 128

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            lib().hf_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


class DeviceModelSet:
    """M DeviceModels of one precision on one device behind one handle
    (hf_model_set_t): the table the model-set rollouts index per workgroup.
    Keeps the DeviceModels alive for as long as the set lives; their layer
    counts may differ."""

    def __init__(self, models):
        models = list(models)
        if not models:
            raise ValueError("DeviceModelSet needs at least one model")
        for i, m in enumerate(models):
            if m.precision != models[0].precision:
                raise ValueError(f"DeviceModelSet: model {i} is {m.precision}, model 0 is {models[0].precision}; a set "
                                 "shares one precision")
            if m.device != models[0].device:
                raise ValueError(f"DeviceModelSet: model {i} is on {m.device}, model 0 on {models[0].device}")
            if not m.chain_ok:
                raise ValueError(f"DeviceModelSet: model {i} is not FluxGNN(input_dim=4, hidden_dim=128)")
            if m.radius != models[0].radius:
                raise ValueError(f"DeviceModelSet: model {i} has stencil radius {m.radius}, model 0 has "
                                 f"{models[0].radius}; a set shares one radius")
        self.models = models
        self.device, self.precision = models[0].device, models[0].precision
        self.handle = c_void_p()
        arr = (c_void_p * len(models))(*[m.handle.value for m in models])
        with torch.cuda.device(self.device):
            check(lib().hf_model_set_create(arr, len(models), self.handle))

    def __len__(self):
        return len(self.models)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            lib().hf_model_set_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


POISSON_MODES = {"spectral": _lib.HF_POISSON_SPECTRAL, "tridiagonal": _lib.HF_POISSON_TRIDIAG}


class Grid:
    """Geometry + time-step constants (src/baseline_solver.py:7-27) and their
    device copies: cell centres x (float32) and the Poisson plan.

    poisson selects the operator every step / rollout / solve of this grid
    applies: "spectral" (default) is the reference's (src/baseline_solver.py:
    59-68, the parity mode); "tridiagonal" is the OPT-IN cyclic-reduction solve
    of the second-order potential form of the same equation, which is NOT the
    reference's operator (~1e-3 from it at nx = 64; include/hybridflux.h
    HF_POISSON_TRIDIAG).  The training loss always uses the spectral plan."""

    def __init__(self, nx=64, length=2 * math.pi, dt=5e-3, nu=1e-3, poisson="spectral"):
        if poisson not in POISSON_MODES:
            raise ValueError(f"poisson must be one of {sorted(POISSON_MODES)}, got {poisson!r}")
        self.nx, self.length, self.dt, self.nu = int(nx), float(length), float(dt), float(nu)
        self.poisson, self.pmode = poisson, POISSON_MODES[poisson]
        self.dx = self.length / self.nx
        self.x = np.linspace(0.5 * self.dx, self.length - 0.5 * self.dx, self.nx)
        self.c32 = float(np.float32(self.dt / self.dx))
        self.dt32 = float(np.float32(self.dt))
        self.nu32 = float(np.float32(self.nu))
        self.dx2_32 = float(np.float32(self.dx ** 2))
        pc = np.empty(lib().hf_poisson_plan_len(self.nx), dtype=np.float64)
        check(lib().hf_poisson_coeffs(self.nx, self.length, pc.ctypes.data_as(c_void_p)))
        self.poisson_c = pc  # the spectral plan (also the training loss's)
        if self.pmode == _lib.HF_POISSON_SPECTRAL:
            self.plan = pc
        else:
            n = int(lib().hf_poisson_plan_size(self.pmode, self.nx))
            if n < 1:  # (-1: unsupported; checked before allocating)
                raise ValueError(f"{poisson} Poisson does not support nx = {self.nx}")
            self.plan = np.empty(n, dtype=np.float64)
            check(lib().hf_poisson_plan(self.pmode, self.nx, self.length, self.plan.ctypes.data_as(c_void_p)))
        self._dev = {}

    def _consts(self, device):
        device = torch.device(device)
        key = str(device)
        if key not in self._dev:
            x = torch.as_tensor(self.x.astype(np.float32), device=device)
            pc = torch.as_tensor(self.poisson_c, device=device)
            plan = pc if self.plan is self.poisson_c else torch.as_tensor(self.plan, device=device)
            self._dev[key] = (x, plan, pc)
        return self._dev[key]

    def on(self, device):
        """(x, Poisson plan of this grid's mode) on device."""
        x, plan, _ = self._consts(device)
        return x, plan

    def spectral_plan(self, device):
        """The spectral plan on device (hf_ablation_loss: the reference trainer's solve)."""
        return self._consts(device)[2]


def _state(t, nx):
    require_device(t, "state")
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[1] != 3 or t.shape[2] != nx:
        raise ValueError(f"state must be float32 [B,3,{nx}], got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def workspace(op, B, nx, T, dev, given=None, model=None, traj=False, flux_face=False):
    """Scratch for the generic (non-fused) sequencing of hf_step / hf_run /
    hf_run_compare: the caller's uint8 device tensor (checked), or one from
    torch's stream-ordered caching allocator, so no hipMalloc runs inside a
    rollout.  Sized by hf_workspace_need for this path: `model` is the
    DeviceModel (None = classical), `traj` / `flux_face` whether the call gets
    a trajectory / face-flux buffer.  Paths that need no scratch (the fused
    rollouts, the one-launch classical rollouts) get None.  Returns (tensor or
    None, bytes)."""
    flags = (_lib.HF_WS_TRAJ if traj is not False and traj is not None else 0) | \
            (_lib.HF_WS_FLUX_FACE if flux_face is not False and flux_face is not None else 0)
    handle = model.handle if model is not None else None
    nbytes = int(lib().hf_workspace_need(handle, op, B, nx, T, flags))
    if nbytes < 0:
        raise ValueError(f"bad workspace query (op={op}, B={B}, nx={nx}, T={T})")
    if given is not None:
        if not (given.is_cuda and given.device == dev and given.numel() * given.element_size() >= nbytes):
            raise ValueError(f"workspace must be a device tensor of >= {nbytes} bytes on {dev}")
        return given, given.numel() * given.element_size()
    if nbytes == 0:
        return None, 0
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def step(model, grid, state, flux_face=False, metrics=False, ws=None):
    """One hybrid (model) or classical (model=None) step for state [B,3,nx]."""
    state = _state(state, grid.nx)
    B, dev = state.shape[0], state.device
    out = torch.empty_like(state)
    F = torch.empty(B, grid.nx, device=dev) if flux_face else None
    M = torch.empty(B, HF_NUM_METRICS, device=dev) if metrics else None
    x, pc = grid.on(dev)
    w, wb = workspace(HF_OP_STEP, B, grid.nx, 1, dev, ws, model=model, flux_face=flux_face)
    with torch.cuda.device(dev):
        check(lib().hf_step_ex(model.handle if model else None, ptr(state), ptr(out), ptr(x), ptr(pc),
                               grid.pmode, B, grid.nx, grid.c32, grid.dt32, grid.nu32, grid.dx2_32, ptr(F), ptr(M), ptr(w), wb,
                            stream_of(dev)))
    return out, F, M


def _buf(want, given, shape, dev):
    """An output buffer: the caller's preallocated tensor (checked), a new one, or None."""
    if isinstance(given, torch.Tensor):
        if tuple(given.shape) != tuple(shape) or given.dtype != torch.float32 or given.device != dev \
                or not given.is_contiguous():
            raise ValueError(f"preallocated output must be contiguous float32 {tuple(shape)} on {dev}")
        return given
    return torch.empty(shape, device=dev) if want else None


def run(model, grid, state0, T, traj=True, flux=False, metrics=False, out=None, ws=None):
    """T-step rollout; returns dict(final, traj [B,T+1,3,nx], flux [B,T,nx], metrics [B,T+1,4]).
    traj/flux/metrics may be bools or preallocated tensors, and ws a preallocated
    workspace (kept out of timed regions).  out may be state0 itself."""
    state0 = _state(state0, grid.nx)
    B, dev = state0.shape[0], state0.device
    T = int(T)
    final = torch.empty_like(state0) if out is None else out
    tr = _buf(traj, traj, (B, T + 1, 3, grid.nx), dev)
    fl = _buf(flux, flux, (B, T, grid.nx), dev)
    me = _buf(metrics, metrics, (B, T + 1, HF_NUM_METRICS), dev)
    x, pc = grid.on(dev)
    w, wb = workspace(HF_OP_RUN, B, grid.nx, T, dev, ws, model=model, traj=tr)
    with torch.cuda.device(dev):
        check(lib().hf_run_ex(model.handle if model else None, ptr(state0), ptr(final), ptr(x), ptr(pc),
                              grid.pmode, B, grid.nx, T, grid.c32, grid.dt32, grid.nu32, grid.dx2_32, ptr(tr), ptr(fl),
                           ptr(me), ptr(w), wb, stream_of(dev)))
    return {"final": final, "traj": tr, "flux": fl, "metrics": me}


def coarsen_traj(traj_f, flux_f, refine, substeps):
    """hf_coarsen_traj: a recorded fine trajectory [B,T_f+1,3,nx_f] (and its flux
    [B,T_f,nx_f] or None) box-averaged over `refine` cells and sampled /
    time-averaged over `substeps` steps -> (traj_c [B,T_f/S+1,3,nx_f/r], flux_c
    [B,T_f/S,nx_f/r] or None).  The definition hf_run_coarse equals bit for bit."""
    require_device(traj_f, "traj")
    if traj_f.dtype != torch.float32 or traj_f.dim() != 4 or traj_f.shape[2] != 3:
        raise ValueError(f"traj must be float32 [B,T_f+1,3,nx_f], got {tuple(traj_f.shape)} {traj_f.dtype}")
    traj_f = traj_f.contiguous()
    B, T1, _, nx_f = traj_f.shape
    r, S, T_f, dev = int(refine), int(substeps), T1 - 1, traj_f.device
    if r < 1 or S < 1 or nx_f % r or T_f % S:
        raise ValueError(f"refine must divide nx_f = {nx_f} and substeps T_f = {T_f}, got {refine}, {substeps}")
    if flux_f is not None:
        require_device(flux_f, "flux")
        if flux_f.dtype != torch.float32 or tuple(flux_f.shape) != (B, T_f, nx_f) or flux_f.device != dev:
            raise ValueError(f"flux must be float32 [{B},{T_f},{nx_f}] on {dev}, got {tuple(flux_f.shape)} {flux_f.dtype}")
        flux_f = flux_f.contiguous()
    tc = torch.empty(B, T_f // S + 1, 3, nx_f // r, device=dev)
    fc = torch.empty(B, T_f // S, nx_f // r, device=dev) if flux_f is not None else None
    with torch.cuda.device(dev):
        check(lib().hf_coarsen_traj(ptr(traj_f), ptr(flux_f), B, nx_f, T_f, r, S, ptr(tc), ptr(fc), stream_of(dev)))
    return tc, fc


def run_coarse_workspace(B, nx_f, T_c, refine, substeps):
    """hf_run_coarse_workspace_bytes: the scratch with which T_c coarse steps run
    as one chunk (0 where the rollout is one launch)."""
    n = int(lib().hf_run_coarse_workspace_bytes(B, nx_f, T_c, refine, substeps))
    if n < 0:
        raise ValueError(f"bad coarse workspace query (B={B}, nx_f={nx_f}, T_c={T_c}, refine={refine}, "
                         f"substeps={substeps})")
    return n


COARSE_WS_CAP = 256 << 20  # run_coarse's own scratch: chunks of coarse steps that fit this (at least one step)


def run_coarse(grid_f, state0, T_c, refine, substeps, traj=True, flux=False, final=False, ws=None):
    """hf_run_coarse: the classical rollout of the FINE grid `grid_f` over T_c *
    substeps fine steps from fine states [B,3,nx_f], coarse-grained as it runs.
    Returns dict(traj [B,T_c+1,3,nx_f/r] | None, flux [B,T_c,nx_f/r] | None,
    final_fine [B,3,nx_f] | None).  ws: a preallocated uint8 workspace (the
    sequenced path runs the chunks of coarse steps that fit it)."""
    state0 = _state(state0, grid_f.nx)
    B, dev, nx_f = state0.shape[0], state0.device, grid_f.nx
    T_c, r, S = int(T_c), int(refine), int(substeps)
    if not (traj or flux or final):
        raise ValueError("run_coarse: ask for at least one of traj, flux, final")
    one = run_coarse_workspace(B, nx_f, min(T_c, 1), r, S)  # validates B, nx_f, r, S, T_c >= 0
    if T_c < 0:
        raise ValueError("run_coarse: T_c must be >= 0")
    nx_c = nx_f // r
    tr = torch.empty(B, T_c + 1, 3, nx_c, device=dev) if traj else None
    fl = torch.empty(B, T_c, nx_c, device=dev) if flux else None
    fin = torch.empty_like(state0) if final else None
    if ws is None and one > 0:
        ws = torch.empty(max(one, min(run_coarse_workspace(B, nx_f, T_c, r, S), COARSE_WS_CAP)), dtype=torch.uint8,
                         device=dev)
    wb = ws.numel() * ws.element_size() if ws is not None else 0
    _, plan = grid_f.on(dev)
    with torch.cuda.device(dev):
        check(lib().hf_run_coarse(ptr(state0), ptr(fin), ptr(plan), grid_f.pmode, B, nx_f, T_c, r, S, grid_f.c32,
                                  grid_f.dt32, grid_f.nu32, grid_f.dx2_32, ptr(tr), ptr(fl), ptr(ws), wb,
                                  stream_of(dev)))
    return {"traj": tr, "flux": fl, "final_fine": fin}


def poisson_traj(grid, traj):
    """Overwrites the E rows of a trajectory [B,T1,3,nx] in place with
    poisson(grid, its n rows): one strided hf_poisson_ex call over all B*T1 rows."""
    require_device(traj, "traj")
    if traj.dtype != torch.float32 or traj.dim() != 4 or traj.shape[2] != 3 or traj.shape[3] != grid.nx \
            or not traj.is_contiguous():
        raise ValueError(f"traj must be contiguous float32 [B,T1,3,{grid.nx}], got {tuple(traj.shape)} {traj.dtype}")
    rows, nx = traj.shape[0] * traj.shape[1], grid.nx
    if rows:
        _, pc = grid.on(traj.device)
        base = traj.data_ptr()
        with torch.cuda.device(traj.device):
            check(lib().hf_poisson_ex(c_void_p(base), 3 * nx, c_void_p(base + 8 * nx), 3 * nx, ptr(pc), grid.pmode,
                                      rows, nx, stream_of(traj.device)))
    return traj


def run_compare(model, grid, state0, T, metrics=True, out=None, ws=None):
    """Hybrid rollout and its classical twin from the same ICs, scored per step
    (scripts/evaluation/evaluate_multi_ic.py:21-94).  Returns dict(final,
    mse [B,T+1,3] (n,u,E), metrics [B,T+1,4], metrics_classical [B,T+1,4])."""
    state0 = _state(state0, grid.nx)
    B, dev = state0.shape[0], state0.device
    T = int(T)
    final = torch.empty_like(state0) if out is None else out
    mse = torch.empty(B, T + 1, 3, device=dev)
    me = torch.empty(B, T + 1, HF_NUM_METRICS, device=dev) if metrics else None
    mc = torch.empty(B, T + 1, HF_NUM_METRICS, device=dev) if metrics else None
    x, pc = grid.on(dev)
    w, wb = workspace(HF_OP_COMPARE, B, grid.nx, T, dev, ws, model=model)
    with torch.cuda.device(dev):
        check(lib().hf_run_compare_ex(model.handle, ptr(state0), ptr(final), ptr(x), ptr(pc), grid.pmode, B,
                                      grid.nx, T,
                                   grid.c32, grid.dt32, grid.nu32, grid.dx2_32, ptr(mse), ptr(me), ptr(mc),
                                   ptr(w), wb, stream_of(dev)))
    return {"final": final, "mse": mse, "metrics": me, "metrics_classical": mc}


def set_states(state0, M, nx):
    """The ICs of a model-set rollout: float32 [B,3,nx] shared by the M models,
    or [M,B,3,nx] with each model's own.  Returns (contiguous tensor, B,
    model stride in floats: 0 when shared)."""
    require_device(state0, "state")
    shared = state0.dim() == 3
    if state0.dtype != torch.float32 or state0.dim() not in (3, 4) or tuple(state0.shape[-2:]) != (3, nx) \
            or (not shared and state0.shape[0] != M):
        raise ValueError(f"state must be float32 [B,3,{nx}] (shared ICs) or [{M},B,3,{nx}] (ICs per model), got "
                         f"{tuple(state0.shape)} {state0.dtype}")
    B = state0.shape[-3]
    return state0.contiguous(), B, 0 if shared else B * 3 * nx


def _set_final(state0, stride, out, M, B, nx):
    """state_final [M,B,3,nx] of a set rollout: the caller's `out` (which may be
    state0 itself only when every model has its own ICs) or a new tensor."""
    if out is None:
        return torch.empty(M, B, 3, nx, device=state0.device)
    final = _buf(True, out, (M, B, 3, nx), state0.device)
    if stride == 0 and B > 0 and final.untyped_storage().data_ptr() == state0.untyped_storage().data_ptr():
        raise ValueError("out must not share memory with state0 when the models share their ICs (every model "
                         "reads all of state0); give each model its own ICs [M,B,3,nx] to roll out in place")
    return final


def set_workspace(op, mset, B, nx, T, dev, given=None, traj=False):
    """workspace() for a model set: the largest single-model need (none at the fused nx)."""
    nbytes = int(lib().hf_set_workspace_need(mset.handle, op, B, nx, T, _lib.HF_WS_TRAJ if traj is not None else 0))
    if nbytes < 0:
        raise ValueError(f"bad workspace query (op={op}, B={B}, nx={nx}, T={T})")
    if given is not None:
        if not (given.is_cuda and given.device == dev and given.numel() * given.element_size() >= nbytes):
            raise ValueError(f"workspace must be a device tensor of >= {nbytes} bytes on {dev}")
        return given, given.numel() * given.element_size()
    if nbytes == 0:
        return None, 0
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def run_set(mset, grid, state0, T, traj=True, flux=False, metrics=False, out=None, ws=None):
    """run() for every model of a DeviceModelSet, one launch at nx in
    {16,32,48,64}: state0 [B,3,nx] (shared) or [M,B,3,nx]; returns run()'s dict
    with a leading model axis (final [M,B,3,nx], traj [M,B,T+1,3,nx], flux
    [M,B,T,nx], metrics [M,B,T+1,4]), model m's block bit-identical to
    run(mset.models[m], ...)."""
    M = len(mset)
    state0, B, stride = set_states(state0, M, grid.nx)
    dev = state0.device
    T = int(T)
    final = _set_final(state0, stride, out, M, B, grid.nx)
    tr = _buf(traj, traj, (M, B, T + 1, 3, grid.nx), dev)
    fl = _buf(flux, flux, (M, B, T, grid.nx), dev)
    me = _buf(metrics, metrics, (M, B, T + 1, HF_NUM_METRICS), dev)
    x, pc = grid.on(dev)
    w, wb = set_workspace(HF_OP_RUN, mset, B, grid.nx, T, dev, ws, traj=tr)
    with torch.cuda.device(dev):
        check(lib().hf_run_set(mset.handle, ptr(state0), stride, ptr(final), ptr(x), ptr(pc), grid.pmode, B, grid.nx, T,
                               grid.c32, grid.dt32, grid.nu32, grid.dx2_32, ptr(tr), ptr(fl), ptr(me), ptr(w), wb,
                               stream_of(dev)))
    return {"final": final, "traj": tr, "flux": fl, "metrics": me}


def run_compare_set(mset, grid, state0, T, metrics=True, out=None, ws=None):
    """run_compare() for every model of a DeviceModelSet (one launch at the fused
    nx): run_compare's dict with a leading model axis."""
    M = len(mset)
    state0, B, stride = set_states(state0, M, grid.nx)
    dev = state0.device
    T = int(T)
    final = _set_final(state0, stride, out, M, B, grid.nx)
    mse = torch.empty(M, B, T + 1, 3, device=dev)
    me = torch.empty(M, B, T + 1, HF_NUM_METRICS, device=dev) if metrics else None
    mc = torch.empty(M, B, T + 1, HF_NUM_METRICS, device=dev) if metrics else None
    x, pc = grid.on(dev)
    w, wb = set_workspace(HF_OP_COMPARE, mset, B, grid.nx, T, dev, ws)
    with torch.cuda.device(dev):
        check(lib().hf_run_compare_set(mset.handle, ptr(state0), stride, ptr(final), ptr(x), ptr(pc), grid.pmode, B,
                                       grid.nx, T, grid.c32, grid.dt32, grid.nu32, grid.dx2_32, ptr(mse), ptr(me),
                                       ptr(mc), ptr(w), wb, stream_of(dev)))
    return {"final": final, "mse": mse, "metrics": me, "metrics_classical": mc}


def chain_flux(model, node_features, B, nx, flux_face=False):
    """FluxGNN.forward on B disjoint periodic chains of nx cells -> [B*2nx]
    (a model of radius R: the first 2nx fluxes of each IC's radius-R block).
    flux_face: also the face fluxes [B,nx] = 0.5 (fe[i] + fe[nx+i]), as (fe, ff)."""
    require_device(node_features, "node_features")
    nf = node_features.contiguous()
    if nf.dtype != torch.float32 or nf.shape != (B * nx, 4):
        raise ValueError(f"node_features must be float32 [{B * nx},4], got {tuple(nf.shape)} {nf.dtype}")
    fe = torch.empty(B * 2 * nx, device=nf.device)
    ff = torch.empty(B, nx, device=nf.device) if flux_face else None
    with torch.cuda.device(nf.device):
        check(lib().hf_chain_flux(model.handle, ptr(nf), B, nx, ptr(fe), ptr(ff), stream_of(nf.device)))
    return (fe, ff) if flux_face else fe


def graph_flux(model, node_features, edge_index):
    """FluxGNN.forward on an arbitrary graph (generic path) -> [E]."""
    require_device(node_features, "node_features")
    nf = node_features.to(torch.float32).contiguous()
    ei = edge_index.to(device=nf.device, dtype=torch.int64).contiguous()
    N, E = nf.shape[0], ei.shape[1]
    if nf.dim() != 2 or nf.shape[1] != model.in_dim:
        raise ValueError(f"node_features must be [N,{model.in_dim}], got {tuple(nf.shape)}")
    flux = torch.empty(E, device=nf.device)
    if E == 0:
        return flux
    lo, hi = int(ei.min()), int(ei.max())  # reference raises IndexError on these too
    if lo < 0 or hi >= N:
        raise IndexError(f"edge_index entries must lie in [0, {N}), got [{lo}, {hi}]")
    ws = torch.empty(int(lib().hf_graph_workspace_bytes(model.handle, N, E)), dtype=torch.uint8,
                     device=nf.device)
    with torch.cuda.device(nf.device):
        check(lib().hf_graph_flux(model.handle, ptr(nf), N, ptr(ei), E, ptr(flux), ptr(ws),
                                  stream_of(nf.device)))
    return flux


def graph_flux_radius(model, node_features, edge_index, B, nx):
    """FluxGNN.forward of a radius-R DeviceModel on its own radius-R chain graph
    (edge_index: graph_constructor.chain_edge_index(nx, B, radius=R), unmodified)
    -> all [B*2*R*nx] fluxes, on the generic kernels with the fused kernels'
    arithmetic (hf_graph_flux_radius: neighbour sums times W_b / (2R))."""
    require_device(node_features, "node_features")
    nf = node_features.to(torch.float32).contiguous()
    ei = edge_index.to(device=nf.device, dtype=torch.int64).contiguous()
    N, E = B * nx, 2 * model.radius * B * nx
    if tuple(nf.shape) != (N, model.in_dim) or tuple(ei.shape) != (2, E):
        raise ValueError(f"radius-{model.radius} graph of {B} x {nx} cells: node_features must be [{N},{model.in_dim}] "
                         f"and edge_index [2,{E}], got {tuple(nf.shape)} and {tuple(ei.shape)}")
    flux = torch.empty(E, device=nf.device)
    if E == 0:
        return flux
    ws = torch.empty(int(lib().hf_graph_workspace_bytes(model.handle, N, E)), dtype=torch.uint8, device=nf.device)
    with torch.cuda.device(nf.device):
        check(lib().hf_graph_flux_radius(model.handle, ptr(nf), B, nx, ptr(ei), ptr(flux), ptr(ws),
                                         stream_of(nf.device)))
    return flux


def _graph_inputs(node_features, edge_index, in_dim):
    require_device(node_features, "node_features")
    nf = node_features.detach().to(torch.float32).contiguous()
    ei = edge_index.to(device=nf.device, dtype=torch.int64).contiguous()
    if nf.dim() != 2 or nf.shape[1] != in_dim:
        raise ValueError(f"node_features must be [N,{in_dim}], got {tuple(nf.shape)}")
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError(f"edge_index must be [2,E], got {tuple(ei.shape)}")
    N, E = nf.shape[0], ei.shape[1]
    from .graph_constructor import chain_tag
    tag = chain_tag(edge_index)
    chain_nx = tag[1] if tag is not None and tag[0] * tag[1] == N and E == 2 * N else 0
    if E and not chain_nx:  # an unmodified tagged chain is in range by construction
        lo, hi = int(ei.min()), int(ei.max())  # the reference raises IndexError on these too
        if lo < 0 or hi >= N:
            raise IndexError(f"edge_index entries must lie in [0, {N}), got [{lo}, {hi}]")
    return nf, ei, N, E, chain_nx


def graph_forward_train(params, dims, node_features, edge_index):
    """Training forward (hf_graph_forward_train): params is the flat float32
    device buffer in state-dict order.  Returns (flux [E], tape, nf, ei)."""
    in_dim, hidden, layers = dims
    nf, ei, N, E, chain_nx = _graph_inputs(node_features, edge_index, in_dim)
    if params.device != nf.device:
        raise RuntimeError(f"FluxGNN parameters on {params.device} but node_features on {nf.device}")
    flux = torch.empty(E, device=nf.device)
    tape = torch.empty(int(lib().hf_graph_tape_bytes(in_dim, hidden, layers, N, E)), dtype=torch.uint8,
                       device=nf.device)
    with torch.cuda.device(nf.device):
        check(lib().hf_graph_forward_train(ptr(params), in_dim, hidden, layers, ptr(nf), N, ptr(ei), E, chain_nx,
                                           ptr(flux), ptr(tape), stream_of(nf.device)))
    return flux, tape, nf, ei, chain_nx


def graph_backward(params, dims, nf, ei, chain_nx, tape, grad_flux, want_nf_grad):
    """hf_graph_backward: (d params flat [P], d node_features [N,in] or None)."""
    in_dim, hidden, layers = dims
    N, E = nf.shape[0], ei.shape[1]
    g = grad_flux.detach().to(device=nf.device, dtype=torch.float32).contiguous()
    gp = torch.empty_like(params)
    gnf = torch.empty_like(nf) if want_nf_grad else None
    ws = torch.empty(int(lib().hf_graph_backward_workspace_bytes(in_dim, hidden, layers, N, E)),
                     dtype=torch.uint8, device=nf.device)
    with torch.cuda.device(nf.device):
        check(lib().hf_graph_backward(ptr(params), in_dim, hidden, layers, ptr(nf), N, ptr(ei), E, chain_nx, ptr(tape),
                                      ptr(g), ptr(gp), ptr(gnf) if gnf is not None else None, ptr(ws),
                                      stream_of(nf.device)))
    return gp, gnf


def pure_gnn_forward_train(params, dims, node_features, edge_index):
    """PureGNN's training forward (hf_pure_gnn_forward_train): params is the flat
    float32 device buffer in state-dict order.  Returns (delta [N,3], tape, nf,
    ei, chain_nx); edge_index is range-checked (_graph_inputs)."""
    in_dim, hidden, layers = dims
    nf, ei, N, E, chain_nx = _graph_inputs(node_features, edge_index, in_dim)
    if params.device != nf.device:
        raise RuntimeError(f"PureGNN parameters on {params.device} but node_features on {nf.device}")
    delta = torch.empty(N, 3, device=nf.device)
    nb = int(lib().hf_pure_gnn_tape_bytes(in_dim, hidden, layers, N, E))
    if nb < 0:
        raise ValueError(f"PureGNN training needs N >= 1 and at most 8 layers (N = {N}, layers = {layers})")
    tape = torch.empty(nb, dtype=torch.uint8, device=nf.device)
    with torch.cuda.device(nf.device):
        check(lib().hf_pure_gnn_forward_train(ptr(params), in_dim, hidden, layers, ptr(nf), N, ptr(ei), E, chain_nx,
                                              ptr(delta), ptr(tape), stream_of(nf.device)))
    return delta, tape, nf, ei, chain_nx


def pure_gnn_backward(params, dims, nf, ei, chain_nx, tape, grad_delta, want_nf_grad):
    """hf_pure_gnn_backward: (d params flat [P], d node_features [N,in] or None)."""
    in_dim, hidden, layers = dims
    N, E = nf.shape[0], ei.shape[1]
    g = grad_delta.detach().to(device=nf.device, dtype=torch.float32).contiguous()
    gp = torch.empty_like(params)
    gnf = torch.empty_like(nf) if want_nf_grad else None
    ws = torch.empty(int(lib().hf_pure_gnn_backward_workspace_bytes(in_dim, hidden, layers, N, E)),
                     dtype=torch.uint8, device=nf.device)
    with torch.cuda.device(nf.device):
        check(lib().hf_pure_gnn_backward(ptr(params), in_dim, hidden, layers, ptr(nf), N, ptr(ei), E, chain_nx,
                                         ptr(tape), ptr(g), ptr(gp), ptr(gnf) if gnf is not None else None, ptr(ws),
                                         stream_of(nf.device)))
    return gp, gnf


def state_mse(delta, state_t, state_next):
    """hf_state_mse: (loss [1], d loss / d delta [B*nx,3]) of the PureGNN
    trainer's loss for delta [B*nx,3] and states [B,3,nx] on the device."""
    require_device(delta, "delta")
    d = delta.detach().to(torch.float32).contiguous()
    st = state_t.detach().to(device=d.device, dtype=torch.float32).contiguous()
    sn = state_next.detach().to(device=d.device, dtype=torch.float32).contiguous()
    if st.dim() != 3 or st.shape[1] != 3 or sn.shape != st.shape or tuple(d.shape) != (st.shape[0] * st.shape[2], 3):
        raise ValueError(f"state_mse: delta [B*nx,3] with states [B,3,nx], got {tuple(d.shape)}, "
                         f"{tuple(st.shape)}, {tuple(sn.shape)}")
    B, _, nx = st.shape
    nb = int(lib().hf_state_mse_workspace_bytes(B, nx))
    if nb < 0:
        raise ValueError(f"state_mse: need B >= 1, nx >= 1 (B = {B}, nx = {nx})")
    loss = torch.empty(1, device=d.device)
    gd = torch.empty_like(d)
    ws = torch.empty(nb, dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        check(lib().hf_state_mse(ptr(d), ptr(st), ptr(sn), B, nx, ptr(loss), ptr(gd), ptr(ws), nb,
                                 stream_of(d.device)))
    return loss, gd


def _pinn_dims(dims, B):
    dim, hidden, layers = dims
    nb = int(lib().hf_pinn_tape_bytes(dim, hidden, layers, B))
    if nb < 0:
        raise ValueError(f"PINN training needs B >= 1, positive dims and 2..8 layers (B = {B}, dims = {dims})")
    return dim, hidden, layers, nb


def pinn_forward_train(params, dims, state, out=None):
    """PINN's training forward (hf_pinn_forward_train): params is the flat
    float32 device buffer in state-dict order, state [B, dim] float32 on its
    device.  Returns (out [B, dim] = state + net(state), tape).  out: a
    preallocated contiguous float32 [B, dim] on the state's device to write."""
    require_device(state, "state")
    if state.dtype != torch.float32 or state.dim() != 2 or state.shape[1] != dims[0] or not state.is_contiguous():
        raise ValueError(f"pinn_forward_train: state must be contiguous float32 [B,{dims[0]}], got "
                         f"{tuple(state.shape)} {state.dtype}")
    if params.device != state.device:
        raise RuntimeError(f"PINN parameters on {params.device} but the state on {state.device}")
    B = state.shape[0]
    dim, hidden, layers, nb = _pinn_dims(dims, B)
    if out is None:
        out = torch.empty_like(state)
    elif out.dtype != torch.float32 or out.shape != state.shape or out.device != state.device or not out.is_contiguous():
        raise ValueError(f"pinn_forward_train: out must be contiguous float32 {tuple(state.shape)} on {state.device}")
    tape = torch.empty(nb, dtype=torch.uint8, device=state.device)
    with torch.cuda.device(state.device):
        check(lib().hf_pinn_forward_train(ptr(params), dim, hidden, layers, ptr(state), B, ptr(out), ptr(tape),
                                          stream_of(state.device)))
    return out, tape


def pinn_backward(params, dims, state, tape, grad_out, want_state_grad, grad_params=None):
    """hf_pinn_backward: (d params flat [P], d state [B, dim] or None).
    grad_params: a preallocated flat buffer to overwrite."""
    dim, hidden, layers = dims
    B = state.shape[0]
    g = grad_out.detach().to(device=state.device, dtype=torch.float32).contiguous()
    if g.numel() != state.numel():
        raise ValueError(f"pinn_backward: grad_out must hold {B} x {dim} values, got {tuple(g.shape)}")
    gp = torch.empty_like(params) if grad_params is None else grad_params
    gs = torch.empty_like(state) if want_state_grad else None
    nb = int(lib().hf_pinn_backward_workspace_bytes(dim, hidden, layers, B))
    ws = torch.empty(nb, dtype=torch.uint8, device=state.device)
    with torch.cuda.device(state.device):
        check(lib().hf_pinn_backward(ptr(params), dim, hidden, layers, ptr(state), B, ptr(tape), ptr(g), ptr(gp),
                                     ptr(gs), ptr(ws), nb, stream_of(state.device)))
    return gp, gs


_PINN_PLANS = {}


def pinn_loss_plan(nx, length, device):
    """The spectral Poisson plan hf_pinn_loss reads (hf_poisson_coeffs(nx,
    length)) on device, cached per (nx, length, device)."""
    key = (int(nx), float(length), str(device))
    pc = _PINN_PLANS.get(key)
    if pc is None:
        host = np.empty(lib().hf_poisson_plan_len(int(nx)), dtype=np.float64)
        check(lib().hf_poisson_coeffs(int(nx), float(length), host.ctypes.data_as(c_void_p)))
        pc = _PINN_PLANS[key] = torch.from_numpy(host).to(device)
    return pc


def pinn_loss(pred, state_t, state_next, dx, dt, nu, weights, length=None):
    """hf_pinn_loss: (losses [5] = (loss, data, cont, mom, pois), d loss / d pred
    [B,3,nx]) of the PINN trainer's loss (train_pinn.py:64-111, :163-175) for
    pred, state_t, state_next [B,3,nx]; pred on the device, the states staged
    to it.  length: the domain length of the Poisson operator (default nx dx)."""
    require_device(pred, "pred")
    p = pred.detach().to(torch.float32).contiguous()
    st = state_t.detach().to(device=p.device, dtype=torch.float32).contiguous()
    sn = state_next.detach().to(device=p.device, dtype=torch.float32).contiguous()
    if p.dim() != 3 or p.shape[1] != 3 or st.shape != p.shape or sn.shape != p.shape:
        raise ValueError(f"pinn_loss: pred, state_t, state_next must be [B,3,nx], got {tuple(p.shape)}, "
                         f"{tuple(st.shape)}, {tuple(sn.shape)}")
    B, _, nx = p.shape
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
    if w.size != 4:
        raise ValueError("pinn_loss: weights must be (w_data, w_continuity, w_momentum, w_poisson)")
    nb = int(lib().hf_pinn_loss_workspace_bytes(B, nx))
    if nb < 0:
        raise ValueError(f"pinn_loss: need B >= 1, nx >= 1 (B = {B}, nx = {nx})")
    pc = pinn_loss_plan(nx, nx * float(dx) if length is None else length, p.device)
    losses = torch.empty(5, device=p.device)
    gp = torch.empty_like(p)
    ws = torch.empty(nb, dtype=torch.uint8, device=p.device)
    with torch.cuda.device(p.device):
        check(lib().hf_pinn_loss(ptr(p), ptr(st), ptr(sn), B, nx, float(dt), float(dx), float(nu), ptr(w), ptr(pc),
                                 ptr(losses), ptr(gp), ptr(ws), nb, stream_of(p.device)))
    return losses, gp


def poisson(grid, n):
    """Poisson E for densities n [B,nx]: the grid's mode (spectral: src/baseline_solver.py:59-68)."""
    require_device(n, "n")
    n = n.to(torch.float32).contiguous()
    B = n.shape[0]
    E = torch.empty_like(n)
    _, pc = grid.on(n.device)
    with torch.cuda.device(n.device):
        check(lib().hf_poisson_ex(ptr(n), grid.nx, ptr(E), grid.nx, ptr(pc), grid.pmode, B, grid.nx,
                                  stream_of(n.device)))
    return E


def ic_seeds(seeds):
    """Seeds (a range, list, numpy array or CPU tensor of integers) -> int64
    numpy array, validated on the host as np.random.RandomState validates an
    integer seed.  None (numpy: seed from the OS) has no device counterpart."""
    if seeds is None:
        raise ValueError("device_rng needs integer seeds; seed=None draws from the OS and cannot be reproduced")
    if isinstance(seeds, torch.Tensor):
        if seeds.is_cuda:
            raise ValueError("seeds must be on the host (they are validated there and uploaded once)")
        seeds = seeds.numpy()
    if not isinstance(seeds, np.ndarray):
        seeds = list(seeds)
        if any(s is None for s in seeds):
            raise ValueError("device_rng needs integer seeds; seed=None draws from the OS and cannot be reproduced")
        seeds = np.asarray(seeds) if seeds else np.zeros(0, dtype=np.int64)
    if seeds.dtype.kind not in "iu":
        if seeds.dtype.kind != "O":
            raise TypeError(f"seeds must be integers, got dtype {seeds.dtype}")
        import operator
        seeds = np.asarray([operator.index(s) for s in seeds.reshape(-1)], dtype=object)  # (ints beyond int64)
    seeds = seeds.reshape(-1)
    if seeds.size and (seeds.min() < 0 or seeds.max() > 0xFFFFFFFF):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    return np.ascontiguousarray(seeds.astype(np.int64))


def initial_conditions(grid, seeds, debug=False, device=None):
    """ICs of src/baseline_solver.py:29-57 for integer seeds, drawn on the device
    (hf_initial_conditions: numpy's MT19937 words, one wave per seed) -> state
    [B,3,nx] with E = poisson(grid, n).  debug: also the draw table [B,
    HF_IC_TABLE_LEN] float64 (mode count, (km, amp, ph) x 7, words consumed;
    include/hybridflux.h), which equals numpy's draws exactly."""
    s = ic_seeds(seeds)
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("hybridflux: no HIP device is visible; this engine has no CPU path")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    B, nx = int(s.size), grid.nx
    st = torch.empty(B, 3, nx, dtype=torch.float32, device=device)
    table = torch.empty(B, _lib.HF_IC_TABLE_LEN, dtype=torch.float64, device=device) if debug else None
    if B:
        key = ("x64", str(device))
        if key not in grid._dev:
            grid._dev[key] = torch.as_tensor(grid.x, dtype=torch.float64, device=device)
        sd = torch.as_tensor(s, device=device)
        with torch.cuda.device(device):
            check(lib().hf_initial_conditions(ptr(sd), B, nx, ptr(grid._dev[key]), ptr(st), ptr(table),
                                              stream_of(device)))
        st[:, 2] = poisson(grid, st[:, 0])
    return (st, table) if debug else st


def noise_sigma(sigma):
    """(sigma_n, sigma_u, sigma_E) -> host float32 [3]; each >= 0."""
    s = np.ascontiguousarray(np.asarray(sigma, dtype=np.float32).reshape(-1))
    if s.size != 3 or not (s >= 0).all():
        raise ValueError(f"sigma must be (sigma_n, sigma_u, sigma_E), each >= 0, got {sigma!r}")
    return s


def state_noise(state, seeds, sigma, zero_mean=True, grid=None, x=None, out=None, return_noise=False):
    """hf_state_noise: state [B,3,nx] (contiguous float32 on the device) plus
    seeded Gaussian noise, sample b from np.random.RandomState(seeds[b])
    .standard_normal(3 nx) (blocks n, u, E) drawn on the device, one wave per
    sample: out[ch] = state[ch] + f32(sigma[ch]) * f32(g_ch), a channel with
    sigma 0 copied bit for bit.  zero_mean: the mean of the n noise is removed
    (float64, fixed order), so the charge stays; needs nx <= 6144.  grid (an
    engine.Grid): E is recomputed from the perturbed n by the grid's Poisson
    solve, and sigma_E must be 0.  x [nx] (float32 on the device): also the node
    features [B*nx,4] = [n', u', E', x].  seeds: integers on the host (validated
    as numpy validates a seed, uploaded once) or an int64 tensor [B] on the
    device, used as it is (no host sync; a seed outside [0, 2^32) gives a NaN
    sample).  out: the tensor to write, `state` itself for an in-place call.
    Returns out, then the node features (with x), then the added float32 values
    [B,3,nx] (with return_noise)."""
    require_device(state, "state")
    if state.dim() != 3 or state.shape[1] != 3 or state.shape[2] < 1 or state.dtype != torch.float32 \
            or not state.is_contiguous():
        raise ValueError(f"state must be contiguous float32 [B,3,nx], got {tuple(state.shape)} {state.dtype}")
    B, _, nx = state.shape
    dev = state.device
    sig = noise_sigma(sigma)
    if isinstance(seeds, torch.Tensor) and seeds.is_cuda:
        if seeds.dtype != torch.int64 or seeds.device != dev:
            raise ValueError(f"device seeds must be int64 on {dev}, got {seeds.dtype} on {seeds.device}")
        sd = seeds.reshape(-1).contiguous()
    else:
        sd = torch.as_tensor(ic_seeds(seeds), device=dev)
    if sd.numel() != B:
        raise ValueError(f"need one seed per sample: {sd.numel()} seeds for {B} states")
    if out is None:
        out = torch.empty_like(state)
    elif out is not state and (out.shape != state.shape or out.dtype != state.dtype or out.device != dev
                               or not out.is_contiguous()):
        raise ValueError(f"out must be contiguous float32 {tuple(state.shape)} on {dev}")
    plan, pmode = None, 0
    if grid is not None:
        if grid.nx != nx:
            raise ValueError(f"grid.nx = {grid.nx} but the states have nx = {nx}")
        if sig[2] != 0:
            raise ValueError("with a grid E is recomputed from the perturbed n: sigma_E must be 0")
        plan, pmode = grid.on(dev)[1], grid.pmode
    nf = None
    if x is not None:
        require_device(x, "x")
        if x.dtype != torch.float32 or x.numel() != nx or not x.is_contiguous():
            raise ValueError(f"x must be contiguous float32 [{nx}], got {tuple(x.shape)} {x.dtype}")
        nf = torch.empty(B * nx, 4, dtype=torch.float32, device=dev)
    noise = torch.empty_like(state) if return_noise else None
    with torch.cuda.device(dev):
        check(lib().hf_state_noise(ptr(sd), B, nx, ptr(sig), _lib.HF_NOISE_ZERO_MEAN if zero_mean else 0, ptr(state),
                                   ptr(out), ptr(plan), pmode, ptr(x), ptr(nf), ptr(noise), stream_of(dev)))
    res = (out,) + ((nf,) if x is not None else ()) + ((noise,) if return_noise else ())
    return res[0] if len(res) == 1 else res


def _series(t, shape_tail, what):
    require_device(t, what)
    if t.dim() == 4:  # [M,B,T+1,.] of a model set: the rows are independent, so M*B of them
        t = t.reshape(-1, *t.shape[2:]) if t.is_contiguous() else t
    if t.dtype != torch.float32 or tuple(t.shape[2:]) != shape_tail or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous float32 [B,T+1,{','.join(map(str, shape_tail))}], "
                         f"got {tuple(t.shape)} {t.dtype}")
    return t


def traj_metrics(traj):
    """Metric series [B,T1,4] of trajectories [B,T1,3,nx] (hf_traj_metrics)."""
    require_device(traj, "traj")
    traj = traj.to(torch.float32).contiguous()
    B, T1, _, nx = traj.shape
    out = torch.empty(B, T1, HF_NUM_METRICS, device=traj.device)
    with torch.cuda.device(traj.device):
        check(lib().hf_traj_metrics(ptr(traj), B, T1, nx, ptr(out), stream_of(traj.device)))
    return out


def traj_mse(a, b):
    """Per-step channel MSE [B,T1,3] of two trajectories [B,T1,3,nx] (hf_traj_mse)."""
    require_device(a, "traj a")
    require_device(b, "traj b")
    a, b = a.to(torch.float32).contiguous(), b.to(device=a.device, dtype=torch.float32).contiguous()
    if a.shape != b.shape or a.dim() != 4 or a.shape[2] != 3:
        raise ValueError(f"trajectories must both be [B,T1,3,nx], got {tuple(a.shape)} and {tuple(b.shape)}")
    B, T1, _, nx = a.shape
    out = torch.empty(B, T1, 3, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().hf_traj_mse(ptr(a), ptr(b), B, T1, nx, ptr(out), stream_of(a.device)))
    return out


def rollout_summary(metrics, mse=None, metrics_ref=None, drift=False):
    """hf_rollout_summary: (summary [B,8], drift [B,T+1,4] or None); fields in
    include/hybridflux.h (HF_NUM_SUMMARY).  Series with a leading model axis
    ([M,B,T+1,.], a model set's) give summary [M,B,8] and drift [M,B,T+1,4]:
    the kernel works per row."""
    lead = tuple(metrics.shape[:2]) if isinstance(metrics, torch.Tensor) and metrics.dim() == 4 else None
    metrics = _series(metrics, (HF_NUM_METRICS,), "metrics")
    B, T1 = metrics.shape[:2]
    dev = metrics.device
    if mse is not None:
        mse = _series(mse, (3,), "mse")
    if metrics_ref is not None:
        metrics_ref = _series(metrics_ref, (HF_NUM_METRICS,), "metrics_ref")
    for o in (mse, metrics_ref):
        if o is not None and (o.shape[:2] != (B, T1) or o.device != dev):
            raise ValueError("metric series must share [B,T+1] and the device")
    summ = torch.empty(B, _lib.HF_NUM_SUMMARY, device=dev)
    dr = torch.empty(B, T1, 4, device=dev) if drift else None
    with torch.cuda.device(dev):
        check(lib().hf_rollout_summary(ptr(metrics), ptr(mse), ptr(metrics_ref), B, T1 - 1, ptr(summ), ptr(dr),
                                       stream_of(dev)))
    if lead is not None:
        summ = summ.reshape(*lead, _lib.HF_NUM_SUMMARY)
        dr = dr.reshape(*lead, T1, 4) if dr is not None else None
    return summ, dr


def chain_batch(idx, state_t, flux_t, state_next, x):
    """hf_chain_batch_gather: a training batch of a device dataset
    (train_ablation.py:27-44, indexed by the batch) and its chain node
    features [n, u, E, x] (src/graph_constructor.py:6-39, batched) in one pass.
    idx [B] sample indices; state_t / state_next [N,3,nx], flux_t [N,nx]
    float32 device tensors; x [nx].  Returns (st [B,3,nx], ft [B,nx],
    sn [B,3,nx], node_features [B*nx,4])."""
    for t, what in ((state_t, "state_t"), (flux_t, "flux_t"), (state_next, "state_next")):
        require_device(t, what)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"chain batch: {what} must be a contiguous float32 tensor")
    N, _, nx = state_t.shape
    dev = state_t.device
    if state_next.shape != state_t.shape or flux_t.shape != (N, nx):
        raise ValueError("chain batch: dataset shapes must be state [N,3,nx], flux_t [N,nx]")
    idx = torch.as_tensor(idx, device=dev).to(torch.long).reshape(-1).contiguous()
    x = torch.as_tensor(x, dtype=torch.float32, device=dev).reshape(-1).contiguous()
    if x.numel() != nx:
        raise ValueError("chain batch: x must hold nx positions")
    B = idx.numel()
    st = torch.empty(B, 3, nx, device=dev)
    ft = torch.empty(B, nx, device=dev)
    sn = torch.empty(B, 3, nx, device=dev)
    nf = torch.empty(B * nx, 4, device=dev)
    with torch.cuda.device(dev):
        check(lib().hf_chain_batch_gather(ptr(idx), B, ptr(state_t), ptr(flux_t), ptr(state_next), N, nx, ptr(x),
                                          ptr(st), ptr(ft), ptr(sn), ptr(nf), stream_of(dev)))
    return st, ft, sn, nf


def adam_flat(params, grads, exp_avg, exp_avg_sq, step, done, lr, beta1, beta2, eps):
    """hf_adam_flat: torch.optim.Adam's update on one flat float32 parameter
    buffer (train_ablation.py:208-209), the step count `step` (float32 [1]) on
    the device and incremented by the call; `done` a uint32-sized zeroed
    buffer the kernel leaves zero."""
    for t, what in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"),
                    (step, "step"), (done, "done")):
        require_device(t, what)
        if not t.is_contiguous():
            raise ValueError(f"adam_flat: {what} must be contiguous")
    n = params.numel()
    if any(t.numel() != n or t.dtype != torch.float32 for t in (grads, exp_avg, exp_avg_sq)) or \
            params.dtype != torch.float32 or step.dtype != torch.float32 or step.numel() < 1 or done.numel() * \
            done.element_size() < 4:
        raise ValueError("adam_flat: float32 buffers of one size, a float32 step and a 4-byte done counter")
    dev = params.device
    with torch.cuda.device(dev):
        check(lib().hf_adam_flat(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), n, ptr(step), ptr(done),
                                 float(lr), float(beta1), float(beta2), float(eps), stream_of(dev)))


OPT_NUM_STATS = _lib.HF_OPT_NUM_STATS


def adam_flat_workspace(n, dev):
    """hf_adam_flat_workspace_bytes of scratch (the norm's float64 partials) for
    adam_flat_ex on `dev`, as a float64 tensor."""
    nb = int(lib().hf_adam_flat_workspace_bytes(n))
    if nb < 0:
        raise ValueError(f"adam_flat workspace: need n >= 0 (n = {n})")
    return torch.empty(nb // 8, dtype=torch.float64, device=dev)


def adam_flat_ex(params, grads, exp_avg, exp_avg_sq, step, done, lr, beta1, beta2, eps, weight_decay=0.0,
                 max_norm=float("inf"), skip_nonfinite=False, ws=None, stats=None):
    """hf_adam_flat_ex: the guarded step on one flat float32 parameter buffer --
    clip_grad_norm_(max_norm) + torch.optim.AdamW(weight_decay) + the skip of a
    step whose gradient norm is not finite, in two launches without a host
    sync.  lr: a float, or a one-element float32 device tensor the kernel reads
    at launch time (so a captured step follows a scheduler).  ws:
    adam_flat_workspace(n) (needed for clipping, skipping and stats); stats:
    float32 [4] = (norm, coef, skipped, skipped so far), zeroed before the
    first step; the other arguments as adam_flat."""
    tensors = [(params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"),
               (step, "step"), (done, "done")]
    dev_lr = lr if isinstance(lr, torch.Tensor) else None
    tensors += [(t, what) for t, what in ((dev_lr, "lr"), (ws, "ws"), (stats, "stats")) if t is not None]
    dev = params.device
    for t, what in tensors:
        require_device(t, what)
        if not t.is_contiguous() or t.device != dev:
            raise ValueError(f"adam_flat_ex: {what} must be contiguous and on the parameters' device")
    n = params.numel()
    if any(t.numel() != n or t.dtype != torch.float32 for t in (grads, exp_avg, exp_avg_sq)) or \
            params.dtype != torch.float32 or step.dtype != torch.float32 or step.numel() < 1 or done.numel() * \
            done.element_size() < 4:
        raise ValueError("adam_flat_ex: float32 buffers of one size, a float32 step and a 4-byte done counter")
    if dev_lr is not None and (dev_lr.dtype != torch.float32 or dev_lr.numel() != 1):
        raise ValueError("adam_flat_ex: a tensor lr must hold one float32")
    if stats is not None and (stats.dtype != torch.float32 or stats.numel() < OPT_NUM_STATS):
        raise ValueError(f"adam_flat_ex: stats must hold {OPT_NUM_STATS} float32")
    if ws is not None and ws.numel() * ws.element_size() < int(lib().hf_adam_flat_workspace_bytes(n)):
        raise ValueError("adam_flat_ex: the workspace is smaller than hf_adam_flat_workspace_bytes(n)")
    with torch.cuda.device(dev):
        check(lib().hf_adam_flat_ex(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), n, ptr(step), ptr(done),
                                    ptr(dev_lr), 0.0 if dev_lr is not None else float(lr), float(beta1), float(beta2),
                                    float(eps), float(weight_decay), float(max_norm), int(bool(skip_nonfinite)),
                                    ptr(ws), ptr(stats), stream_of(dev)))


def unroll_workspace(B, nx, dev):
    """hf_unroll_workspace_bytes of scratch for unroll_update on `dev` (a uint8 tensor)."""
    nb = int(lib().hf_unroll_workspace_bytes(B, nx))
    if nb < 0:
        raise ValueError(f"unroll workspace: need B >= 1, nx >= 1 (B = {B}, nx = {nx})")
    return torch.empty(nb, dtype=torch.uint8, device=dev)


def _unroll_state(t, B, nx, dev, what):
    require_device(t, what)
    if t.dtype != torch.float32 or tuple(t.shape) != (B, 3, nx) or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous float32 [{B},3,{nx}] on {dev}, got {tuple(t.shape)} {t.dtype}")
    return t


def _weights3(weights):
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
    if w.size != 3:
        raise ValueError("channel weights must be (w_n, w_u, w_E)")
    return w


def state_moments(states):
    """hf_state_moments: (e, q) = (0.5 (sum u^2 + sum E^2) / nx, sum n / nx) of
    every state of `states` [..., 3, nx] (contiguous float32 on the device), in
    float64 [..., 2]: HF_NUM_METRICS [0] and [1] without the rounding to float32."""
    require_device(states, "states")
    if states.dim() < 3 or states.shape[-2] != 3 or states.shape[-1] < 1 or states.dtype != torch.float32 \
            or not states.is_contiguous():
        raise ValueError(f"states must be contiguous float32 [...,3,nx], got {tuple(states.shape)} {states.dtype}")
    rows, nx = states.numel() // (3 * states.shape[-1]), states.shape[-1]
    if rows < 1:
        raise ValueError("state moments: need at least one state")
    out = torch.empty(*states.shape[:-2], 2, dtype=torch.float64, device=states.device)
    with torch.cuda.device(states.device):
        check(lib().hf_state_moments(ptr(states), rows, nx, ptr(out), stream_of(states.device)))
    return out


def _cons_terms(what, cons, cons_scale, cons_ref, cons_coef, B, dev, target):
    """The conservation arguments of an _ex update: (lam [2] host float32,
    cons_scale, ref [B,2] float64, coef [B,2] float32 (allocated when None));
    cons None: no terms, (None, cons_scale, None, None)."""
    if cons is None:
        return None, float(cons_scale), None, None
    lam = np.ascontiguousarray(np.asarray(cons, dtype=np.float32).reshape(-1))
    if lam.size != 2 or not (lam >= 0).all():
        raise ValueError(f"{what}: cons must be (lam_e, lam_q), both >= 0")
    if target is None:
        raise ValueError(f"{what}: cons needs a target")
    if cons_ref is None or cons_ref.dtype != torch.float64 or tuple(cons_ref.shape) != (B, 2) or cons_ref.device != dev \
            or not cons_ref.is_contiguous():
        raise ValueError(f"{what}: cons_ref must be contiguous float64 [{B},2] on {dev}")
    cons_coef = torch.empty(B, 2, device=dev) if cons_coef is None else cons_coef
    _cons_coef(what, cons_coef, B, dev)
    return lam, float(cons_scale), cons_ref, cons_coef


def _cons_coef(what, coef, B, dev):
    if coef.dtype != torch.float32 or tuple(coef.shape) != (B, 2) or coef.device != dev or not coef.is_contiguous():
        raise ValueError(f"{what}: cons_coef must be contiguous float32 [{B},2] on {dev}")
    return coef


def _loss_row(what, loss, n, dev, text=None):
    """The loss row of an unrolled-training call, allocated when None.  text:
    what a plain call says of a wrong one (the _ex calls' message otherwise)."""
    loss = torch.empty(n, device=dev) if loss is None else loss
    if loss.dtype != torch.float32 or loss.numel() != n or loss.device != dev or not loss.is_contiguous():
        raise ValueError(f"{what}: "
                         + (text or f"loss must be {n} contiguous float32 element(s) on the state's device"))
    return loss


_ONE_LOSS = "loss must be one float32 element on the state's device"


def _adjoint_call(what, plain, ex_call, ex, cons_coef, B, dev):
    """The entry point of an unrolled-training adjoint and the argument it takes
    before the stream: the _ex one with cons_coef (checked; may be None) when
    ex or cons_coef is given, else the plain one with none."""
    if not ex and cons_coef is None:
        return plain, ()
    if cons_coef is not None:
        _cons_coef(what, cons_coef, B, dev)
    return ex_call, (ptr(cons_coef),)


def _ws_ex(query, B, nx, dev, what):
    nb = int(query(B, nx))
    if nb < 0:
        raise ValueError(f"{what}: need B >= 1, nx >= 1 (B = {B}, nx = {nx})")
    return torch.empty(nb, dtype=torch.uint8, device=dev)


def unroll_workspace_ex(B, nx, dev):
    """hf_unroll_workspace_bytes_ex of scratch for unroll_update with cons on `dev` (a uint8 tensor)."""
    return _ws_ex(lib().hf_unroll_workspace_bytes_ex, B, nx, dev, "unroll workspace")


def pure_unroll_workspace_ex(B, nx, dev):
    """hf_pure_unroll_workspace_bytes_ex of scratch for pure_unroll_update with cons on `dev` (a uint8 tensor)."""
    return _ws_ex(lib().hf_pure_unroll_workspace_bytes_ex, B, nx, dev, "pure unroll workspace")


def pinn_unroll_workspace_ex(B, nx, dev):
    """hf_pinn_unroll_workspace_bytes_ex of scratch for pinn_unroll_loss with cons on `dev` (a uint8 tensor)."""
    return _ws_ex(lib().hf_pinn_unroll_workspace_bytes_ex, B, nx, dev, "pinn unroll workspace")


def unroll_update(grid, flux_edge, state, x=None, target=None, weights=(1.0, 1.0, 1.0), scale=0.0, want_nf=True,
                  out=None, loss=None, ws=None, cons=None, cons_scale=0.0, cons_ref=None, cons_coef=None, ex=False):
    """hf_unroll_update: one hybrid step of `state` [B,3,nx] from FluxGNN's edge
    fluxes flux_edge [B*2nx] (src/hybrid_solver.py:45-63).  Returns (state_next
    [B,3,nx], node_features_next [B*nx,4] or None, loss [1] or None): the next
    step's FluxGNN input, and with `target` [B,3,nx] the term scale * sum w_ch
    (state_next - target)^2.  x: the positions [nx] of the node features
    (default the grid's).  out / loss / ws: preallocated state_next, loss
    element and workspace (unroll_workspace).  cons = (lam_e, lam_q) (or
    ex=True): hf_unroll_update_ex -- loss is the row [4] = (total, state, energy,
    charge) of the step with the energy and charge terms against cons_ref [B,2]
    float64 at cons_scale, the workspace unroll_workspace_ex's, and cons_coef
    [B,2] receives (ce, cq) for unroll_adjoint."""
    require_device(state, "state")
    B, _, nx = state.shape
    dev = state.device
    st = _unroll_state(state, B, nx, dev, "state")
    ex = ex or cons is not None
    call, nloss = (lib().hf_unroll_update_ex, 4) if ex else (lib().hf_unroll_update, 1)
    fe = flux_edge.detach()
    if fe.dtype != torch.float32 or fe.numel() != B * 2 * nx or fe.device != dev or not fe.is_contiguous() \
            or nx != grid.nx:
        raise ValueError(f"unroll update: flux_edge must be contiguous float32 [{B}*2*{nx}] on {dev}, nx the grid's")
    xg, _ = grid.on(dev)
    x = xg if x is None else x
    if x.dtype != torch.float32 or x.numel() != nx or x.device != dev or not x.is_contiguous():
        raise ValueError(f"unroll update: x must be contiguous float32 [{nx}] on {dev}")
    pc = grid.spectral_plan(dev)
    out = torch.empty_like(st) if out is None else _unroll_state(out, B, nx, dev, "out")
    nf = torch.empty(B * nx, 4, device=dev) if want_nf else None
    w = None
    if target is not None:
        target = _unroll_state(target, B, nx, dev, "target")
        w = _weights3(weights)
        loss = _loss_row("unroll update", loss, nloss, dev, None if ex else _ONE_LOSS)
    else:
        loss = None
    lam, cons_scale, cons_ref, cons_coef = _cons_terms("unroll update", cons, cons_scale, cons_ref, cons_coef, B, dev,
                                                       target)
    if ws is None:
        ws = unroll_workspace_ex(B, nx, dev) if cons is not None else unroll_workspace(B, nx, dev)
    extra = (ptr(lam), cons_scale, ptr(cons_ref), ptr(cons_coef)) if ex else ()
    with torch.cuda.device(dev):
        check(call(ptr(fe), ptr(st), ptr(x), ptr(pc), grid.pmode, B, nx, grid.c32, grid.dt32, ptr(out), ptr(nf),
                   ptr(target), ptr(w), float(scale), ptr(loss), ptr(ws), ws.numel() * ws.element_size(), *extra,
                   stream_of(dev)))
    return out, nf, loss


def unroll_adjoint(grid, state, state_next, target, weights, scale, direct_next=None, gnf_next=None, want_direct=True,
                   cons_coef=None, ex=False):
    """hf_unroll_adjoint: the adjoint of unroll_update's step.  state (s_k),
    state_next (the predicted s_{k+1}) and target (s*_{k+1}) [B,3,nx];
    direct_next [B,3,nx] / gnf_next [B*nx,4]: the direct part this call returned
    for step k+1 and FluxGNN's d node_features of step k+1 (None at the last
    step, or to cut the state gradient).  Returns (d loss / d flux_edge [B,2nx],
    direct part [B,3,nx] or None).  cons_coef [B,2] (or ex=True):
    hf_unroll_adjoint_ex, the seed with the energy term's ce u, ce E."""
    require_device(state, "state")
    B, _, nx = state.shape
    dev = state.device
    st = _unroll_state(state, B, nx, dev, "state")
    sn = _unroll_state(state_next, B, nx, dev, "state_next")
    tg = _unroll_state(target, B, nx, dev, "target")
    if nx != grid.nx:
        raise ValueError("unroll adjoint: nx must be the grid's")
    if direct_next is not None:
        direct_next = _unroll_state(direct_next, B, nx, dev, "direct_next")
    if gnf_next is not None and (gnf_next.dtype != torch.float32 or tuple(gnf_next.shape) != (B * nx, 4)
                                 or gnf_next.device != dev or not gnf_next.is_contiguous()):
        raise ValueError(f"unroll adjoint: gnf_next must be contiguous float32 [{B * nx},4] on {dev}")
    w = _weights3(weights)
    pc = grid.spectral_plan(dev)
    g_fe = torch.empty(B, 2 * nx, device=dev)
    direct = torch.empty(B, 3, nx, device=dev) if want_direct else None
    call, extra = _adjoint_call("unroll adjoint", lib().hf_unroll_adjoint, lib().hf_unroll_adjoint_ex, ex, cons_coef, B,
                                dev)
    with torch.cuda.device(dev):
        check(call(ptr(st), ptr(sn), ptr(tg), ptr(w), float(scale), ptr(direct_next), ptr(gnf_next), ptr(pc),
                   grid.pmode, B, nx, grid.c32, grid.dt32, ptr(g_fe), ptr(direct), *extra, stream_of(dev)))
    return g_fe, direct


def pure_unroll_workspace(B, nx, dev):
    """hf_pure_unroll_workspace_bytes of scratch for pure_unroll_update on `dev` (a uint8 tensor)."""
    nb = int(lib().hf_pure_unroll_workspace_bytes(B, nx))
    if nb < 0:
        raise ValueError(f"pure unroll workspace: need B >= 1, nx >= 1 (B = {B}, nx = {nx})")
    return torch.empty(nb, dtype=torch.uint8, device=dev)


def _unroll_cells(t, B, nx, width, dev, what):
    """A per-cell tensor [B*nx, width] of the PureGNN side (delta, node features and their gradients)."""
    require_device(t, what)
    if t.dtype != torch.float32 or tuple(t.shape) != (B * nx, width) or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous float32 [{B * nx},{width}] on {dev}, got {tuple(t.shape)} "
                         f"{t.dtype}")
    return t


def pure_unroll_update(delta, state, x, target=None, weights=(1.0, 1.0, 1.0), scale=0.0, want_nf=True, out=None,
                       loss=None, ws=None, cons=None, cons_scale=0.0, cons_ref=None, cons_coef=None, ex=False):
    """hf_pure_unroll_update: one step of PureGNN's rollout, state_next = state
    + delta^T for `state` [B,3,nx] and PureGNN's delta [B*nx,3]
    (evaluate_multi_ic.py:53-64).  Returns (state_next [B,3,nx],
    node_features_next [B*nx,4] = [n', u', E', x] or None, loss [1] or None):
    the next step's PureGNN input, and with `target` [B,3,nx] the term scale *
    sum w_ch (state_next - target)^2.  x: the positions [nx].  out / loss / ws:
    preallocated state_next, loss element and workspace (pure_unroll_workspace).
    cons = (lam_e, lam_q) (or ex=True): hf_pure_unroll_update_ex, as
    unroll_update's (loss row [4], pure_unroll_workspace_ex, cons_ref, cons_coef)."""
    require_device(state, "state")
    ex = ex or cons is not None
    call, nloss = (lib().hf_pure_unroll_update_ex, 4) if ex else (lib().hf_pure_unroll_update, 1)
    if state.dim() != 3:
        raise ValueError(f"state must be [B,3,nx], got {tuple(state.shape)}")
    B, _, nx = state.shape
    dev = state.device
    st = _unroll_state(state, B, nx, dev, "state")
    d = _unroll_cells(delta.detach(), B, nx, 3, dev, "delta")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.numel() != nx or x.device != dev \
            or not x.is_contiguous():
        raise ValueError(f"pure unroll update: x must be contiguous float32 [{nx}] on {dev}")
    out = torch.empty_like(st) if out is None else _unroll_state(out, B, nx, dev, "out")
    nf = torch.empty(B * nx, 4, device=dev) if want_nf else None
    w, nb = None, 0
    if target is not None:
        target = _unroll_state(target, B, nx, dev, "target")
        w = _weights3(weights)
        loss = _loss_row("pure unroll update", loss, nloss, dev, None if ex else _ONE_LOSS)
        if ws is None:
            ws = pure_unroll_workspace_ex(B, nx, dev) if cons is not None else pure_unroll_workspace(B, nx, dev)
        if ws.device != dev or not ws.is_contiguous():
            raise ValueError(f"pure unroll update: the workspace must be contiguous on {dev}")
        nb = ws.numel() * ws.element_size()
    else:
        loss = ws = None
    lam, cons_scale, cons_ref, cons_coef = _cons_terms("pure unroll update", cons, cons_scale, cons_ref, cons_coef, B,
                                                       dev, target)
    extra = (ptr(lam), cons_scale, ptr(cons_ref), ptr(cons_coef)) if ex else ()
    with torch.cuda.device(dev):
        check(call(ptr(d), ptr(st), ptr(x), B, nx, ptr(out), ptr(nf), ptr(target), ptr(w), float(scale), ptr(loss),
                   ptr(ws), nb, *extra, stream_of(dev)))
    return out, nf, loss


def pure_unroll_adjoint(state_next, target, weights, scale, grad_delta_next=None, gnf_next=None, cons_coef=None,
                        ex=False):
    """hf_pure_unroll_adjoint: the adjoint of pure_unroll_update's step.
    state_next (the predicted s_{k+1}) and target (s*_{k+1}) [B,3,nx];
    grad_delta_next [B*nx,3] / gnf_next [B*nx,4]: what this call returned for
    step k+1 and PureGNN's d node_features of step k+1 (None at the last step,
    or to cut the state gradient).  Returns d loss / d delta [B*nx,3].
    cons_coef [B,2] (or ex=True): hf_pure_unroll_adjoint_ex, the seed with the
    terms' (cq, ce u, ce E)."""
    require_device(state_next, "state_next")
    if state_next.dim() != 3:
        raise ValueError(f"state_next must be [B,3,nx], got {tuple(state_next.shape)}")
    B, _, nx = state_next.shape
    dev = state_next.device
    sn = _unroll_state(state_next, B, nx, dev, "state_next")
    tg = _unroll_state(target, B, nx, dev, "target")
    if grad_delta_next is not None:
        grad_delta_next = _unroll_cells(grad_delta_next, B, nx, 3, dev, "grad_delta_next")
    if gnf_next is not None:
        gnf_next = _unroll_cells(gnf_next, B, nx, 4, dev, "gnf_next")
    w = _weights3(weights)
    gd = torch.empty(B * nx, 3, device=dev)
    call, extra = _adjoint_call("pure unroll adjoint", lib().hf_pure_unroll_adjoint, lib().hf_pure_unroll_adjoint_ex,
                                ex, cons_coef, B, dev)
    with torch.cuda.device(dev):
        check(call(ptr(sn), ptr(tg), ptr(w), float(scale), ptr(grad_delta_next), ptr(gnf_next), B, nx, ptr(gd), *extra,
                   stream_of(dev)))
    return gd


def pinn_unroll_workspace(B, nx, dev):
    """hf_pinn_unroll_workspace_bytes of scratch for pinn_unroll_loss on `dev` (a uint8 tensor)."""
    nb = int(lib().hf_pinn_unroll_workspace_bytes(B, nx))
    if nb < 0:
        raise ValueError(f"pinn unroll workspace: need B >= 1, nx >= 1 (B = {B}, nx = {nx})")
    return torch.empty(nb, dtype=torch.uint8, device=dev)


def _pinn_unroll_args(what, pred, target, weights, state, phys, phys_scale, dx, dt, nu, length):
    """The arguments hf_pinn_unroll_loss and hf_pinn_unroll_adjoint share:
    (pred, target, state or None, B, nx, dev, w, lam or None, phys_scale, dt,
    dx, nu, plan or None).  phys = (l_c, l_m, l_p) needs state, dx, dt, nu."""
    require_device(pred, "pred")
    if pred.dim() != 3:
        raise ValueError(f"{what}: pred must be [B,3,nx], got {tuple(pred.shape)}")
    B, _, nx = pred.shape
    dev = pred.device
    p = _unroll_state(pred, B, nx, dev, "pred")
    tg = _unroll_state(target, B, nx, dev, "target")
    w = _weights3(weights)
    if phys is None:
        return p, tg, None, B, nx, dev, w, None, 0.0, 1.0, 1.0, 0.0, None
    lam = np.ascontiguousarray(np.asarray(phys, dtype=np.float32).reshape(-1))
    if lam.size != 3:
        raise ValueError(f"{what}: phys must be (l_continuity, l_momentum, l_poisson)")
    if state is None or dx is None or dt is None or nu is None:
        raise ValueError(f"{what}: phys needs state, dx, dt and nu")
    st = _unroll_state(state, B, nx, dev, "state")
    pc = pinn_loss_plan(nx, nx * float(dx) if length is None else length, dev)
    return p, tg, st, B, nx, dev, w, lam, float(phys_scale), float(dt), float(dx), float(nu), pc


def pinn_unroll_loss(pred, target, weights, scale, state=None, phys=None, phys_scale=0.0, dx=None, dt=None, nu=None,
                     length=None, losses=None, ws=None, cons=None, cons_scale=0.0, cons_ref=None, cons_coef=None,
                     ex=False):
    """hf_pinn_unroll_loss: one step's term of PINN's K-step loss, losses [5] =
    (total, data, cont, mom, pois) with data = scale sum w_ch (pred - target)^2
    and, with phys = (l_c, l_m, l_p), phys_scale l sum r^2 of hf_pinn_loss's
    residuals at p = pred, (n, u, E) = state; all states contiguous float32
    [B,3,nx] on pred's device.  phys None: entries 2..4 are 0 and state is not
    read.  length: the domain length of the Poisson operator (default nx dx).
    losses / ws: a preallocated float32 [5] and workspace (pinn_unroll_workspace).
    cons = (lam_e, lam_q) (or ex=True): hf_pinn_unroll_loss_ex -- losses [7] =
    (..., energy, charge) with the energy and charge terms against cons_ref [B,2]
    float64 at cons_scale, the workspace pinn_unroll_workspace_ex's, and cons_coef
    [B,2] receives (ce, cq) for pinn_unroll_adjoint."""
    p, tg, st, B, nx, dev, w, lam, phys_scale, dt, dx, nu, pc = _pinn_unroll_args(
        "pinn_unroll_loss", pred, target, weights, state, phys, phys_scale, dx, dt, nu, length)
    ex = ex or cons is not None
    call, nloss = (lib().hf_pinn_unroll_loss_ex, 7) if ex else (lib().hf_pinn_unroll_loss, 5)
    losses = _loss_row("pinn_unroll_loss", losses, nloss, dev,
                       None if ex else "losses must be five contiguous float32 elements on pred's device")
    clam, cons_scale, cons_ref, cons_coef = _cons_terms("pinn_unroll_loss", cons, cons_scale, cons_ref, cons_coef, B,
                                                        dev, tg)
    if ws is None:
        ws = pinn_unroll_workspace_ex(B, nx, dev) if cons is not None else pinn_unroll_workspace(B, nx, dev)
    if ws.device != dev or not ws.is_contiguous():
        raise ValueError(f"pinn_unroll_loss: the workspace must be contiguous on {dev}")
    extra = (ptr(clam), cons_scale, ptr(cons_ref), ptr(cons_coef)) if ex else ()
    with torch.cuda.device(dev):
        check(call(ptr(p), ptr(st), ptr(tg), B, nx, ptr(w), float(scale), ptr(lam), phys_scale, dt, dx, nu, ptr(pc),
                   ptr(losses), ptr(ws), ws.numel() * ws.element_size(), *extra, stream_of(dev)))
    return losses


def pinn_unroll_adjoint(pred, target, weights, scale, state=None, phys=None, phys_scale=0.0, dx=None, dt=None, nu=None,
                        length=None, pred_next=None, grad_state_next=None, cons_coef=None, ex=False):
    """hf_pinn_unroll_adjoint: step k's incoming gradient [B,3,nx] for
    pinn_backward = d term_k / d pred (pinn_unroll_loss's arguments), + with
    phys and pred_next (s^_{k+1}) d term_{k+1} / d (state slot), +
    grad_state_next (pinn_backward's d state of step k+1); pred_next and
    grad_state_next None at the last step, or to cut the state gradient.
    cons_coef [B,2] (or ex=True): hf_pinn_unroll_adjoint_ex, d term_k / d pred
    with the terms' (cq, ce p_u, ce p_E)."""
    p, tg, st, B, nx, dev, w, lam, phys_scale, dt, dx, nu, pc = _pinn_unroll_args(
        "pinn_unroll_adjoint", pred, target, weights, state, phys, phys_scale, dx, dt, nu, length)
    if pred_next is not None:
        pred_next = _unroll_state(pred_next, B, nx, dev, "pred_next")
    if grad_state_next is not None:
        grad_state_next = _unroll_state(grad_state_next, B, nx, dev, "grad_state_next")
    g = torch.empty(B, 3, nx, device=dev)
    call, extra = _adjoint_call("pinn_unroll_adjoint", lib().hf_pinn_unroll_adjoint, lib().hf_pinn_unroll_adjoint_ex,
                                ex, cons_coef, B, dev)
    with torch.cuda.device(dev):
        check(call(ptr(p), ptr(st), ptr(tg), ptr(pred_next), ptr(grad_state_next), B, nx, ptr(w), float(scale),
                   ptr(lam), phys_scale, dt, dx, nu, ptr(pc), ptr(g), *extra, stream_of(dev)))
    return g


def ablation_loss_terms(grid, flux_edge, st, ft, sn, lam, rollout_steps=0, dt=None):
    """hf_ablation_loss_ex: the reference trainer's loss (scripts/training/
    train_ablation.py:120-206) for B samples.  flux_edge [B, 2nx], st / sn
    [B,3,nx], ft [B,nx] device tensors; lam = (lambda_state, lambda_poisson,
    lambda_charge, lambda_energy_one[, lambda_energy_multi]); with
    lambda_energy_multi > 0 and 0 < rollout_steps <= 3 the rollout energy term
    (:172-206) is formed in the same pass from the main forward's flux (no
    further model forward reaches it; include/hybridflux.h), with time step dt
    (default the grid's).  Returns (loss, flux MSE, d loss / d flux_edge [B, 2nx])."""
    for t, what in ((flux_edge, "flux_edge"), (st, "state_t"), (ft, "flux_t"), (sn, "state_next")):
        require_device(t, what)
    B, _, nx = st.shape
    dev = st.device
    fe = flux_edge.detach().to(torch.float32).contiguous()
    st, ft, sn = (t.to(torch.float32).contiguous() for t in (st, ft, sn))
    if fe.numel() != B * 2 * nx or ft.shape != (B, nx) or sn.shape != st.shape or nx != grid.nx:
        raise ValueError("ablation loss: shapes must be flux_edge [B,2nx], states [B,3,nx], flux_t [B,nx]")
    loss = torch.empty((), device=dev)
    fl = torch.empty((), device=dev)
    dfe = torch.empty(B, 2 * nx, device=dev)
    ws = torch.empty(int(lib().hf_ablation_loss_workspace_bytes(B, nx)), dtype=torch.uint8, device=dev)
    lam_h = np.zeros(5, dtype=np.float32)
    lam_h[:len(lam)] = np.asarray(lam, dtype=np.float32)
    dt32 = float(np.float32(grid.dt if dt is None else dt))
    pc = grid.spectral_plan(dev)
    with torch.cuda.device(dev):
        check(lib().hf_ablation_loss_ex(ptr(fe), ptr(st), ptr(ft), ptr(sn), B, nx, grid.c32,
                                        float(np.float32(grid.dx)), ptr(lam_h), int(rollout_steps), dt32, ptr(pc),
                                        ptr(loss), ptr(fl), ptr(dfe), ptr(ws), ws.numel(), stream_of(dev)))
    return loss, fl, dfe
