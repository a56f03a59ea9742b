"""GPU parity of unrolled training (hf_unroll_update, hf_unroll_adjoint,
hybridflux.training.unrolled_loss / unrolled_step / train_unrolled): FluxGNN
differentiated through K hybrid solver steps, against the CPU oracle and
torch-CPU float64 autograd of the same K-step loss.

Tolerances:
  one update given the edge fluxes ...... atol 1e-7 per channel (test_gpu_parity's
      gate on a single hybrid step); bit-equal to hf_step's finite-volume update
  step loss ............................. rtol 1e-6 (an elementwise float32
      difference, squared and summed in float64: <= 2 ulp of float32 relative)
  adjoint kernel alone .................. 2e-5 max|ref| + 1e-12 max|g| per tensor
      (test_gpu_training's gradient gate: elementwise float32 expressions and one
      float64 Poisson sum rounded to float32)
  K-step loss value ..................... 2 sqrt(L) K ulp(max|state|): L = mean d^2 moves by
      at most 2 sqrt(L) rms(delta), and each float32 step moves a state by ~1 ulp
  K-step parameter gradients ............ per tensor max(4 d32, 2e-5 max|g64|), d32 the
      error of the same gradient in torch-CPU float32 (measured in the test: the
      split-K partials are summed in another order than the CPU BLAS's, factor 4)
  predicted states, K = 4 ............... atol 2e-6 + rtol 2e-6 (test_gpu_parity's gate
      on hybrid rollouts)
Every measured error is recorded (conftest `record` / close).

Sizes: the update, its loss term and the adjoint run over SHAPES (nx <= 256) and
nx_regimes.UNROLL_WIDE: every FFT instantiation (256, 512, 1024, 2048; a lone IC,
odd IC counts, one IC past a workgroup, two workgroups of the 2048 kernel) and the
circulant kernels at 257, 1000, 4096 and their LDS limit 6144; the bit-for-bit
comparison with hf_step at 100, 256, 257, 512, 1024, 2048, 6144; the K-step
gradients up to 100 with the trained model and at 512, 2048, 6144 with
FluxGNN(4, 64, 2).  Beyond 256 cells dt shrinks with dx (dt_for), which keeps the
values O(1) and the gates unchanged.  E of one update is float32 on both sides and
reaches [0.5, 1), where one ulp is 5.96e-8: a last-bit difference from the oracle's
own rounding is 0.596 of the 1e-7 gate, at nx = 48 as at 6144 (n and u: equal bits)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import close, golden
from nx_regimes import UNROLL_WIDE, UNROLLED_GRAD_WIDE, UPDATE_BITWISE_WIDE, dt_of
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_ATOL = 1e-7
ROLL_ATOL, ROLL_RTOL = 2e-6, 2e-6
REL = 2e-5
# (nx, B): circulant sizes with one cell, two cells, one wave, part of a wave, more
# than a wave, the smallest FFT size with an odd IC count, and one IC more than a
# workgroup of the FFT kernel holds (4 waves x 2 ICs)
SHAPES = [(1, 2), (2, 3), (16, 3), (48, 3), (100, 3), (256, 3), (256, 9)]


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


def w1r2():
    w = golden("weights_W1_r2.npz")
    return {k: w[k] for k in w.files}


def rand_sd64(layers, seed):
    """conftest.rand_sd's distributions at hidden 64 (the chain GEMM training path)."""
    H = 64
    g = np.random.default_rng(seed)
    sd = {"input_mlp.0.weight": g.normal(0, 0.5, (H, 4)), "input_mlp.0.bias": g.normal(0, 0.1, H)}
    for l in range(layers):
        sd[f"update_mlps.{l}.0.weight"] = g.normal(0, 1 / 11, (H, 2 * H))
        sd[f"update_mlps.{l}.0.bias"] = g.normal(0, 0.1, H)
    sd["edge_mlp.0.weight"] = g.normal(0, 1 / 11, (H, 2 * H))
    sd["edge_mlp.0.bias"] = g.normal(0, 0.1, H)
    sd["edge_mlp.2.weight"] = g.normal(0, 1 / 8, (1, H))
    sd["edge_mlp.2.bias"] = g.normal(0, 0.1, 1)
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


def load(hf, sd, dims=(4, 128, 4)):
    m = hf.FluxGNN(*dims)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(DEV)


def dt_for(nx):
    """The reference's 5e-3 at the sizes up to 256 (the cases first written here, kept
    as they were); beyond, nx_regimes.dt_of: the same dt / dx as at nx = 64, so that
    the values, and with them what an absolute gate means, keep their size."""
    return 5e-3 if nx <= 256 else dt_of(nx)


_GRIDS = {}


def grid_of(hf, nx):
    """The engine grid of nx at dt_for(nx), built once (the host builds the circulant
    column in O(nx^2): seconds at 6144) and shared; nothing here changes a grid."""
    if nx not in _GRIDS:
        _GRIDS[nx] = hf.BaselineSolver(nx, dt=dt_for(nx), device=DEV).grid
    return _GRIDS[nx]


def ics(nx, B, seed0=0):
    G = O.Grid(nx, dt=dt_for(nx))
    return G, np.stack([O.initial_condition(G, seed0 + s) for s in range(B)])


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


# ------------------------------------------------- the section 1 step in torch (CPU)
def poisson_t(n, k):
    """Differentiable spectral solve (src/baseline_solver.py:59-68) in n's dtype."""
    rh = torch.fft.fft(n - 1.0, dim=-1)
    keep = k != 0
    Eh = torch.zeros_like(rh)
    Eh[..., keep] = 1j * rh[..., keep] / k[keep]
    return torch.fft.ifft(Eh, dim=-1).real


def step_t(st, fe, c, dt, k):
    nx = st.shape[-1]
    n, u, E = st[:, 0], st[:, 1], st[:, 2]
    F = 0.5 * (fe[:, :nx] + fe[:, nx:])
    n1 = n - c * (F - torch.roll(F, 1, -1))
    Fu = 0.5 * u * u
    u1 = u - c * (Fu - torch.roll(Fu, 1, -1)) + dt * E
    return torch.stack([n1, u1, poisson_t(n1, k)], dim=1)


def consts(G, dtype):
    """c = f32(dt/dx), dt = f32(dt) (the kernels' scalars) and k, x in dtype."""
    return (float(np.float32(G.dt / G.dx)), float(np.float32(G.dt)), torch.as_tensor(G.k, dtype=dtype),
            torch.as_tensor(G.x.astype(np.float32), dtype=dtype))


def unrolled_loss_cpu(sd, G, traj, w, dtype, through=True):
    """The K-step loss of oracle.flux_gnn_forward and step_t in torch-CPU `dtype`;
    returns (loss, {name: grad})."""
    p = {k: torch.as_tensor(v, dtype=dtype).clone().requires_grad_(True) for k, v in sd.items()}
    c, dt, k, x = consts(G, dtype)
    tr = torch.as_tensor(traj, dtype=dtype)
    B, K1, _, nx = tr.shape
    ei = O.chain_edges(nx, B)
    wt = torch.as_tensor(w, dtype=dtype)[None, :, None]
    st, L = tr[:, 0], 0.0
    for j in range(1, K1):
        nf = torch.stack([st[:, 0], st[:, 1], st[:, 2], x.expand(B, nx)], dim=-1).reshape(B * nx, 4)
        fe = O.flux_gnn_forward(p, nf, ei).reshape(B, 2 * nx)
        st = step_t(st, fe, c, dt, k)
        L = L + (wt * (st - tr[:, j]) ** 2).mean() / (K1 - 1)
        if not through:
            st = st.detach()
    L.backward()
    return float(L.detach()), {k: v.grad.numpy().astype(np.float64) for k, v in p.items()}


# ------------------------------------------------------------------ 1. update forward
@pytest.mark.parametrize("nx,B", SHAPES + UNROLL_WIDE)
def test_update_vs_oracle(hf, nx, B):
    from hybridflux import engine
    G, st = ics(nx, B)
    fe = np.random.default_rng(nx * 100 + B).normal(0, 0.3, (B, 2 * nx)).astype(np.float32)
    grid = grid_of(hf, nx)
    out, nf, loss = engine.unroll_update(grid, dev(fe).reshape(-1), dev(st))
    assert loss is None
    want, _ = O.hybrid_update(G, st, fe)
    got = out.cpu().numpy()
    for ch, name in enumerate("nuE"):
        close(got[:, ch], want[:, ch], STEP_ATOL, what=name)
    x, _ = grid.on(torch.device(DEV))
    nf_want, _ = hf.build_chain_graph_batch(out, x)
    assert torch.equal(nf, nf_want)
    out2, nf2, _ = engine.unroll_update(grid, dev(fe).reshape(-1), dev(st), want_nf=False)
    assert nf2 is None and torch.equal(out2, out)


@pytest.mark.parametrize("nx,B", [(100, 3), (256, 3), (256, 9)] + UPDATE_BITWISE_WIDE)
def test_update_bitwise_equals_step(hf, nx, B):
    """At the chain lengths where hf_step is the flux kernel followed by the
    finite-volume kernel on its face flux, the update on the same model's edge
    fluxes gives hf_step's state bit for bit (shared device functions):
    fv_step_kernel<true> up to the LDS limit 6144, fv_step_fft_kernel<true> at
    each of the FFT sizes 256, 512, 1024 and 2048."""
    from hybridflux import engine
    _, st = ics(nx, B, seed0=5)
    m = load(hf, w1r2()).eval()
    grid = grid_of(hf, nx)
    std = dev(st)
    x, _ = grid.on(std.device)
    nf, _ = hf.build_chain_graph_batch(std, x)
    dm = m.device_model(std.device)
    fe = engine.chain_flux(dm, nf, B, nx)
    want, _, _ = engine.step(dm, grid, std)
    got, _, _ = engine.unroll_update(grid, fe, std)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------- 2. loss term
@pytest.mark.parametrize("nx,B", [(16, 3), (100, 3), (256, 9), (64, 300)] + UNROLL_WIDE)
def test_step_loss(hf, nx, B):
    from hybridflux import engine
    G, st = ics(nx, min(B, 4))
    st = np.tile(st, ((B + 3) // 4, 1, 1))[:B]
    g = np.random.default_rng(7)
    st = (st + g.normal(0, 0.01, st.shape)).astype(np.float32)
    fe = g.normal(0, 0.3, (B, 2 * nx)).astype(np.float32)
    tgt = (st + g.normal(0, 0.05, st.shape)).astype(np.float32)
    w, K = (1.0, 0.5, 2.0), 4
    grid = grid_of(hf, nx)
    scale = 1.0 / (K * 3 * B * nx)
    runs = []
    for _ in range(2):
        out, _, loss = engine.unroll_update(grid, dev(fe).reshape(-1), dev(st), target=dev(tgt), weights=w, scale=scale)
        runs.append(loss.cpu().numpy().copy())
    pred = out.cpu().numpy().astype(np.float64)
    want = (np.asarray(w)[None, :, None] * (pred - tgt.astype(np.float64)) ** 2).mean() / K
    close(runs[0], np.asarray([want]), 0.0, 1e-6, what="loss")
    assert np.array_equal(runs[0], runs[1])


# ----------------------------------------------------------------- 3. adjoint alone
def adjoint_case(hf, nx, B, mode):
    from hybridflux import engine
    G, st = ics(nx, B, seed0=3)
    g = np.random.default_rng(nx * 10 + B)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    sn = f32(st + g.normal(0, 0.05, st.shape))
    tg = f32(st + g.normal(0, 0.05, st.shape))
    din = f32(g.normal(0, 1e-3, st.shape))
    gnf = f32(g.normal(0, 1e-3, (B * nx, 4)))
    w, scale = (1.0, 0.5, 2.0), 1.0 / (4 * 3 * B * nx)
    if mode == "e_only":  # only the E gradient is non-zero: a dropped Poisson term cannot hide
        tg = sn.copy()
        gnf[:] = 0
        din[:, :2] = 0
    if mode == "last":
        din_d = gnf_d = None
    else:
        din_d, gnf_d = dev(din), dev(gnf)
    grid = grid_of(hf, nx)
    g_fe, direct = engine.unroll_adjoint(grid, dev(st), dev(sn), dev(tg), w, scale, din_d, gnf_d)
    # reference: float64 autograd of sum(g * step(st, fe)) with fe a free tensor
    gt = 2.0 * np.asarray(w)[None, :, None] * scale * (sn.astype(np.float64) - tg)
    if mode != "last":
        gt = gt + din + gnf.astype(np.float64).reshape(B, nx, 4)[:, :, :3].transpose(0, 2, 1)
    c, dt, k, _ = consts(G, torch.float64)
    s64 = torch.as_tensor(st, dtype=torch.float64).requires_grad_(True)
    fe = torch.zeros(B, 2 * nx, dtype=torch.float64, requires_grad=True)
    (torch.as_tensor(gt) * step_t(s64, fe, c, dt, k)).sum().backward()
    return g_fe.cpu().numpy(), direct.cpu().numpy(), fe.grad.numpy(), s64.grad.numpy(), float(np.abs(gt).max())


@pytest.mark.parametrize("mode", ["full", "last", "e_only"])
@pytest.mark.parametrize("nx,B", SHAPES + UNROLL_WIDE)
def test_adjoint_vs_autograd(hf, record, nx, B, mode):
    g_fe, direct, want_fe, want_d, gmax = adjoint_case(hf, nx, B, mode)
    name = f"test_adjoint_vs_autograd[{nx}-{B}-{mode}]"
    for tag, got, want in (("g_fe", g_fe, want_fe), ("direct", direct, want_d)):
        err = float(np.abs(got.astype(np.float64) - want).max())
        lim = REL * float(np.abs(want).max()) + 1e-12 * gmax
        record(name, f"{tag}_err", err)
        record(name, f"{tag}_limit", lim)
        assert np.isfinite(got).all() and err <= lim, (tag, err, lim)
    if mode == "e_only" and nx > 2:
        assert np.abs(want_fe).max() > 0  # the case does exercise P^T


# --------------------------------------------------------- 4. K-step parameter gradients
def classical_windows(G, B, K):
    _, st = ics(G.nx, B)
    traj, _ = O.classical_run(G, st, K)  # [B,K+1,3,nx], seeds 0..B-1
    return traj


_GRAD_CASES = [(64, 3, 1, 128), (64, 3, 4, 128), (16, 3, 4, 128), (48, 2, 2, 128), (100, 2, 2, 64)]
_GRAD_CASES += [(nx, B, 2, 64) for nx, B in UNROLLED_GRAD_WIDE]  # FluxGNN(4, 64, 2), K = 2
_REF = {}


def grad_reference(nx, B, K, hidden, through):
    """(sd, dims, traj, g64, g32), computed once per case and left unchanged."""
    key = (nx, B, K, hidden, through)
    if key not in _REF:
        G = O.Grid(nx, dt=dt_for(nx))
        sd, dims = (w1r2(), (4, 128, 4)) if hidden == 128 else (rand_sd64(2, 11), (4, 64, 2))
        traj = classical_windows(G, B, K)
        w = (1.0, 1.0, 1.0)
        l64, g64 = unrolled_loss_cpu(sd, G, traj, w, torch.float64, through)
        _, g32 = unrolled_loss_cpu(sd, G, traj, w, torch.float32, through)
        _REF[key] = (sd, dims, traj, l64, g64, g32)
    return _REF[key]


def gpu_grads(hf, sd, dims, traj, nx, through):
    from hybridflux import training
    m = load(hf, sd, dims)
    grid = grid_of(hf, nx)
    x, _ = grid.on(torch.device(DEV))
    loss = training.unrolled_loss(m, dev(traj), x, grid, through_state=through)
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("through", [True, False])
@pytest.mark.parametrize("nx,B,K,hidden", _GRAD_CASES)
def test_unrolled_gradients(hf, record, nx, B, K, hidden, through):
    sd, dims, traj, l64, g64, g32 = grad_reference(nx, B, K, hidden, through)
    loss, got = gpu_grads(hf, sd, dims, traj, nx, through)
    name = f"test_unrolled_gradients[{nx}-{B}-{K}-{hidden}-{through}]"
    record(name, "loss", loss)
    record(name, "loss_rel_err", abs(loss - l64) / abs(l64))
    # L = mean d^2, so |dL| <= 2 sqrt(L) rms(delta); each of the K float32 steps moves a
    # predicted value by at most about one ulp of the largest state
    assert abs(loss - l64) <= 2 * np.sqrt(l64) * K * 2.0 ** -23 * float(np.abs(traj).max())
    others = max(float(np.abs(v).max()) for k, v in g64.items() if k != "edge_mlp.2.bias")
    for k, want in g64.items():
        err = float(np.abs(got[k].astype(np.float64) - want).max())
        scale = float(np.abs(want).max())
        d32 = float(np.abs(g32[k] - want).max())
        record(name, f"{k}_err", err)
        record(name, f"{k}_d32", d32)
        record(name, f"{k}_max", scale)
        assert np.isfinite(got[k]).all()
        if k == "edge_mlp.2.bias":  # analytically 0: a constant edge flux cancels in F_i - F_{i-1}
            assert float(np.abs(got[k]).max()) <= 1e-6 * others, (k, got[k], others)
        else:
            assert err <= max(4 * d32, REL * scale), (k, err, d32, scale)


def test_k1_same_gradient_in_both_modes(hf):
    sd, dims, traj, *_ = grad_reference(64, 3, 1, 128, True)
    _, a = gpu_grads(hf, sd, dims, traj, 64, True)
    _, b = gpu_grads(hf, sd, dims, traj, 64, False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------- 5. rollout consistency
def test_predicted_states_vs_oracle(hf):
    from hybridflux import training
    nx, B, K = 64, 3, 4
    G = O.Grid(nx)
    sd = w1r2()
    traj = classical_windows(G, B, K)
    m = load(hf, sd)
    grid = grid_of(hf, nx)
    x, _ = grid.on(torch.device(DEV))
    _, pred = training.unrolled_loss(m, dev(traj), x, grid, return_states=True)
    assert not pred.requires_grad and tuple(pred.shape) == (K, B, 3, nx)
    want, _ = O.hybrid_run(O.params_from(sd), G, traj[:, 0], K)
    close(pred.permute(1, 0, 2, 3).cpu().numpy(), want[:, 1:], ROLL_ATOL, ROLL_RTOL, what="states")


# ------------------------------------------------------ 6. direct step vs autograd step
@pytest.mark.parametrize("through", [True, False])
def test_direct_step_equals_autograd_step(hf, through):
    """unrolled_step and unrolled_loss -> backward -> FlatAdam.step() run the same
    launches and add the K parameter gradients in the same order (last step
    first): the parameters agree bit for bit, and so do two direct steps."""
    from hybridflux import training
    nx, B, K = 64, 3, 4
    traj = dev(classical_windows(O.Grid(nx), B, K))
    grid = grid_of(hf, nx)
    x, _ = grid.on(torch.device(DEV))

    def fresh():
        m = load(hf, w1r2()).flatten_parameters_()
        return m, training.FlatAdam(m.parameters(), lr=1e-3)

    outs = []
    for _ in range(2):
        m, opt = fresh()
        loss = training.unrolled_step(m, opt, traj, x, grid, through_state=through)
        assert loss is not None and not loss.requires_grad
        outs.append((float(loss), torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()))
    m, opt = fresh()
    before = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()
    la = training.unrolled_loss(m, traj, x, grid, through_state=through)
    opt.zero_grad()
    la.backward()
    opt.step()
    auto = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()
    assert outs[0][0] == outs[1][0] == float(la.detach())
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][1], auto)
    assert not np.array_equal(auto, before)
    # not applicable: a model whose parameters do not share one buffer
    m2 = load(hf, w1r2())
    assert training.unrolled_step(m2, training.FlatAdam(fresh()[0].parameters()), traj, x, grid) is None


# ------------------------------------------------------------------------ 7. trainer
def test_window_dataset(hf):
    from hybridflux import training
    N, T, K, nx = 3, 8, 4, 16
    tr = np.arange(N * (T + 1) * 3 * nx, dtype=np.float32).reshape(N, T + 1, 3, nx)
    d = training.WindowDataset(tr, K, DEV)
    assert len(d) == N * (T - K + 1) == 15
    b = d.batch([0, len(d) - 1, 7]).cpu().numpy()
    assert b.shape == (3, K + 1, 3, nx)
    assert np.array_equal(b[0], tr[0, 0:K + 1])
    assert np.array_equal(b[1], tr[N - 1, T - K:T + 1])
    assert np.array_equal(b[2], tr[1, 2:2 + K + 1])
    with pytest.raises(IndexError):
        d.batch([len(d)])
    with pytest.raises(ValueError):
        training.WindowDataset(tr, T + 1, DEV)


def test_train_unrolled(hf, tmp_path):
    from hybridflux import datagen, training
    nx = 16
    tr = datagen.generate_trajectories(nx=nx, num_initial_conditions=6, steps_per_ic=8, device=DEV)
    assert tr.shape == (6, 9, 3, nx) and tr.dtype == np.float32
    want, _ = O.classical_run(O.Grid(nx), np.stack([O.initial_condition(O.Grid(nx), s) for s in range(6)]), 8)
    close(tr, want, 5e-7, what="trajectories")
    s = hf.BaselineSolver(nx, device=DEV)
    runs = []
    for r in range(2):
        m, h = training.train_unrolled(tr, s.x, s.dt, s.dx, s.nu, K=4, epochs=3, lr=1e-4, batch_size=8, seed=0,
                                       init=w1r2(), device=DEV, save_dir=str(tmp_path / f"run{r}"), log=None)
        runs.append((h, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()))
    h = runs[0][0]
    assert sorted(h) == ["epoch", "loss", "seconds"] and h["epoch"] == [1, 2, 3]
    assert len(h["loss"]) == 3 and np.isfinite(h["loss"]).all() and np.isfinite(h["seconds"]).all()
    assert h["loss"][-1] < h["loss"][0]
    assert runs[1][0]["loss"] == h["loss"] and np.array_equal(runs[0][1], runs[1][1])
    sd = torch.load(tmp_path / "run0" / "hybrid_unrolled_K4.pt", map_location="cpu")
    m2 = hf.FluxGNN(4, 128, 4)
    m2.load_state_dict(sd)
    assert np.array_equal(torch.cat([p.detach().reshape(-1) for p in m2.parameters()]).numpy(), runs[0][1])
    assert (tmp_path / "run0" / "history_unrolled_K4.json").exists()


def test_entry_points_refuse_unsupported(hf):
    """The Python layer surfaces the library's refusals (no fall-back)."""
    from hybridflux import _lib, engine
    grid = hf.BaselineSolver(64, device=DEV, poisson="tridiagonal").grid
    st = dev(ics(64, 2)[1])
    with pytest.raises(_lib.HybridFluxError) as e:
        engine.unroll_update(grid, torch.zeros(2 * 128, device=DEV), st)
    assert e.value.code == _lib.HF_EUNSUPPORTED
    assert ctypes.c_int(e.value.code).value == _lib.HF_EUNSUPPORTED
