"""GPU parity of the energy and charge terms of unrolled training
(hf_state_moments, hf_unroll_update_ex / hf_unroll_adjoint_ex and their PureGNN
and PINN counterparts, and the conservation / conservation_ref keywords of
hybridflux.training's three K-step losses, steps and trainers), against float64
numpy, conservation_ref.py's float64 restatement and torch-CPU autograd.

Tolerances (the gates of the three unrolled-training test files, unchanged):
  hf_state_moments ............ rtol 1e-13: float64 sums of at most 6144 terms of
      one sign, summed in another order than numpy's pairwise sum
  state_next, node features, the state term of the _ex calls ... equal bits with
      the plain calls, with and without cons
  energy / charge values, coefficients ... rtol 1e-6 against the float64 formula
      on the kernel's own state_next (test_gpu_unrolled_training's step-loss
      gate; the coefficients are float32, one rounding); the references sit 10 %
      from the state's own moments, so no residual is cancellation-bound
  adjoint kernels .............. 2e-5 max|ref| + 1e-12 max|g| per tensor, the
      float64 reference of the plain adjoint tests with the seed extended
  K-step parameter gradients ... per tensor max(4 d32, 2e-5 max|g64|), d32 the
      error of the same gradient in torch-CPU float32, measured in the test; on
      the inputs below d32 alone stays under 2e-5 max|g64| for every tensor of
      every case (at most 0.69 of it, FluxGNN at nx = 64 with zero channel weights;
      checked on the CPU when the references' offsets were chosen)
Every measured error is recorded (conftest `record` / close)."""
import numpy as np
import pytest
import torch

import conservation_ref as C
import pinn_unroll_ref as R
import test_gpu_pinn_unrolled_training as TN
import test_gpu_pure_unrolled_training as TP
import test_gpu_unrolled_training as TF
from conftest import close
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2e-5
LAM = (0.7, 1.3)
ONES, ZEROS = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
dev = TF.dev


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


def dev64(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def ref_of(state, rel=0.1):
    """(eref, qref) [B,2] float64, 10 % from the moments of `state` [B,3,nx] (alternating sign over the ICs)."""
    m = C.moments_np(state)
    return m * (1.0 + rel * np.where(np.arange(m.shape[0]) % 2 == 0, 1.0, -1.0)[:, None])


# ------------------------------------------------------------------ 1. hf_state_moments
@pytest.mark.parametrize("rows,nx", [(1, 1), (3, 2), (5, 48), (3, 100), (3, 256), (2, 1030), (1, 6144)])
def test_state_moments(hf, rows, nx):
    from hybridflux import engine
    g = np.random.default_rng(rows * 10000 + nx)
    s = np.stack([1 + 0.1 * g.normal(size=(rows, nx)), 0.3 * g.normal(size=(rows, nx)), 0.3 * g.normal(size=(rows, nx))],
                 axis=1).astype(np.float32)
    runs = [engine.state_moments(dev(s)) for _ in range(2)]
    assert runs[0].dtype == torch.float64 and tuple(runs[0].shape) == (rows, 2)
    close(runs[0], C.moments_np(s), 0.0, 1e-13, what="moments")
    assert torch.equal(runs[0], runs[1])
    win = engine.state_moments(dev(s).view(rows, 1, 3, nx))  # leading dimensions are kept
    assert tuple(win.shape) == (rows, 1, 2) and torch.equal(win.view(rows, 2), runs[0])


# ------------------------------------------------------- 2. the three forward _ex kernels
def check_row(row, coef, pred, ref, K, B, plain_loss, n_base):
    """The energy and charge values and the coefficients against the float64 formula on the kernel's own state."""
    p64 = torch.as_tensor(pred.cpu().numpy(), dtype=torch.float64)
    en, ch = C.cons_terms(p64, torch.as_tensor(ref), LAM, K)
    row = row.cpu().numpy()
    close(row[n_base:], np.array([float(en), float(ch)]), 0.0, 1e-6, what="energy_charge")
    close(coef, C.cons_coef(pred.cpu().numpy(), ref, LAM, K), 0.0, 1e-6, what="coef")
    close(row[:1], np.array([float(plain_loss) + float(en) + float(ch)]), 0.0, 1e-6, what="total")
    assert float(en) > 0 and float(ch) > 0


@pytest.mark.parametrize("nx,B", [(1, 2), (2, 3), (48, 3), (100, 3), (256, 3), (256, 9), (2048, 3)])
def test_hybrid_update_ex(hf, nx, B):
    from hybridflux import engine
    _, st = TF.ics(nx, B)
    g = np.random.default_rng(nx * 100 + B)
    st = (st + g.normal(0, 0.01, st.shape)).astype(np.float32)
    fe = g.normal(0, 0.3, (B, 2 * nx)).astype(np.float32)
    tgt = (st + g.normal(0, 0.05, st.shape)).astype(np.float32)
    w, K = (1.0, 0.5, 2.0), 4
    grid = TF.grid_of(hf, nx)
    scale = 1.0 / (K * 3 * B * nx)
    args = (grid, dev(fe).reshape(-1), dev(st))
    kw = dict(target=dev(tgt), weights=w, scale=scale)
    out0, nf0, loss0 = engine.unroll_update(*args, **kw)
    out1, nf1, row1 = engine.unroll_update(*args, ex=True, **kw)  # cons NULL: the plain bits, total == state
    assert torch.equal(out1, out0) and torch.equal(nf1, nf0)
    assert tuple(row1.shape) == (4,) and float(row1[0]) == float(row1[1]) == float(loss0[0]) and not row1[2:].any()
    ref = ref_of(out0.cpu().numpy())
    runs = []
    for _ in range(2):
        coef = torch.full((B, 2), 123.5, device=DEV)
        out2, nf2, row2 = engine.unroll_update(*args, cons=LAM, cons_scale=1.0 / (K * B), cons_ref=dev64(ref),
                                               cons_coef=coef, **kw)
        assert torch.equal(out2, out0) and torch.equal(nf2, nf0) and float(row2[1]) == float(loss0[0])
        runs.append((row2.clone(), coef))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    check_row(runs[0][0], runs[0][1], out0, ref, K, B, loss0[0], 2)


@pytest.mark.parametrize("nx,B", [(1, 2), (64, 3), (1024, 2), (1030, 3), (2500, 2)])
def test_pure_update_ex(hf, nx, B):
    from hybridflux import engine
    G, st = TP.ics(nx, B)
    g = np.random.default_rng(nx * 100 + B)
    st = (st + g.normal(0, 0.01, st.shape)).astype(np.float32)
    delta = g.normal(0, 0.05, (B * nx, 3)).astype(np.float32)
    tgt = (st + g.normal(0, 0.05, st.shape)).astype(np.float32)
    w, K = (1.0, 0.5, 2.0), 4
    scale = 1.0 / (K * 3 * B * nx)
    args = (dev(delta), dev(st), TP.xdev(G))
    kw = dict(target=dev(tgt), weights=w, scale=scale)
    out0, nf0, loss0 = engine.pure_unroll_update(*args, **kw)
    out1, nf1, row1 = engine.pure_unroll_update(*args, ex=True, **kw)
    assert torch.equal(out1, out0) and torch.equal(nf1, nf0)
    assert tuple(row1.shape) == (4,) and float(row1[0]) == float(row1[1]) == float(loss0[0]) and not row1[2:].any()
    ref = ref_of(out0.cpu().numpy())
    runs = []
    for _ in range(2):
        coef = torch.full((B, 2), 123.5, device=DEV)
        out2, nf2, row2 = engine.pure_unroll_update(*args, cons=LAM, cons_scale=1.0 / (K * B), cons_ref=dev64(ref),
                                                    cons_coef=coef, **kw)
        assert torch.equal(out2, out0) and torch.equal(nf2, nf0) and float(row2[1]) == float(loss0[0])
        runs.append((row2.clone(), coef))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    check_row(runs[0][0], runs[0][1], out0, ref, K, B, loss0[0], 2)


@pytest.mark.parametrize("phys", [None, R.REF_LAMBDA])
@pytest.mark.parametrize("nx,B", [(1, 2), (2, 3), (64, 3), (100, 2)])
def test_pinn_loss_ex(hf, nx, B, phys):
    from hybridflux import engine
    pred, st, tg = TN.states(nx, B, 3, 100 + nx)
    w, K = (1.0, 0.5, 2.0), 3
    scale, ps = 1.0 / (K * 3 * B * nx), 1.0 / (K * B * nx)
    kw = {} if phys is None else dict(state=dev(st), phys=phys, phys_scale=ps, dx=TN.dx_of(nx), dt=TN.DT, nu=TN.NU)
    row0 = engine.pinn_unroll_loss(dev(pred), dev(tg), w, scale, **kw)
    row1 = engine.pinn_unroll_loss(dev(pred), dev(tg), w, scale, ex=True, **kw)
    assert tuple(row1.shape) == (7,) and torch.equal(row1[:5], row0) and not row1[5:].any()
    ref = ref_of(pred.numpy())
    runs = []
    for _ in range(2):
        coef = torch.full((B, 2), 123.5, device=DEV)
        row2 = engine.pinn_unroll_loss(dev(pred), dev(tg), w, scale, cons=LAM, cons_scale=1.0 / (K * B),
                                       cons_ref=dev64(ref), cons_coef=coef, **kw)
        assert torch.equal(row2[1:5], row0[1:])
        runs.append((row2, coef))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    check_row(runs[0][0], runs[0][1], dev(pred), ref, K, B, row0[0], 5)


# ------------------------------------------------------- 3. the three adjoint _ex kernels
def coef_for(B, nx, seed):
    """Coefficients of the size the forward leaves at these shapes: 2 lam cons_scale r / nx with |r| about 0.1."""
    return (np.random.default_rng(seed).normal(0, 1.0, (B, 2)) * 0.2 / (4 * B * nx)).astype(np.float32)


def gate(record, name, what, got, want, gmax):
    err = float(np.abs(got.astype(np.float64) - want).max())
    lim = REL * float(np.abs(want).max()) + 1e-12 * gmax
    record(name, f"{what}_err", err)
    record(name, f"{what}_limit", lim)
    assert np.isfinite(got).all() and err <= lim, (what, err, lim)


@pytest.mark.parametrize("nx,B", [(1, 2), (2, 3), (48, 3), (100, 3), (256, 3), (256, 9), (2048, 3)])
def test_hybrid_adjoint_ex(hf, record, request, nx, B):
    from hybridflux import engine
    name = request.node.nodeid.split("::", 1)[-1]
    G, st = TF.ics(nx, B, seed0=3)
    g = np.random.default_rng(nx * 10 + B)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    sn, tg = f32(st + g.normal(0, 0.05, st.shape)), f32(st + g.normal(0, 0.05, st.shape))
    din, gnf = f32(g.normal(0, 1e-3, st.shape)), f32(g.normal(0, 1e-3, (B * nx, 4)))
    w, scale = (1.0, 0.5, 2.0), 1.0 / (4 * 3 * B * nx)
    grid = TF.grid_of(hf, nx)
    args = (grid, dev(st), dev(sn), dev(tg), w, scale, dev(din), dev(gnf))
    plain = engine.unroll_adjoint(*args)
    null = engine.unroll_adjoint(*args, ex=True)  # a NULL coefficient pointer: the plain bits
    assert torch.equal(null[0], plain[0]) and torch.equal(null[1], plain[1])
    coef = coef_for(B, nx, nx + B)
    g_fe, direct = engine.unroll_adjoint(*args, cons_coef=dev(coef))
    other = coef.copy()
    other[:, 1] = 7.0  # cq is not read: the charge term has no gradient through the conservative update
    g_fe2, direct2 = engine.unroll_adjoint(*args, cons_coef=dev(other))
    assert torch.equal(g_fe2, g_fe) and torch.equal(direct2, direct)
    gt = 2.0 * np.asarray(w)[None, :, None] * scale * (sn.astype(np.float64) - tg) + C.seed_np(sn, coef, hybrid=True)
    gt = gt + din + gnf.astype(np.float64).reshape(B, nx, 4)[:, :, :3].transpose(0, 2, 1)
    c, dt, k, _ = TF.consts(G, torch.float64)
    s64 = torch.as_tensor(st, dtype=torch.float64).requires_grad_(True)
    fe = torch.zeros(B, 2 * nx, dtype=torch.float64, requires_grad=True)
    (torch.as_tensor(gt) * C.hybrid_step_t(s64, fe, c, dt, k)).sum().backward()
    gmax = float(np.abs(gt).max())
    gate(record, name, "g_fe", g_fe.cpu().numpy(), fe.grad.numpy(), gmax)
    gate(record, name, "direct", direct.cpu().numpy(), s64.grad.numpy(), gmax)
    if nx > 2:  # the energy term does move the result
        assert not torch.equal(direct, plain[1])


@pytest.mark.parametrize("nx,B", [(1, 2), (64, 3), (1024, 2), (1030, 3), (2500, 2)])
def test_pure_adjoint_ex(hf, record, request, nx, B):
    from hybridflux import engine
    name = request.node.nodeid.split("::", 1)[-1]
    _, st = TP.ics(nx, B, seed0=3)
    g = np.random.default_rng(nx * 10 + B)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    sn, tg = f32(st + g.normal(0, 0.05, st.shape)), f32(st + g.normal(0, 0.05, st.shape))
    gdn, gnf = f32(g.normal(0, 1e-3, (B * nx, 3))), f32(g.normal(0, 1e-3, (B * nx, 4)))
    w, scale = (1.0, 0.5, 2.0), 1.0 / (4 * 3 * B * nx)
    args = (dev(sn), dev(tg), w, scale, dev(gdn), dev(gnf))
    plain = engine.pure_unroll_adjoint(*args)
    assert torch.equal(engine.pure_unroll_adjoint(*args, ex=True), plain)
    coef = coef_for(B, nx, nx + B)
    runs = [engine.pure_unroll_adjoint(*args, cons_coef=dev(coef)) for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], plain)
    gt = 2.0 * np.asarray(w)[None, :, None] * scale * (sn.astype(np.float64) - tg) + C.seed_np(sn, coef)
    gt = gt + gdn.astype(np.float64).reshape(B, nx, 3).transpose(0, 2, 1)
    gt = gt + gnf.astype(np.float64).reshape(B, nx, 4)[:, :, :3].transpose(0, 2, 1)
    want = gt.transpose(0, 2, 1).reshape(B * nx, 3)  # s' = s + delta^T: dL/ddelta is dL/ds' transposed
    gate(record, name, "grad_delta", runs[0].cpu().numpy(), want, float(np.abs(gt).max()))


@pytest.mark.parametrize("phys", [None, R.REF_LAMBDA])
@pytest.mark.parametrize("nx,B", [(1, 2), (2, 3), (64, 3), (100, 2)])
def test_pinn_adjoint_ex(hf, record, request, nx, B, phys):
    from hybridflux import engine
    name = request.node.nodeid.split("::", 1)[-1]
    K = 3
    pred, st, tg, nxt = TN.states(nx, B, 4, 200 + nx)
    w = (1.0, 0.5, 2.0)
    carry = 1e-3 * torch.randn(B, 3, nx, generator=torch.Generator().manual_seed(nx))
    scale, ps = 1.0 / (K * 3 * B * nx), 1.0 / (K * B * nx)
    kw = dict(pred_next=dev(nxt), grad_state_next=dev(carry))
    if phys is not None:
        kw.update(state=dev(st), phys=phys, phys_scale=ps, dx=TN.dx_of(nx), dt=TN.DT, nu=TN.NU)
    plain = engine.pinn_unroll_adjoint(dev(pred), dev(tg), w, scale, **kw)
    assert torch.equal(engine.pinn_unroll_adjoint(dev(pred), dev(tg), w, scale, ex=True, **kw), plain)
    coef = coef_for(B, nx, nx + B)
    runs = [engine.pinn_unroll_adjoint(dev(pred), dev(tg), w, scale, cons_coef=dev(coef), **kw) for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], plain)
    want = TN.adjoint_ref(pred, st, tg, nxt, carry, w, phys, K, nx, (1, 2, 3)) + C.seed_np(pred.numpy(), coef)
    gate(record, name, "grad", runs[0].cpu().numpy(), want, float(np.abs(want).max()))


# ------------------------------------------- 4. end-to-end gradients vs float64 autograd
class Flux:
    cases = [(64, 3, 4, 128), (16, 3, 4, 128), (256, 3, 2, 64)]
    zero_grad = ("edge_mlp.2.bias",)  # analytically 0: a constant edge flux cancels in F_i - F_{i-1}

    @staticmethod
    def setup(hf, nx, B, K, H):
        G = O.Grid(nx, dt=TF.dt_for(nx))
        sd, dims = (TF.w1r2(), (4, 128, 4)) if H == 128 else (TF.rand_sd64(2, 11), (4, 64, 2))
        return G, sd, dims, TF.classical_windows(G, B, K)

    @staticmethod
    def cpu(G, sd, traj, w, lam, ref, dtype, through):
        B = traj.shape[0]
        return C.loss_and_grads(lambda p: C.flux_step(p, G, B, dtype), sd, traj, w, lam, ref, dtype, through)

    @staticmethod
    def model(hf, sd, dims):
        return TF.load(hf, sd, dims)

    @staticmethod
    def call(hf, fn, m, traj, nx, *a, **kw):
        grid = TF.grid_of(hf, nx)
        x, _ = grid.on(torch.device(DEV))
        return fn(m, *a, traj, x, grid, **kw)


class Pure:
    cases = [(64, 3, 3, 64), (1030, 2, 2, 64)]
    zero_grad = ()

    @staticmethod
    def setup(hf, nx, B, K, H):
        G = O.Grid(nx)
        return G, TP.sd64(), (4, 64, 3), TP.classical_windows(G, B, K)

    @staticmethod
    def cpu(G, sd, traj, w, lam, ref, dtype, through):
        B = traj.shape[0]
        return C.loss_and_grads(lambda p: C.pure_step(p, G, B, dtype), sd, traj, w, lam, ref, dtype, through)

    @staticmethod
    def model(hf, sd, dims):
        return TP.load(hf, sd, dims)

    @staticmethod
    def call(hf, fn, m, traj, nx, *a, **kw):
        return fn(m, *a, traj, TP.xdev(O.Grid(nx)), **kw)


class Pinn:
    cases = [(64, 3, 3, 256), (5, 2, 2, 8)]
    zero_grad = ()

    @staticmethod
    def setup(hf, nx, B, K, H):
        L = 4 if H == 256 else 2
        sd = {k: v.detach().numpy().copy() for k, v in TN.make_model(hf, nx, H, L).state_dict().items()}
        return None, sd, (3 * nx, H, L), TN.windows(nx, B, K).numpy()

    @staticmethod
    def cpu(G, sd, traj, w, lam, ref, dtype, through):
        return C.loss_and_grads(C.pinn_step, sd, traj, w, lam, ref, dtype, through)

    @staticmethod
    def model(hf, sd, dims):
        m = hf.PINN(*dims)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        return m.to(DEV)

    @staticmethod
    def call(hf, fn, m, traj, nx, *a, **kw):
        return fn(m, *a, traj, **kw)


MODELS = {"flux": Flux, "pure": Pure, "pinn": Pinn}
LOSS = {"flux": "unrolled_loss", "pure": "pure_unrolled_loss", "pinn": "pinn_unrolled_loss"}
STEP = {"flux": "unrolled_step", "pure": "pure_unrolled_step", "pinn": "pinn_unrolled_step"}
GRAD_CASES = [(kind, *c) for kind, M in MODELS.items() for c in M.cases]
_REF = {}


def grad_reference(hf, kind, nx, B, K, H, w, lam, through):
    """(sd, dims, traj, ref, l64, g64, g32, rows64), computed once per case and left unchanged."""
    key = (kind, nx, B, K, H, w, lam, through)
    if key not in _REF:
        M = MODELS[kind]
        G, sd, dims, traj = M.setup(hf, nx, B, K, H)
        ref = C.offset_ref(traj)
        l64, g64, _, rows = M.cpu(G, sd, traj, w, lam, ref, torch.float64, through)
        _, g32, _, _ = M.cpu(G, sd, traj, w, lam, ref, torch.float32, through)
        _REF[key] = (sd, dims, traj, ref, l64, g64, g32, rows)
    return _REF[key]


def gpu_grads(hf, kind, sd, dims, traj, ref, nx, w, lam, through):
    from hybridflux import training
    M = MODELS[kind]
    m = M.model(hf, sd, dims)
    loss, pred, rows = M.call(hf, getattr(training, LOSS[kind]), m, dev(traj), nx, channel_weights=w, through_state=through,
                              conservation=lam, conservation_ref=dev64(ref), return_states=True)
    assert loss.shape == () and loss.requires_grad and not rows.requires_grad
    loss.backward()
    return float(loss.detach()), rows.cpu().numpy(), {k: p.grad.detach().cpu().numpy().copy()
                                                      for k, p in m.named_parameters()}


@pytest.mark.parametrize("through", [True, False])
@pytest.mark.parametrize("w", [ONES, ZEROS])
@pytest.mark.parametrize("kind,nx,B,K,H", GRAD_CASES)
def test_unrolled_gradients(hf, record, request, kind, nx, B, K, H, w, through):
    sd, dims, traj, ref, l64, g64, g32, rows64 = grad_reference(hf, kind, nx, B, K, H, w, (1.0, 1.0), through)
    loss, rows, got = gpu_grads(hf, kind, sd, dims, traj, ref, nx, w, (1.0, 1.0), through)
    name = request.node.nodeid.split("::", 1)[-1]
    record(name, "loss_rel_err", abs(loss - l64) / abs(l64))
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    assert rows.shape == (K, 4 if kind != "pinn" else 7)
    close(rows[:, -2:], rows64[:, -2:], 0.0, 1e-5, what="energy_charge")
    assert set(got) == set(g64)
    others = max(float(np.abs(v).max()) for k, v in g64.items() if k not in MODELS[kind].zero_grad)
    for k, want in g64.items():
        err = float(np.abs(got[k].astype(np.float64) - want).max())
        scale = float(np.abs(want).max())
        d32 = float(np.abs(g32[k] - want).max())
        record(name, f"{k}_err", err)
        record(name, f"{k}_d32", d32)
        record(name, f"{k}_max", scale)
        assert np.isfinite(got[k]).all()
        if k in MODELS[kind].zero_grad:
            assert float(np.abs(got[k]).max()) <= 1e-6 * others, (k, got[k], others)
        else:
            assert scale > 0 and err <= max(4 * d32, REL * scale), (k, err, d32, scale)


@pytest.mark.parametrize("nx,B,K,H", Flux.cases)
def test_flux_charge_term_has_no_gradient(hf, record, request, nx, B, K, H):
    """FluxGNN with lam = (0, 1) and zero channel weights: analytically zero (the face
    fluxes telescope), here at most 1e-6 of the energy-only gradient's largest entry;
    the charge value is still reported."""
    sd, dims, traj, ref, *_ = grad_reference(hf, "flux", nx, B, K, H, ZEROS, (1.0, 1.0), True)
    _, rows_q, gq = gpu_grads(hf, "flux", sd, dims, traj, ref, nx, ZEROS, (0.0, 1.0), True)
    _, rows_e, ge = gpu_grads(hf, "flux", sd, dims, traj, ref, nx, ZEROS, (1.0, 0.0), True)
    top = max(float(np.abs(v).max()) for v in ge.values())
    worst = max(float(np.abs(v).max()) for v in gq.values())
    name = request.node.nodeid.split("::", 1)[-1]
    record(name, "charge_only_max", worst)
    record(name, "energy_only_max", top)
    assert top > 0 and worst <= 1e-6 * top, (worst, top)
    assert rows_q[:, 3].sum() > 0 and not rows_q[:, 2].any() and rows_e[:, 2].sum() > 0 and not rows_e[:, 3].any()


# -------------------------------------------------------------- 5. steps and trainers
def flat_of(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()


STEP_CASES = {"flux": (64, 3, 4, 128), "pure": (64, 3, 3, 64), "pinn": (64, 3, 3, 256)}


@pytest.mark.parametrize("through", [True, False])
@pytest.mark.parametrize("kind", list(MODELS))
def test_direct_step_equals_autograd_step(hf, kind, through):
    """With the terms on, the direct step and loss -> backward -> FlatAdam.step() give the
    same parameters bit for bit, and so do two direct steps."""
    from hybridflux import training
    M = MODELS[kind]
    nx, B, K, H = STEP_CASES[kind]
    _, sd, dims, traj = M.setup(hf, nx, B, K, H)
    traj = dev(traj)
    kw = dict(through_state=through, conservation=LAM, conservation_ref="start")

    def fresh():
        m = M.model(hf, sd, dims).flatten_parameters_()
        return m, training.FlatAdam(m.parameters(), lr=1e-3)

    outs = []
    for _ in range(2):
        m, opt = fresh()
        loss = M.call(hf, getattr(training, STEP[kind]), m, traj, nx, opt, **kw)
        assert loss is not None and not loss.requires_grad
        outs.append((float(loss), flat_of(m)))
    m, opt = fresh()
    before = flat_of(m)
    la = M.call(hf, getattr(training, LOSS[kind]), m, traj, nx, **kw)
    opt.zero_grad()
    la.backward()
    opt.step()
    auto = flat_of(m)
    assert outs[0][0] == outs[1][0] == float(la.detach())
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][1], auto)
    assert not np.array_equal(auto, before)
    m, opt = fresh()  # and the terms do move the step
    M.call(hf, getattr(training, STEP[kind]), m, traj, nx, opt, through_state=through)
    assert not np.array_equal(flat_of(m), auto)


@pytest.mark.parametrize("kind", list(MODELS))
def test_keyword_forms(hf, kind):
    """conservation=None is the call without the argument; "target" and "start" are the
    tensor form built from hf_state_moments; all bit for bit, loss and gradients."""
    from hybridflux import engine, training
    M = MODELS[kind]
    nx, B, K, H = STEP_CASES[kind]
    _, sd, dims, traj = M.setup(hf, nx, B, K, H)
    traj = dev(traj)

    def run(**kw):
        m = M.model(hf, sd, dims)
        out = M.call(hf, getattr(training, LOSS[kind]), m, traj, nx, return_states=True, **kw)
        out[0].backward()
        return float(out[0].detach()), out[-1].cpu().numpy(), flat_of(m), \
            torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu().numpy()

    a, b = run(), run(conservation=None)
    assert a[0] == b[0] and np.array_equal(a[3], b[3])
    mom = engine.state_moments(traj.contiguous())  # [B,K+1,2]
    forms = {"target": mom[:, 1:].contiguous(), "start": mom[:, :1].expand(B, K, 2).contiguous()}
    for word, tensor in forms.items():
        c, d = run(conservation=LAM, conservation_ref=word), run(conservation=LAM, conservation_ref=tensor)
        assert c[0] == d[0] and np.array_equal(c[1], d[1]) and np.array_equal(c[3], d[3]), word
        assert c[1].shape == (K, 4 if kind != "pinn" else 7) and np.isfinite(c[1]).all()
        assert not np.array_equal(c[3], a[3])
    # with lam = (0, 0) the terms are reported as 0 and the steps' totals are the plain call's
    # (the sum over the K steps reads a column of the rows here: 1e-6 for its order)
    z = run(conservation=(0.0, 0.0))
    assert abs(z[0] - a[0]) <= 1e-6 * abs(a[0]) and not z[1][:, -2:].any()
    if kind != "pinn":
        assert np.array_equal(z[1][:, 0], z[1][:, 1])


@pytest.mark.parametrize("ref", ["target", "start"])
@pytest.mark.parametrize("kind", list(MODELS))
def test_trainers(hf, tmp_path, kind, ref):
    """2 epochs on 2 ICs x 6 steps: the history holds finite energy_loss and charge_loss, two runs agree."""
    from hybridflux import datagen, training
    nx, K = 16, 3
    tr = datagen.generate_trajectories(nx=nx, num_initial_conditions=2, steps_per_ic=6, device=DEV)
    s = hf.BaselineSolver(nx, device=DEV)
    kw = dict(K=K, epochs=2, batch_size=4, seed=0, device=DEV, save_dir=None, log=None, conservation=(10.0, 10.0),
              conservation_ref=ref)
    runs = []
    for _ in range(2):
        if kind == "flux":
            m, h = training.train_unrolled(tr, s.x, s.dt, s.dx, s.nu, init=TF.w1r2(), lr=1e-4, **kw)
        elif kind == "pure":
            m, h = training.train_pure_gnn_unrolled(tr, s.x, hidden_dim=64, num_layers=3, **kw)
        else:
            m, h = training.train_pinn_unrolled(tr, s.dx, s.dt, s.nu, hidden_dim=64, num_layers=3, **kw)
        runs.append((h, flat_of(m)))
    h = runs[0][0]
    assert sorted(h) == ["charge_loss", "energy_loss", "epoch", "loss", "seconds"] and h["epoch"] == [1, 2]
    for key in ("loss", "energy_loss", "charge_loss"):
        assert len(h[key]) == 2 and np.isfinite(h[key]).all() and min(h[key]) >= 0, key
        assert runs[1][0][key] == h[key]
    assert all(e + c <= l * (1 + 1e-6) for e, c, l in zip(h["energy_loss"], h["charge_loss"], h["loss"]))
    assert np.array_equal(runs[0][1], runs[1][1]) and max(h["energy_loss"]) > 0
