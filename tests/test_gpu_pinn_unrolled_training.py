"""GPU parity of PINN's unrolled training (hf_pinn_unroll_loss,
hf_pinn_unroll_adjoint, hybridflux.training.pinn_unrolled_loss /
pinn_unrolled_step / train_pinn_unrolled): PINN differentiated through K steps
of its own rollout state <- state + net(state), against torch-CPU float64
autograd of tests/pinn_unroll_ref.py's restatement (which
test_pinn_unroll_ref_cpu.py ties to the reference trainer's own values) and the
reference's own Adam run (tests/golden/pinn_train.npz).

Gates, those of the sibling file test_gpu_pure_unrolled_training.py unless named:
  loss kernel alone, 5 values ........... rtol 1e-6 against float64 (its "step loss" gate)
  loss kernel, phys NULL ................ the total equals engine.pure_unroll_update's
      loss on the same states BIT FOR BIT: every shape here has nx <= 1024, one tile
      of that kernel per IC, so the partial layout is the same (beyond 1024 cells
      that kernel cuts its partials per tile and only rtol 1e-6 would hold)
  adjoint kernel alone .................. 2e-5 max|ref| + 1e-12 max|g| per tensor
      (its "adjoint kernel alone" gate); part 2 alone is the difference of two
      kernel outputs, under the same gate with g the whole gradient
  K-step loss value and terms ........... rtol 1e-5 (its "K-step loss value" gate)
  K-step parameter gradients ............ per tensor max(4 d32, 2e-5 max|g64|), d32 the
      error of the same gradient in torch-CPU float32, measured in the test
  predicted states ...................... atol 1e-5 + rtol 1e-5 (test_gpu_baselines' gate on
      PINN rollouts)
  exact case ............................ zero tolerance
  K = 1 against the one-step trainer .... loss row rtol 1e-6; six Adam steps: loss rtol
      1e-4, weights atol 2e-5, every element (test_gpu_pinn_training's gate)
Every measured error is recorded (conftest `record` / close).
The shapes here stop at nx = 300; the loss and adjoint kernels at 2048, 4097 and the
LDS limit 6144 are in test_gpu_nx_regimes.py (through this file's helpers)."""
import math

import numpy as np
import pytest
import torch

import pinn_unroll_ref as R
from conftest import close, golden
from nx_regimes import long_wave
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2e-5
DT, NU = 5e-3, 1e-3
ONES = (1.0, 1.0, 1.0)
# (nx, H, L, B, K): the MFMA path; the generic path at an odd nx; two cells; one cell;
# more ICs than a wave sums in one pass; more cells than threads
SHAPES = [(64, 256, 4, 5, 3), (21, 40, 3, 7, 2), (2, 32, 2, 3, 3), (1, 32, 2, 2, 2), (16, 64, 2, 33, 4),
          (300, 32, 2, 2, 2)]
LAMS = {"zero": None, "ref": R.REF_LAMBDA, "cont": (1.0, 0.0, 0.0), "mom": (0.0, 1.0, 0.0), "pois": (0.0, 0.0, 1.0)}


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def dx_of(nx):
    return 2 * math.pi / nx


def phys_kw(lam, nx):
    return {} if lam is None else dict(dx=dx_of(nx), dt=DT, nu=NU, physics_weights=lam)


def states(nx, B, n, seed):
    """n random states [n,B,3,nx] float32 around (1, 0, 0), each 0.02 from the one before;
    beyond 1024 cells (test_gpu_nx_regimes.py's sizes) the densities carry
    nx_regimes.long_wave, without which P p_n is lost next to p_E."""
    g = torch.Generator().manual_seed(seed)
    s = torch.stack([1 + 0.1 * torch.randn(B, nx, generator=g), 0.1 * torch.randn(B, nx, generator=g),
                     0.1 * torch.randn(B, nx, generator=g)], dim=1)
    if nx > 1024:
        s[:, 0] += torch.as_tensor(long_wave(nx, B), dtype=torch.float32)
    out = [s]
    for _ in range(n - 1):
        out.append(out[-1] + 0.02 * torch.randn(B, 3, nx, generator=g))
    return torch.stack(out)


# ----------------------------------------------------------------- 1. loss kernel alone
@pytest.mark.parametrize("lam", list(LAMS))
@pytest.mark.parametrize("nx,H,L,B,K", SHAPES)
def test_loss_kernel(hf, nx, H, L, B, K, lam):
    from hybridflux import engine
    lam_v = LAMS[lam]
    pred, st, tg = states(nx, B, 3, 100 + nx)
    w = (1.0, 0.5, 2.0)
    scale, ps = 1.0 / (K * 3 * B * nx), 1.0 / (K * B * nx)
    kw = {} if lam_v is None else dict(state=dev(st), phys=lam_v, phys_scale=ps, dx=dx_of(nx), dt=DT, nu=NU)
    runs = [engine.pinn_unroll_loss(dev(pred), dev(tg), w, scale, **kw).cpu().numpy().copy() for _ in range(2)]
    Pm = R.poisson_matrix(nx, nx * dx_of(nx)) if lam_v is not None else None
    want = R.step_terms(pred.double(), st.double(), tg.double(), w, lam_v, dx_of(nx), DT, NU, Pm, K)
    close(runs[0], np.array([float(v) for v in want]), 0.0, 1e-6, what="losses")
    assert np.array_equal(runs[0], runs[1])
    if lam_v is None:
        assert not runs[0][2:].any() and runs[0][0] == runs[0][1]
        # hf_pure_unroll_update's loss on the same states (state = pred, delta = 0): equal bits
        _, _, pure = engine.pure_unroll_update(torch.zeros(B * nx, 3, device=DEV), dev(pred),
                                               torch.zeros(nx, device=DEV), target=dev(tg), weights=w, scale=scale,
                                               want_nf=False)
        assert float(pure[0]) == float(runs[0][0])
    else:
        for j, v in enumerate(lam_v):
            assert (runs[0][2 + j] == 0.0) == (v == 0.0)


def test_loss_kernel_leaves_state_unread_without_phys(hf):
    """phys NULL: dev_state and dev_plan may be NULL (they are not read), and nothing but losses[0..4] is written."""
    from hybridflux import _lib, engine
    nx, B = 21, 3
    pred, tg = states(nx, B, 2, 5)
    p, t = dev(pred), dev(tg)
    out = torch.full((7,), 123.5, device=DEV)
    ws = engine.pinn_unroll_workspace(B, nx, DEV)
    w = np.ones(3, dtype=np.float32)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().hf_pinn_unroll_loss(_lib.ptr(p), None, _lib.ptr(t), B, nx, _lib.ptr(w), 0.25, None, 0.0, 0.0,
                                                  0.0, 0.0, None, _lib.ptr(out[1:6]), _lib.ptr(ws), ws.numel(),
                                                  engine.stream_of(p.device)))
    got = out.cpu().numpy()
    assert got[0] == 123.5 and got[6] == 123.5
    close(got[1:3], np.full(2, 0.25 * float(((pred.double() - tg.double()) ** 2).sum())), 0.0, 1e-6, what="data")


# -------------------------------------------------------------- 2. adjoint kernel alone
def adjoint_ref(pred, st, tg, nxt, carry, w, lam, K, nx, parts):
    """float64 autograd in p of the chosen parts: 1 = term_k(p, st), 2 = term_{k+1}(nxt, p), 3 = <carry, p>."""
    p = pred.double().requires_grad_(True)
    Pm = R.poisson_matrix(nx, nx * dx_of(nx)) if lam is not None else None
    tot = 0.0 * p.sum()
    if 1 in parts:
        tot = tot + R.step_terms(p, st.double(), tg.double(), w, lam, dx_of(nx), DT, NU, Pm, K)[0]
    if 2 in parts and lam is not None:
        tot = tot + R.step_terms(nxt.double(), p, tg.double(), w, lam, dx_of(nx), DT, NU, Pm, K)[0]
    if 3 in parts:
        tot = tot + (carry.double() * p).sum()
    tot.backward()
    return p.grad.numpy()


def adjoint_gpu(pred, st, tg, nxt, carry, w, lam, K, nx):
    from hybridflux import engine
    B = pred.shape[0]
    scale, ps = 1.0 / (K * 3 * B * nx), 1.0 / (K * B * nx)
    kw = {} if lam is None else dict(state=dev(st), phys=lam, phys_scale=ps, dx=dx_of(nx), dt=DT, nu=NU)
    runs = [engine.pinn_unroll_adjoint(dev(pred), dev(tg), w, scale, pred_next=None if nxt is None else dev(nxt),
                                       grad_state_next=None if carry is None else dev(carry), **kw).cpu().numpy()
            for _ in range(2)]
    assert np.array_equal(runs[0], runs[1])
    return runs[0].astype(np.float64)


def gate(record, name, what, got, want, gmax):
    err = float(np.abs(got - want).max())
    lim = REL * float(np.abs(want).max()) + 1e-12 * gmax
    record(name, f"{what}_err", err)
    record(name, f"{what}_limit", lim)
    assert np.isfinite(got).all() and err <= lim, (what, err, lim)


@pytest.mark.parametrize("lam", list(LAMS))
@pytest.mark.parametrize("nx,H,L,B,K", SHAPES)
def test_adjoint_kernel(hf, record, request, nx, H, L, B, K, lam):
    """The three parts one by one, then together, and every NULL combination."""
    lam_v = LAMS[lam]
    name = request.node.nodeid.split("::", 1)[-1]
    pred, st, tg, nxt = states(nx, B, 4, 200 + nx)
    w = (1.0, 0.5, 2.0)
    carry = 1e-3 * torch.randn(B, 3, nx, generator=torch.Generator().manual_seed(nx))
    full = adjoint_ref(pred, st, tg, nxt, carry, w, lam_v, K, nx, (1, 2, 3))
    gmax = float(np.abs(full).max())
    # part 1 alone: no next state, no carry
    g1 = adjoint_gpu(pred, st, tg, None, None, w, lam_v, K, nx)
    gate(record, name, "part1", g1, adjoint_ref(pred, st, tg, nxt, carry, w, lam_v, K, nx, (1,)), gmax)
    # part 3 alone: zero channel weights and no residual terms leave the carry, exactly
    g3 = adjoint_gpu(pred, st, tg, nxt, carry, (0.0, 0.0, 0.0), None, K, nx)
    assert np.array_equal(g3, carry.numpy().astype(np.float64))
    # parts 1 + 2, and part 2 alone as what the next state adds (also against the gather formulas)
    g12 = adjoint_gpu(pred, st, tg, nxt, None, w, lam_v, K, nx)
    gate(record, name, "part12", g12, adjoint_ref(pred, st, tg, nxt, carry, w, lam_v, K, nx, (1, 2)), gmax)
    if lam_v is None:
        assert np.array_equal(g12, g1)  # without residual terms the next state is not read
    else:
        want2 = adjoint_ref(pred, st, tg, nxt, carry, w, lam_v, K, nx, (2,))
        gather = R.state_slot_grad_np(nxt.numpy(), pred.numpy(), lam_v, 1.0 / (K * B * nx), dx_of(nx), DT, NU)
        assert np.abs(gather - want2).max() <= 1e-11 * max(np.abs(want2).max(), 1e-300)
        gate(record, name, "part2", g12 - g1, want2, gmax)
    # parts 1 + 3 (the last residual-free hand-over) and all three
    g13 = adjoint_gpu(pred, st, tg, None, carry, w, lam_v, K, nx)
    gate(record, name, "part13", g13, adjoint_ref(pred, st, tg, nxt, carry, w, lam_v, K, nx, (1, 3)), gmax)
    g123 = adjoint_gpu(pred, st, tg, nxt, carry, w, lam_v, K, nx)
    gate(record, name, "all", g123, full, gmax)


# --------------------------------------------------------------------- 3. exact case
@pytest.mark.parametrize("nx,B", [(1, 2), (2, 3), (64, 5), (300, 3)])
def test_exact_case(hf, nx, B):
    """Integer states and targets, power-of-two weights and scale, no residual terms:
    every product and sum is exact in float64 and fits float32, so the loss and the
    gradient (the carry included) equal their float64 values with zero tolerance."""
    from hybridflux import engine
    g = torch.Generator().manual_seed(nx)
    pred = torch.randint(-3, 4, (B, 3, nx), generator=g).float()
    tg = torch.randint(-3, 4, (B, 3, nx), generator=g).float()
    carry = torch.randint(-8, 9, (B, 3, nx), generator=g).float() / 512.0
    w, scale = (1.0, 0.5, 2.0), 2.0 ** -10
    wt = torch.tensor(w, dtype=torch.float64)[None, :, None]
    d = pred.double() - tg.double()
    losses = engine.pinn_unroll_loss(dev(pred), dev(tg), w, scale).cpu().numpy().astype(np.float64)
    want = float((wt * d * d).sum()) * scale
    assert losses[0] == want and losses[1] == want and not losses[2:].any()
    got = engine.pinn_unroll_adjoint(dev(pred), dev(tg), w, scale, grad_state_next=dev(carry)).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), (2.0 * scale * wt * d + carry.double()).numpy())
    got0 = engine.pinn_unroll_adjoint(dev(pred), dev(tg), w, scale).cpu().numpy()
    assert np.array_equal(got0.astype(np.float64), (2.0 * scale * wt * d).numpy())


# ------------------------------------------------------- 4. K-step gradients and states
def make_model(hf, nx, H, L):
    torch.manual_seed(nx + H + L)
    m = hf.PINN(3 * nx, H, L)
    if (nx, H, L) == (64, 256, 4):  # the reference-trained weights
        b = golden("baselines.npz")
        m.load_state_dict({k[5:]: torch.from_numpy(b[k]) for k in b.files if k.startswith("pinn.")})
    return m


def windows(nx, B, K):
    return states(nx, B, K + 1, 300 + nx).transpose(0, 1).contiguous()  # [B,K+1,3,nx]


_REF = {}


def reference(hf, nx, H, L, B, K, lam, through):
    """{dtype: (loss, grads, states, terms)} on the CPU, computed once per case and left unchanged."""
    key = (nx, H, L, B, K, lam, through)
    if key not in _REF:
        sd = {k: v.detach().clone() for k, v in make_model(hf, nx, H, L).state_dict().items()}
        traj, out = windows(nx, B, K), {}
        for dtype in (torch.float64, torch.float32):
            p = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
            loss, st, terms = R.unrolled_loss(lambda s: O.pinn_forward(p, s), traj.to(dtype), ONES, LAMS[lam],
                                              dx_of(nx), DT, NU, through)
            loss.backward()
            out[dtype] = (float(loss.detach()), {k: v.grad.double().numpy() for k, v in p.items()},
                          st.double().numpy(), terms.double().numpy())
        _REF[key] = out
    return _REF[key]


@pytest.mark.parametrize("through", [True, False])
@pytest.mark.parametrize("lam", list(LAMS))
@pytest.mark.parametrize("nx,H,L,B,K", SHAPES)
def test_unrolled_gradients(hf, record, request, nx, H, L, B, K, lam, through):
    from hybridflux import training
    ref = reference(hf, nx, H, L, B, K, lam, through)
    l64, g64, s64, t64 = ref[torch.float64]
    l32, g32, _, _ = ref[torch.float32]
    m = make_model(hf, nx, H, L).to(DEV)
    loss, pred, terms = training.pinn_unrolled_loss(m, dev(windows(nx, B, K)), through_state=through,
                                                    return_states=True, **phys_kw(LAMS[lam], nx))
    assert loss.shape == () and loss.requires_grad and not pred.requires_grad and not terms.requires_grad
    assert tuple(pred.shape) == (K, B, 3, nx) and tuple(terms.shape) == (K, 5)
    loss.backward()
    loss = float(loss.detach())
    name = request.node.nodeid.split("::", 1)[-1]
    record(name, "loss_rel_err", abs(loss - l64) / abs(l64))
    record(name, "loss_rel_err_cpu32", abs(l32 - l64) / abs(l64))
    close(pred, s64, 1e-5, 1e-5, what="states")
    close(terms, t64, 0.0, 1e-5, what="terms")
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    got = {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}
    assert set(got) == set(g64)
    for k, want in g64.items():
        err, scale = float(np.abs(got[k] - want).max()), float(np.abs(want).max())
        d32 = float(np.abs(g32[k] - want).max())
        record(name, f"{k}_err", err)
        record(name, f"{k}_d32", d32)
        record(name, f"{k}_max", scale)
        assert np.isfinite(got[k]).all() and scale > 0
        assert err <= max(4 * d32, REL * scale), (k, err, d32, scale)


def test_k1_same_gradient_in_both_modes(hf):
    from hybridflux import training
    nx, H, L, B = 21, 40, 3, 7
    traj = dev(windows(nx, B, 1))
    outs = []
    for through in (True, False):
        m = make_model(hf, nx, H, L).to(DEV)
        loss = training.pinn_unrolled_loss(m, traj, through_state=through, **phys_kw(R.REF_LAMBDA, nx))
        loss.backward()
        outs.append((float(loss.detach()), [p.grad.clone() for p in m.parameters()]))
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)


# ------------------------------------------------------ 5. direct step vs autograd step
def flat_of(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()


@pytest.mark.parametrize("lam", ["zero", "ref"])
@pytest.mark.parametrize("through", [True, False])
def test_direct_step_equals_autograd_step(hf, through, lam):
    """pinn_unrolled_step and pinn_unrolled_loss -> backward -> FlatAdam.step() run the
    same launches and add the K parameter gradients in the same order (last step
    first): the parameters agree bit for bit, and so do two direct steps."""
    from hybridflux import training
    nx, H, L, B, K = 64, 256, 4, 5, 3
    traj, kw = dev(windows(nx, B, K)), phys_kw(LAMS[lam], nx)

    def fresh():
        m = make_model(hf, nx, H, L).to(DEV).flatten_parameters_()
        return m, training.FlatAdam(m.parameters(), lr=1e-3)

    outs = []
    for _ in range(2):
        m, opt = fresh()
        loss = training.pinn_unrolled_step(m, opt, traj, through_state=through, **kw)
        assert loss is not None and not loss.requires_grad
        outs.append((float(loss), flat_of(m)))
    m, opt = fresh()
    before = flat_of(m)
    la = training.pinn_unrolled_loss(m, traj, through_state=through, **kw)
    opt.zero_grad()
    la.backward()
    opt.step()
    auto = flat_of(m)
    assert outs[0][0] == outs[1][0] == float(la.detach())
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][1], auto)
    assert not np.array_equal(auto, before)


def test_direct_step_not_applicable(hf):
    """Parameter hooks, an optimizer over other parameters, or parameters that do not
    share one buffer: pinn_unrolled_step returns None and changes nothing."""
    from hybridflux import training
    nx, H, L, B, K = 16, 64, 2, 3, 2
    traj = dev(windows(nx, B, K))
    m = make_model(hf, nx, H, L).to(DEV).flatten_parameters_()
    before = flat_of(m)
    opt = training.FlatAdam(m.parameters(), lr=1e-3)
    h = m.net[0].weight.register_hook(lambda g: None)
    assert training.pinn_unrolled_step(m, opt, traj) is None
    h.remove()
    other = make_model(hf, nx, H, L).to(DEV).flatten_parameters_()
    assert training.pinn_unrolled_step(m, training.FlatAdam(other.parameters()), traj) is None
    loose = make_model(hf, nx, H, L).to(DEV)
    assert training.pinn_unrolled_step(loose, torch.optim.SGD(loose.parameters(), lr=0.1), traj) is None
    assert np.array_equal(flat_of(m), before)
    assert training.pinn_unrolled_step(m, opt, traj) is not None
    with pytest.raises(TypeError):
        training.pinn_unrolled_loss(hf.PureGNN(4, 64, 3).to(DEV), traj)
    with pytest.raises(ValueError):
        training.pinn_unrolled_loss(m, dev(windows(8, B, K)))


# ------------------------------------------- 6. ties to the reference's own trainer, K = 1
@pytest.fixture(scope="module")
def fx():
    return golden("pinn_train.npz")


def fixture_model(hf, fx):
    m = hf.PINN(96, 64, 3)
    m.load_state_dict({k[5:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("init.")})
    return m.to(DEV).flatten_parameters_()


def fixture_windows(fx):
    traj, bic, bt = fx["traj"], fx["batch_ic"], fx["batch_t"]
    return [dev(np.stack([traj[bic[j], bt[j]], traj[bic[j], bt[j] + 1]], axis=1)) for j in range(6)]


def test_k1_row_equals_one_step_loss(hf, fx):
    """K = 1, w = (1,1,1), l = (0.1, 0.1, 0.01): the step's row is pinn_step's losses (there
    unweighted terms, here each with its weight), rtol 1e-6."""
    from hybridflux import training
    dx, dt, nu = float(fx["dx"]), float(fx["dt"]), float(fx["nu"])
    win = fixture_windows(fx)[0]
    m = fixture_model(hf, fx)
    _, _, terms = training.pinn_unrolled_loss(m, win, dx, dt, nu, physics_weights=R.REF_LAMBDA, return_states=True)
    one = training.pinn_step(m, torch.optim.SGD(m.parameters(), lr=0.0), win[:, 0], win[:, 1], dx, dt, nu)
    want = one.cpu().numpy().astype(np.float64) * np.array((1.0,) + training.PINN_LOSS_WEIGHTS)
    close(terms[0], want, 0.0, 1e-6, what="row")


def test_six_adam_steps_vs_reference(hf, fx, record, request):
    """Six pinn_unrolled_steps at K = 1 with the reference weights on the fixture's six
    batches against the reference's own loop (torch.optim.Adam(lr=1e-3) from init.*)."""
    from hybridflux import training
    dx, dt, nu = float(fx["dx"]), float(fx["dt"]), float(fx["nu"])
    m = fixture_model(hf, fx)
    opt = training.FlatAdam(m.parameters(), lr=1e-3)
    losses = []
    for win in fixture_windows(fx):
        loss = training.pinn_unrolled_step(m, opt, win, dx, dt, nu, physics_weights=R.REF_LAMBDA)
        assert loss is not None
        losses.append(float(loss))
    close(np.array(losses), np.asarray(fx["adam_losses"])[:, 0], 0.0, 1e-4, what="losses")
    worst = 0.0
    for k, v in m.state_dict().items():
        worst = max(worst, close(v, fx[f"adam_final.{k}"], 2e-5, 0.0, what=f"final.{k}"))
    record(request.node.nodeid.split("::", 1)[-1], "weights_max_abs", worst)


# ------------------------------------------------------------------------ 7. trainer
@pytest.mark.parametrize("lam", ["zero", "ref"])
def test_train_pinn_unrolled(hf, tmp_path, lam):
    from hybridflux import datagen, training
    nx, K = 16, 3
    tr = datagen.generate_trajectories(nx=nx, num_initial_conditions=4, steps_per_ic=8, device=DEV)
    assert tr.shape == (4, 9, 3, nx)
    base = hf.BaselineSolver(nx=nx, dt=DT, nu=NU, device=DEV)
    m, h = training.train_pinn_unrolled(tr, dx_of(nx), DT, NU, K=K, epochs=2, batch_size=8, hidden_dim=64,
                                        num_layers=3, physics_weights=LAMS[lam], seed=0, device=DEV,
                                        save_dir=str(tmp_path), log=None)
    assert sorted(h) == ["epoch", "loss", "seconds"] and h["epoch"] == [1, 2]
    assert len(h["loss"]) == 2 and np.isfinite(h["loss"]).all()
    assert (tmp_path / f"history_pinn_unrolled_K{K}.json").exists()
    sd = torch.load(tmp_path / f"pinn_unrolled_K{K}.pt", map_location="cpu")
    assert sorted(sd) == sorted(hf.PINN(3 * nx, 64, 3).state_dict())
    fresh = hf.PINN(3 * nx, 64, 3)
    fresh.load_state_dict(sd)
    assert np.array_equal(flat_of(fresh), flat_of(m))
    out = fresh.to(DEV).rollout(dev(tr[:3, 0]), 5, metrics=True, compare=base)
    for k in ("final", "traj", "metrics", "mse", "metrics_classical"):
        assert torch.isfinite(out[k]).all(), k
