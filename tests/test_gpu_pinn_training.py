"""GPU parity of PINN training (scripts/training/train_pinn.py:48-201): the HIP
training forward / backward (hf_pinn_forward_train / hf_pinn_backward) behind
hybridflux.training.pinn_forward, the one-launch physics loss (hf_pinn_loss)
and the trainer (pinn_step, train_pinn), against the reference's own autograd
and Adam run (tests/golden/pinn_train.npz, made by make_pinn_train.py) and,
where no fixture covers a shape, torch-CPU float64 autograd of this file's own
restatement of the loss (restated_loss below) over O.pinn_forward;
tests/test_abi_pinn_train_cpu.py checks that restatement against the reference's
own values without a GPU.

PINN.forward stays the inference call: under autograd it raises
(test_inference_guard_stays), and training goes through pinn_forward.

Gates (the project's existing ones).  Forward values: atol 2e-6 + rtol 1e-5.
Loss values: rtol 1e-5.  Gradients: |got - ref| <= 2e-5 * max|ref| + 1e-9 per
tensor.  Six Adam steps: per-step loss rtol 1e-4, final weights atol 2e-5 with
no element left out.  The reference alone, float32 against float64 (f64_* in
the fixture): first-batch losses rel 9.4e-8, gradients 4.5e-7 * max|ref|, six
steps' losses rel 3.0e-7, final weights max abs 1.6e-7, so every gate leaves
at least 30x over the reference's own rounding.

hf_pinn_loss alone runs here up to nx = 1024; 2048, 4097 and the LDS limit 6144 are
in test_gpu_nx_regimes.py (through check_loss below).
"""
import math

import numpy as np
import pytest
import torch

from conftest import close, golden
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2e-5
DT, NU = 5e-3, 1e-3
WEIGHTS = (1.0, 0.1, 0.1, 0.01)
KEYS5 = ("loss", "data", "cont", "mom", "pois")


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    return hybridflux


@pytest.fixture(scope="module")
def fx():
    return golden("pinn_train.npz")


def grad_close(got, want, what):
    """The gradient gate, through close(): atol = 2e-5 * max|ref| + 1e-9."""
    want = np.asarray(want)
    close(got, want, REL * float(np.abs(want).max()) + 1e-9, 0.0, what=what)


def poisson_column(nx, length):
    """First column of the engine's spectral Poisson operator (hf_poisson_coeffs: a host helper)."""
    from ctypes import c_void_p

    from hybridflux._lib import check, lib
    pc = np.empty(lib().hf_poisson_plan_len(nx), dtype=np.float64)
    check(lib().hf_poisson_coeffs(nx, float(length), pc.ctypes.data_as(c_void_p)))
    return pc[:nx].copy()


def restated_loss(pred, st, sn, dx, dt, nu, w, col):
    """The loss of the issue's formulas in torch (any dtype; differentiable in
    pred): returns (loss, data, cont, mom, pois).  P is the circulant with
    first column col: (P f)[i] = sum_j col[(i - j) mod nx] f[j]; col may also be that
    matrix itself, already built in pred's dtype (the wide sizes build it once)."""
    nx = pred.shape[-1]
    n, u, E = st[:, 0], st[:, 1], st[:, 2]
    pn, pu, pE = pred[:, 0], pred[:, 1], pred[:, 2]
    up, dn = (lambda f: torch.roll(f, -1, -1)), (lambda f: torch.roll(f, 1, -1))  # f[i+1], f[i-1]
    r_c = (pn - n) / dt + (up(n * u) - dn(n * u)) / (2 * dx)
    r_m = (pu - u) / dt + u * (up(u) - dn(u)) / (2 * dx) + E - nu * (up(u) - 2 * u + dn(u)) / dx ** 2
    i = torch.arange(nx)
    Pm = col if np.ndim(col) == 2 else torch.as_tensor(col, dtype=pred.dtype)[(i[:, None] - i[None, :]) % nx]
    keep = torch.ones(nx, dtype=pred.dtype)
    keep[0] = 0.0
    X = -(pn @ Pm.T) * keep  # X[0] = 0
    r_p = pE - X
    data, cont, mom, pois = ((pred - sn) ** 2).mean(), (r_c ** 2).mean(), (r_m ** 2).mean(), (r_p ** 2).mean()
    return w[0] * data + w[1] * cont + w[2] * mom + w[3] * pois, data, cont, mom, pois


def fixture_model(hf, fx, prefix="init."):
    m = hf.PINN(96, 64, 3)
    m.load_state_dict({k[len(prefix):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(prefix)})
    return m


def fixture_batch(fx, k):
    ic, t = fx["batch_ic"][k], fx["batch_t"][k]
    return torch.from_numpy(fx["traj"][ic, t]), torch.from_numpy(fx["traj"][ic, t + 1])


def consts(fx):
    return float(fx["dx"]), float(fx["dt"]), float(fx["nu"])


@pytest.mark.parametrize("path", ["autograd", "direct"])
@pytest.mark.parametrize("where", ["device", "host"])
def test_fixture_first_batch(hf, fx, where, path):
    """Prediction, the five loss values, dL/dpred and dL/dparams of the fixture's
    first batch equal the reference's, through pinn_forward + pinn_physics_loss +
    backward() and through pinn_step's direct path (losses and dL/dparams; lr = 0
    keeps the weights), with everything on the device and with host tensors and a
    CPU-resident module (the gradients then land on the CPU)."""
    from hybridflux import training as T
    dev = DEV if where == "device" else "cpu"
    dx, dt, nu = consts(fx)
    m = fixture_model(hf, fx).to(dev)
    st, sn = (t.to(dev) for t in fixture_batch(fx, 0))
    if path == "autograd":
        pred = T.pinn_forward(m, st)
        assert pred.requires_grad and pred.shape == st.shape and pred.device.type == torch.device(dev).type
        close(pred, fx["first_pred"], 2e-6, 1e-5, what="pred")
        pred.retain_grad()
        loss, terms = T.pinn_physics_loss(pred, st, sn, dx, dt, nu)
        assert not terms.requires_grad and terms.shape == (4,)
        close(torch.cat([loss.detach().reshape(1), terms]), fx["first_losses"], 0.0, 1e-5, what="losses")
        loss.backward()
        grad_close(pred.grad, fx["first_grad_pred"], "grad_pred")
    else:
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        assert T._pinn_direct_ok(m, opt)
        losses = T.pinn_step(m, opt, st, sn, dx, dt, nu)
        assert losses.shape == (5,) and losses.is_cuda
        close(losses, fx["first_losses"], 0.0, 1e-5, what="losses")
    for k, p in m.named_parameters():
        assert p.grad.device == p.device, k
        grad_close(p.grad, fx[f"first_grad.{k}"], f"grad.{k}")


SHAPES = [(192, 256, 4, 32),   # the reference shape, with baselines.npz's pinn.* weights
          (192, 256, 2, 5),    # no hidden layer, a partial tile
          (96, 64, 3, 130),    # B crosses a 128-row tile, two weight-gradient splits
          (96, 64, 8, 3),      # the layer limit
          (144, 96, 3, 7),     # nx = 48: the generic path
          (15, 16, 2, 3),      # odd nx = 5
          (6, 8, 3, 2),        # nx = 2
          (3, 8, 2, 4)]        # nx = 1: every difference and P vanish


def shape_case(hf, D, H, L, B, seed=5):
    torch.manual_seed(seed)
    m = hf.PINN(D, H, L)
    if (D, H, L) == (192, 256, 4):
        b = golden("baselines.npz")
        m.load_state_dict({k[5:]: torch.from_numpy(b[k]) for k in b.files if k.startswith("pinn.")})
    nx = D // 3
    g = torch.Generator().manual_seed(seed + 1)
    st = torch.stack([1 + 0.1 * torch.randn(B, nx, generator=g), 0.1 * torch.randn(B, nx, generator=g),
                      0.1 * torch.randn(B, nx, generator=g)], dim=1)
    sn = st + 0.01 * torch.randn(B, 3, nx, generator=g)
    return m, st, sn


def restated_run(m, st, sn, dx, dt, nu, w):
    """float64 CPU autograd of O.pinn_forward + restated_loss: pred, the five loss
    values, dL/dparams, dL/dstate (through pred only, as pinn_physics_loss)."""
    p = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
    s = st.double().requires_grad_(True)
    pred = O.pinn_forward(p, s)
    nx = st.shape[-1]
    vals = restated_loss(pred, s.detach(), sn.double(), dx, dt, nu, w, poisson_column(nx, nx * dx))
    vals[0].backward()
    return pred.detach().numpy(), np.array([float(v.detach()) for v in vals]), {k: v.grad.numpy() for k, v in p.items()}, \
        s.grad.numpy()


@pytest.mark.parametrize("D,H,L,B", SHAPES)
def test_shapes_vs_restatement(hf, D, H, L, B):
    """pinn_forward + pinn_physics_loss + backward() on every path's shapes (the f32
    MFMA GEMMs for D % 32 == H % 32 == 0, the generic kernels otherwise) against
    float64 autograd of the restatement: prediction, losses, dL/dparams, dL/dstate."""
    from hybridflux import training as T
    m, st, sn = shape_case(hf, D, H, L, B)
    dx = 2 * math.pi / (D // 3)
    pred_r, vals_r, gp_r, gs_r = restated_run(m, st, sn, dx, DT, NU, WEIGHTS)
    m = m.to(DEV)
    s = st.to(DEV).requires_grad_(True)
    pred = T.pinn_forward(m, s)
    close(pred, pred_r, 2e-6, 1e-5, what="pred")
    loss, terms = T.pinn_physics_loss(pred, s, sn.to(DEV), dx, DT, NU, WEIGHTS)
    close(torch.cat([loss.detach().reshape(1), terms]), vals_r, 0.0, 1e-5, what="losses")
    loss.backward()
    grad_close(s.grad, gs_r, "grad_state")
    for k, p in m.named_parameters():
        grad_close(p.grad, gp_r[k], f"grad.{k}")


def loss_case(nx, B=3, seed=11):
    g = torch.Generator().manual_seed(seed + nx)
    st = torch.stack([1 + 0.1 * torch.randn(B, nx, generator=g), 0.1 * torch.randn(B, nx, generator=g),
                      0.1 * torch.randn(B, nx, generator=g)], dim=1)
    sn = st + 0.01 * torch.randn(B, 3, nx, generator=g)
    pred = st + 0.02 * torch.randn(B, 3, nx, generator=g)
    return pred, st, sn


def check_loss(pred, st, sn, dx, w, tag="", dt=DT, col=None):
    from hybridflux import engine
    nx = pred.shape[-1]
    p64 = pred.double().requires_grad_(True)
    col = poisson_column(nx, nx * dx) if col is None else col
    vals = restated_loss(p64, st.double(), sn.double(), dx, dt, NU, w, col)
    vals[0].backward()
    losses, gp = engine.pinn_loss(pred.to(DEV), st.to(DEV), sn.to(DEV), dx, dt, NU, w)
    close(losses, np.array([float(v.detach()) for v in vals]), 0.0, 1e-5, what=f"losses{tag}")
    grad_close(gp, p64.grad.numpy(), f"grad_pred{tag}")
    return losses, gp


@pytest.mark.parametrize("nx", [1, 2, 5, 21, 32, 64, 100, 256, 1024])
def test_loss_kernel_vs_restatement(nx):
    """hf_pinn_loss alone, B = 3: the five losses and dL/dpred at nx = 1 and 2 (every
    difference and P vanish), odd sizes, sizes past one pass of the 256 threads
    (1024) and the solver's FFT sizes (256, 1024: the loss applies the circulant)."""
    pred, st, sn = loss_case(nx)
    check_loss(pred, st, sn, 2 * math.pi / nx, WEIGHTS)


def test_loss_each_term_alone():
    """Each of the four weights the only non-zero one: a wrong term cannot hide behind another."""
    pred, st, sn = loss_case(21)
    for k in range(4):
        w = tuple(1.0 if j == k else 0.0 for j in range(4))
        check_loss(pred, st, sn, 2 * math.pi / 21, w, tag=f"_{KEYS5[k + 1]}")


def test_loss_cell0_rule():
    """A large p_E[0]: X[0] = 0 (the Poisson loss holds p_E[0]^2 whole), r~[0] = 0 in the
    P r~ term (dL/dp_n does not see p_E[0] at all: bit-equal with and without it) and
    cell 0 is kept in dL/dp_E (= 2 w_p p_E[0] / N1)."""
    pred, st, sn = loss_case(32)
    big = pred.clone()
    big[:, 2, 0] = 50.0
    dx = 2 * math.pi / 32
    w = (0.0, 0.0, 0.0, 1.0)
    _, g0 = check_loss(pred, st, sn, dx, w, tag="_plain")
    losses, g1 = check_loss(big, st, sn, dx, w, tag="_big")
    assert torch.equal(g0[:, 0], g1[:, 0])
    n1 = 3 * 32
    close(g1[:, 2, 0], np.full(3, 2 * 50.0 / n1), 0.0, 1e-6, what="grad_pE0")
    assert float(losses[4]) > 3 * 50.0 ** 2 / n1


@pytest.mark.parametrize("D,H,L,B", [(96, 64, 3, 130), (144, 96, 3, 7)])
def test_deterministic(hf, D, H, L, B):
    """Two calls of forward_train, loss and backward give equal bits, on a GEMM shape
    (two weight-gradient splits) and on a generic one."""
    from hybridflux import engine
    m, st, sn = shape_case(hf, D, H, L, B)
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).to(DEV)
    s = st.to(DEV).reshape(B, D).contiguous()
    dx = 2 * math.pi / (D // 3)

    def run():
        out, tape = engine.pinn_forward_train(flat, (D, H, L), s)
        losses, gp = engine.pinn_loss(out.reshape(B, 3, -1), st.to(DEV), sn.to(DEV), dx, DT, NU, WEIGHTS)
        gw, gs = engine.pinn_backward(flat, (D, H, L), s, tape, gp.reshape(B, D), True)
        return out, losses, gp, gw, gs

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_six_adam_steps_vs_reference(hf, fx):
    """pinn_step with FlatAdam on the flattened model on the fixture's six batches
    against the reference's loop (torch.optim.Adam(lr=1e-3)): per-step loss values
    rtol 1e-4, final weights atol 2e-5, every element; the same six steps through the
    captured step (three eager steps, the capture, three replays) are bit-equal."""
    from hybridflux import training as T
    dx, dt, nu = consts(fx)
    batches = [tuple(t.to(DEV) for t in fixture_batch(fx, k)) for k in range(6)]

    def six(graphed):
        m = fixture_model(hf, fx).to(DEV).flatten_parameters_()
        opt = T.FlatAdam(m.parameters(), lr=1e-3)
        rows = []
        if not graphed:
            for st, sn in batches:
                rows.append(T.pinn_step(m, opt, st, sn, dx, dt, nu))
        else:
            gs = T.GraphedPinnStep(m, opt, (32, 3, 32), dx, dt, nu, device=DEV)
            for k, (st, sn) in enumerate(batches):
                if k == 3:
                    torch.cuda.synchronize()
                    gs.capture()
                if gs.graph is None:
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        rows.append(gs(st, sn))
                    torch.cuda.current_stream().wait_stream(side)
                else:
                    rows.append(gs(st, sn))
        return torch.stack(rows).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    rows, sd = six(False)
    close(rows, fx["adam_losses"], 0.0, 1e-4, what="losses")
    for k, v in sd.items():
        close(v, fx[f"adam_final.{k}"], 2e-5, 0.0, what=f"final.{k}")
    rows_g, sd_g = six(True)
    assert torch.equal(rows, rows_g)
    for k in sd:
        assert torch.equal(sd[k], sd_g[k]), k


def test_step_with_hooks_takes_autograd(hf, fx):
    """A parameter hook (or anomaly mode) sends pinn_step through the autograd
    composition, which runs the hook; losses and gradients are the direct path's bit
    for bit (the same kernels; autograd's seed of 1 multiplies exactly)."""
    from hybridflux import training as T
    dx, dt, nu = consts(fx)
    st, sn = (t.to(DEV) for t in fixture_batch(fx, 0))

    def run(hook):
        m = fixture_model(hf, fx).to(DEV)
        calls = []
        if hook:
            m.net[0].weight.register_hook(lambda g: calls.append(1))
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        assert T._pinn_direct_ok(m, opt) == (not hook)
        losses = T.pinn_step(m, opt, st, sn, dx, dt, nu)
        return losses, [p.grad.clone() for p in m.parameters()], calls

    l0, g0, c0 = run(False)
    l1, g1, c1 = run(True)
    assert c0 == [] and c1 == [1]
    assert torch.equal(l0, l1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    with torch.autograd.detect_anomaly(check_nan=False):
        m = fixture_model(hf, fx).to(DEV)
        assert not T._pinn_direct_ok(m, torch.optim.SGD(m.parameters(), lr=0.0))


def test_train_pinn(hf, fx):
    """train_pinn, 2 epochs on 64 samples at nx = 32: the reference's history keys,
    finite values, a falling loss, the reference PINN's state-dict keys and shapes;
    the checkpoint loads into hybridflux.PINN and rolls out scored, unchanged."""
    from hybridflux import training as T
    dx, dt, nu = consts(fx)
    traj = fx["traj"]
    st, sn = traj[:, :-1].reshape(-1, 3, 32)[:64], traj[:, 1:].reshape(-1, 3, 32)[:64]
    model, hist = T.train_pinn(st, sn, dx, dt, nu, epochs=2, batch_size=32, hidden_dim=64, num_layers=3, seed=3,
                               device=DEV)
    assert sorted(hist) == sorted(["loss", "loss_data", "loss_continuity", "loss_momentum", "loss_poisson"])
    for k, v in hist.items():
        assert len(v) == 2 and np.isfinite(v).all(), k
    assert hist["loss"][1] < hist["loss"][0]
    sd = model.state_dict()
    ref = {k[5:]: fx[k].shape for k in fx.files if k.startswith("init.")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    m2 = hf.PINN(96, 64, 3)
    m2.load_state_dict({k: v.detach().cpu().clone() for k, v in sd.items()})
    base = hf.BaselineSolver(nx=32, dt=dt, nu=nu, device=DEV)
    out = m2.to(DEV).rollout(torch.as_tensor(st[:4], device=DEV), 5, metrics=True, compare=base)
    for k in ("final", "traj", "metrics", "mse", "metrics_classical"):
        assert torch.isfinite(out[k]).all(), k


def test_inference_guard_stays(hf, fx):
    """PINN.forward is the inference call: with grad enabled and trainable parameters it
    raises, before and after flatten_parameters_(); training goes through
    hybridflux.training.pinn_forward, and under no_grad forward() runs as before."""
    from hybridflux import training as T
    m = fixture_model(hf, fx).to(DEV)
    st, _ = fixture_batch(fx, 0)
    st = st.to(DEV)
    with pytest.raises(NotImplementedError):
        m(st)
    m.flatten_parameters_()
    with pytest.raises(NotImplementedError):
        m(st)
    with torch.no_grad():
        inf = m(st)
    close(T.pinn_forward(m, st), inf.cpu().numpy(), 2e-6, 1e-5, what="train_vs_inference")
