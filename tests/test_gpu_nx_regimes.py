"""The training-side loss kernels over the whole range of nx their launchers
accept (tests/nx_regimes.py has the regimes, the boundaries and the cases):
hf_ablation_loss in each of its four Poisson paths, hf_pinn_loss and the PINN
unroll loss / adjoint up to the LDS limit 6144.  The other wide cases extend
the parametrisations where the kernels' tests already live:
hf_unroll_update / hf_unroll_adjoint and the K-step FluxGNN gradients in
test_gpu_unrolled_training.py (UNROLL_WIDE, UPDATE_BITWISE_WIDE,
UNROLLED_GRAD_WIDE), the PureGNN unroll kernels in
test_gpu_pure_unrolled_training.py (PURE_WIDE).

Every reference is float64 on the CPU and independent of the engine's Poisson
kernels: the ablation loss against ablation_terms64 below (torch FFT solve;
test_nx_regimes_cpu.py ties it to the oracle's per-sample loss and the solve to
a dense circulant product), the PINN kernels against pinn_unroll_ref and
test_gpu_pinn_training's restated_loss.

Gates, the project's existing ones:
  ablation loss, flux loss .............. rtol 2e-6 (test_gpu_training's gate on the same
      kernels against the torch form: float32 sums of nx / 256 terms per thread and a
      fixed tree, a few ulp of float32 relative)
  ablation d loss / d flux_edge ......... 2e-5 max|ref| per tensor (the gradient gate:
      an elementwise float32 expression of O(1) values; an elementwise relative gate
      has no meaning against float64 where the two terms of an element cancel)
  hf_pinn_loss .......................... losses rtol 1e-5, dL/dpred 2e-5 max|ref| + 1e-9
      (test_gpu_pinn_training's check_loss)
  PINN unroll loss ...................... rtol 1e-6; adjoint 2e-5 max|ref| + 1e-12 max|g|
      (test_gpu_pinn_unrolled_training's gates)
Every loss value is bitwise repeatable across two launches.  Every measured
error is recorded (conftest `record` / close)."""
import numpy as np
import pytest
import torch

import pinn_unroll_ref as R
import test_gpu_pinn_training as PT
import test_gpu_pinn_unrolled_training as PU
from conftest import close
from nx_regimes import LOSS_WIDE, LOSS_WIDE_B, LOSS_WIDE_FULL, PINN_WIDE, PINN_WIDE_B, dt_of, long_wave
from test_gpu_unrolled_training import grid_of, poisson_t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2e-5
LOSS_RTOL = 2e-6


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


# ------------------------------------------------ the ablation loss in float64 (CPU)
def ablation_terms64(fe, st, ft, sn, c, dt, dx, k, cfg):
    """The loss of scripts/training/train_ablation.py:120-206 per sample, from the
    edge fluxes fe [B,2nx] directly (no model), in torch float64: returns (loss [B],
    flux_loss [B]); the batch loss is their mean.  st, sn [B,3,nx], ft [B,nx]; c =
    dt / dx and dt as the caller rounds them; k the wavenumbers (oracle Grid.k).
    The predicted E' is detached, as the reference's solve_poisson_np is.  The
    rollout energy term needs rollout_steps <= 3: e_0, e_1, e_2 then depend on the
    model through this same fe only (u_2 reads E' of the n' the loss already has)."""
    f64 = lambda a: torch.as_tensor(a, dtype=torch.float64)  # noqa: E731
    st, ft, sn, k = f64(st), f64(ft), f64(sn), f64(k)
    nx = st.shape[-1]
    n, u, E = st[:, 0], st[:, 1], st[:, 2]
    mse = lambda a, b: ((a - b) ** 2).mean(-1)  # noqa: E731
    F = 0.5 * (fe[:, :nx] + fe[:, nx:])
    flux_loss = mse(F, ft)
    loss = flux_loss
    n1 = n - c * (F - torch.roll(F, 1, -1))
    E1 = poisson_t(n1.detach(), k)
    if cfg["lambda_state"] > 0:
        loss = loss + cfg["lambda_state"] * mse(n1, sn[:, 0])
    if cfg["lambda_poisson"] > 0:
        loss = loss + cfg["lambda_poisson"] * mse(E1, sn[:, 2])
    if cfg["lambda_charge"] > 0:
        loss = loss + cfg["lambda_charge"] * ((n1 - 1.0).sum(-1) * dx - (n - 1.0).sum(-1) * dx) ** 2
    if cfg["lambda_energy_one"] > 0:
        e_p = 0.5 * (sn[:, 1] ** 2 + E1 ** 2).mean(-1)
        e_t = 0.5 * (sn[:, 1] ** 2 + sn[:, 2] ** 2).mean(-1)
        loss = loss + cfg["lambda_energy_one"] * (e_p - e_t) ** 2
    K = cfg["rollout_steps"]
    if K > 0 and cfg["lambda_energy_multi"] > 0:
        assert K <= 3
        us, Es = [u], [E, E1]
        for j in range(1, K):
            Fu = 0.5 * us[-1] ** 2
            us.append(us[-1] - c * (Fu - torch.roll(Fu, 1, -1)) + dt * Es[j - 1])
        en = torch.stack([0.5 * (v ** 2).mean(-1) for v in us])  # [K, B]
        loss = loss + cfg["lambda_energy_multi"] * ((en - en[0]) ** 2).mean(0)
    return loss, flux_loss


def loss_inputs(nx, B):
    """Random states around 1 (test_gpu_training's test_loss_terms_any_nx), with
    nx_regimes.long_wave on the density, so that the predicted E' has amplitude 0.4
    and the Poisson and energy terms feel it (the test asserts by how much), and a
    wide velocity channel, so that the rollout energies move: e_1 - e_0 is about
    -c var(u), which a unit variance puts at 0.05."""
    g = torch.Generator().manual_seed(nx)
    st = 1.0 + 0.1 * torch.randn(B, 3, nx, generator=g)
    st[:, 0] += torch.as_tensor(long_wave(nx, B), dtype=torch.float32)
    st[:, 1] = 0.5 + torch.randn(B, nx, generator=g)
    sn = 1.0 + 0.1 * torch.randn(B, 3, nx, generator=g)
    ft = 0.1 * torch.randn(B, nx, generator=g)
    fe = 0.1 * torch.randn(B, 2 * nx, generator=g)
    return st, ft, sn, fe


_LOSS_CASES = [(nx, "physics") for nx in LOSS_WIDE] + [(nx, "full") for nx in LOSS_WIDE_FULL]


@pytest.mark.parametrize("nx,cfg_name", _LOSS_CASES)
def test_ablation_loss_wide(hf, record, request, nx, cfg_name):
    """hf_ablation_loss_ex against ablation_terms64: loss, flux loss and d loss /
    d flux_edge, B = 5, in every Poisson path: the one-launch kernel at its largest
    size 2047, three launches around poisson_fft_kernel (512, 1024, 2048), around
    poisson_kernel (2049, 6144) and around poisson_tiled_kernel (6160).  'full' adds
    the rollout energy term formed by loss_terms_kernel (K = 3) in both the FFT and
    the circulant three-launch path; the inputs make it at least 1e-4 of the loss
    (asserted on the reference), 50 times the gate."""
    from hybridflux import engine
    from oracle import hybrid_oracle as O
    B = LOSS_WIDE_B
    cfg = hf.ABLATION_CONFIGS[cfg_name]
    st, ft, sn, fe0 = loss_inputs(nx, B)
    grid = grid_of(hf, nx)  # (dt_of(nx): every size here is past 256)
    assert grid.dt == dt_of(nx)
    lam = (cfg["lambda_state"], cfg["lambda_poisson"], cfg["lambda_charge"], cfg["lambda_energy_one"],
           cfg["lambda_energy_multi"])
    K = cfg["rollout_steps"] if cfg["lambda_energy_multi"] > 0 else 0
    runs = []
    for _ in range(2):
        loss, fl, dfe = engine.ablation_loss_terms(grid, fe0.to(DEV), st.to(DEV), ft.to(DEV), sn.to(DEV), lam, K)
        runs.append((loss.cpu().numpy().copy(), fl.cpu().numpy().copy(), dfe.cpu().numpy().copy()))
    G = O.Grid(nx, dt=dt_of(nx))
    fe = fe0.double().requires_grad_(True)
    l64, f64 = ablation_terms64(fe, st, ft, sn, grid.c32, grid.dt32, float(np.float32(G.dx)), G.k, cfg)
    l64.mean().backward()
    want_l, want_f, want_g = float(l64.mean().detach()), float(f64.mean().detach()), fe.grad.numpy()
    name = request.node.nodeid.split("::", 1)[-1]
    # the case has teeth: an E' off by one part in a thousand (k scaled) moves the
    # reference loss by more than ten times the gate
    off, _ = ablation_terms64(fe.detach(), st, ft, sn, grid.c32, grid.dt32, float(np.float32(G.dx)), G.k * 1.001, cfg)
    moved = abs(float(off.mean()) - want_l) / want_l
    record(name, "loss_moved_by_E_off_1e-3", moved)
    assert moved >= 10 * LOSS_RTOL
    if K:
        base, _ = ablation_terms64(fe.detach(), st, ft, sn, grid.c32, grid.dt32, float(np.float32(G.dx)), G.k,
                                   dict(cfg, lambda_energy_multi=0.0))
        share = (want_l - float(base.mean())) / want_l
        record(name, "rollout_term_share_of_loss", share)
        assert share >= 1e-4
    close(runs[0][0].reshape(1), np.asarray([want_l]), 0.0, LOSS_RTOL, what="loss")
    close(runs[0][1].reshape(1), np.asarray([want_f]), 0.0, LOSS_RTOL, what="flux_loss")
    close(runs[0][2], want_g, REL * float(np.abs(want_g).max()), 0.0, what="dfe")
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------- hf_pinn_loss
@pytest.mark.parametrize("nx", PINN_WIDE)  # (outer loop: both cases of a size share its dense circulant)
@pytest.mark.parametrize("phys", ["on", "off"])
def test_pinn_loss_wide(hf, nx, phys):
    """hf_pinn_loss (pinn_loss_kernel: the circulant in 16 nx bytes of LDS, 98,304 B at
    the limit 6144) at a power of two, an odd size past it and the limit, B = 3,
    against the float64 restatement: the five losses and dL/dpred, with the reference
    weights and with the data term alone (no residual, no O(nx^2) work)."""
    from hybridflux import engine
    pred, st, sn = PT.loss_case(nx, B=PINN_WIDE_B)
    wave = torch.as_tensor(long_wave(nx, PINN_WIDE_B), dtype=torch.float32)  # a P p_n of amplitude 0.4
    for t in (pred, st, sn):
        t[:, 0] += wave
    dx = PU.dx_of(nx)
    w = PT.WEIGHTS if phys == "on" else (1.0, 0.0, 0.0, 0.0)
    Pm = R.poisson_matrix(nx, nx * dx)
    losses, gp = PT.check_loss(pred, st, sn, dx, w, dt=dt_of(nx), col=Pm)
    again, gp2 = engine.pinn_loss(pred.to(DEV), st.to(DEV), sn.to(DEV), dx, dt_of(nx), PT.NU, w)
    assert torch.equal(losses, again) and torch.equal(gp, gp2)
    if phys == "off":
        assert float(losses[0]) == float(losses[1])


# ------------------------------------------------------ the PINN unroll loss / adjoint
@pytest.mark.parametrize("lam", ["zero", "ref"])
@pytest.mark.parametrize("nx", PINN_WIDE)
def test_pinn_unroll_loss_wide(hf, nx, lam):
    """hf_pinn_unroll_loss (pinn_unroll_loss_kernel) at kernel level, B = 3, K = 2:
    the five values against pinn_unroll_ref.step_terms in float64, twice with equal
    bits; without residual terms the total also agrees with hf_pure_unroll_update's
    loss on the same states to rtol 1e-6 (beyond 1024 cells that kernel cuts its
    partials per tile, so the bits may differ)."""
    from hybridflux import engine
    lam_v, B, K, dev = PU.LAMS[lam], PINN_WIDE_B, 2, PU.dev
    pred, st, tg = PU.states(nx, B, 3, 100 + nx)
    w = (1.0, 0.5, 2.0)
    dx, dt = PU.dx_of(nx), dt_of(nx)
    scale, ps = 1.0 / (K * 3 * B * nx), 1.0 / (K * B * nx)
    kw = {} if lam_v is None else dict(state=dev(st), phys=lam_v, phys_scale=ps, dx=dx, dt=dt, nu=PU.NU)
    runs = [engine.pinn_unroll_loss(dev(pred), dev(tg), w, scale, **kw).cpu().numpy().copy() for _ in range(2)]
    Pm = R.poisson_matrix(nx, nx * dx) if lam_v is not None else None
    want = R.step_terms(pred.double(), st.double(), tg.double(), w, lam_v, dx, dt, PU.NU, Pm, K)
    close(runs[0], np.array([float(v) for v in want]), 0.0, 1e-6, what="losses")
    assert np.array_equal(runs[0], runs[1])
    if lam_v is None:
        assert not runs[0][2:].any() and runs[0][0] == runs[0][1]
        _, _, pure = engine.pure_unroll_update(torch.zeros(B * nx, 3, device=DEV), dev(pred),
                                               torch.zeros(nx, device=DEV), target=dev(tg), weights=w, scale=scale,
                                               want_nf=False)
        close(pure.cpu().numpy(), runs[0][:1].astype(np.float64), 0.0, 1e-6, what="pure_loss")
    else:
        assert all(runs[0][2:] != 0.0)


@pytest.mark.parametrize("lam", ["zero", "ref"])
@pytest.mark.parametrize("nx", PINN_WIDE)
def test_pinn_unroll_adjoint_wide(hf, record, request, nx, lam):
    """hf_pinn_unroll_adjoint (pinn_unroll_adjoint_kernel) at kernel level, B = 3:
    test_gpu_pinn_unrolled_training's test_adjoint_kernel (the three parts one by one
    and together, every NULL combination, each call twice with equal bits) at the wide
    sizes; q_c and q_m reuse all 16 nx bytes of the circulant's LDS at 6144."""
    PU.test_adjoint_kernel(hf, record, request, nx, 0, 0, PINN_WIDE_B, 2, lam)
