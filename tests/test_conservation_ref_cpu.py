"""CPU checks of the energy and charge terms of unrolled training: the torch
restatement conservation_ref.py (against the existing float64 restatements of the
three K-step losses with lam = 0, against central finite differences in float64,
and its e and q against the oracle's metrics), the C ABI's argument checks and
size queries of hf_state_moments and the six _ex entry points (no kernel is
launched: the dummy pointers are never dereferenced), and the Python argument
errors."""
import ctypes
import math

import numpy as np
import pytest
import torch

import conservation_ref as C
import pinn_unroll_ref as R
from conftest import golden
from hybridflux import _lib
from oracle import hybrid_oracle as O

D = ctypes.c_void_p(1)
D2 = ctypes.c_void_p(2)
W = np.ones(3, dtype=np.float32)
WP = W.ctypes.data_as(ctypes.c_void_p)
DT, NU = 5e-3, 1e-3


def lam_ptr(a, b):
    v = np.asarray([a, b], dtype=np.float32)
    return v, v.ctypes.data_as(ctypes.c_void_p)


def windows(nx, B, K):
    G = O.Grid(nx)
    st = np.stack([O.initial_condition(G, s) for s in range(B)])
    traj, _ = O.classical_run(G, st, K)
    return G, traj


def small_flux(seed=0, H=8):
    g = np.random.default_rng(seed)
    sd = {"input_mlp.0.weight": g.normal(0, 0.5, (H, 4)), "input_mlp.0.bias": g.normal(0, 0.1, H),
          "update_mlps.0.0.weight": g.normal(0, 0.3, (H, 2 * H)), "update_mlps.0.0.bias": g.normal(0, 0.1, H),
          "edge_mlp.0.weight": g.normal(0, 0.3, (H, 2 * H)), "edge_mlp.0.bias": g.normal(0, 0.1, H),
          "edge_mlp.2.weight": g.normal(0, 0.3, (1, H)), "edge_mlp.2.bias": g.normal(0, 0.1, 1)}
    return {k: np.asarray(v, np.float64) for k, v in sd.items()}


def pure_sd():
    f = golden("pure_gnn_train.npz")
    return {k[len("init."):]: f[k] for k in f.files if k.startswith("init.")}


def pinn_sd(nx, H, L, seed=0):
    import hybridflux
    torch.manual_seed(seed)
    return {k: v.detach().numpy() for k, v in hybridflux.PINN(3 * nx, H, L).state_dict().items()}


# ----------------------------------------------------------------- 1. the restatement
def test_moments_are_the_oracle_metrics():
    _, traj = windows(48, 3, 4)
    e, q, _ = O.rollout_metrics(traj)
    m = C.moments_np(traj)
    assert np.abs(m[..., 0] - e).max() <= 1e-15 * np.abs(e).max()
    assert np.abs(m[..., 1] - q).max() <= 1e-15 * np.abs(q).max()


def test_lam_zero_is_the_existing_flux_restatement():
    from test_gpu_unrolled_training import unrolled_loss_cpu, w1r2
    nx, B, K = 16, 3, 2
    G, traj = windows(nx, B, K)
    sd, w = w1r2(), (1.0, 0.5, 2.0)
    for through in (True, False):
        l0, g0 = unrolled_loss_cpu(sd, G, traj, w, torch.float64, through)
        for ref in (None, C.offset_ref(traj)):
            l1, g1, _, rows = C.loss_and_grads(lambda p: C.flux_step(p, G, B, torch.float64), sd, traj, w, (0.0, 0.0),
                                               ref, torch.float64, through)
            assert l1 == l0 and rows.shape == (K, 4) and not rows[:, 2:].any()
            for k in g0:
                assert np.array_equal(g0[k], g1[k]), k


def test_lam_zero_is_the_existing_pure_restatement():
    from test_gpu_pure_unrolled_training import pure_unrolled_loss_cpu
    nx, B, K = 16, 3, 2
    G, traj = windows(nx, B, K)
    sd, w = pure_sd(), (1.0, 0.5, 2.0)
    for through in (True, False):
        l0, g0, s0 = pure_unrolled_loss_cpu(sd, G, traj, w, torch.float64, through)
        l1, g1, s1, _ = C.loss_and_grads(lambda p: C.pure_step(p, G, B, torch.float64), sd, traj, w, (0.0, 0.0),
                                         C.offset_ref(traj), torch.float64, through)
        assert l1 == l0 and np.array_equal(s1.transpose(1, 0, 2, 3), s0)
        for k in g0:
            assert np.array_equal(g0[k], g1[k]), k


@pytest.mark.parametrize("lam", [None, R.REF_LAMBDA])
def test_lam_zero_is_the_existing_pinn_restatement(lam):
    nx, B, K = 5, 2, 2
    dx = 2 * math.pi / nx
    _, traj = windows(nx, B, K)
    sd = pinn_sd(nx, 8, 2)
    tr = torch.as_tensor(traj, dtype=torch.float64)
    p0 = C.params(sd, torch.float64)
    l0, s0, t0 = R.unrolled_loss(C.pinn_step(p0), tr, (1.0, 0.5, 2.0), lam, dx, DT, NU)
    l0.backward()
    l1, g1, s1, rows = C.loss_and_grads(C.pinn_step, sd, traj, (1.0, 0.5, 2.0), (0.0, 0.0), C.offset_ref(traj),
                                        torch.float64, True, C.pinn_base(lam, dx, DT, NU, nx, torch.float64))
    assert l1 == float(l0.detach()) and np.array_equal(s1, s0.numpy())
    assert rows.shape == (K, 7) and np.array_equal(rows[:, :5], t0.numpy()) and not rows[:, 5:].any()
    for k, v in p0.items():
        assert np.array_equal(v.grad.numpy(), g1[k]), k


def fd_check(make_step, sd, traj, lam, ref, base=C.state_mse, w=(1.0, 1.0, 1.0), n=6, h=1e-6):
    """Central differences in float64 along n random parameter directions against autograd."""
    l, g, _, rows = C.loss_and_grads(make_step, sd, traj, w, lam, ref, torch.float64, True, base)
    assert rows[:, -2:].sum() > 0.1 * l  # the terms are a real share of the loss
    rng = np.random.default_rng(1)
    tr, rf = torch.as_tensor(traj, dtype=torch.float64), torch.as_tensor(ref)
    for _ in range(n):
        d = {k: rng.normal(size=np.shape(v)) for k, v in sd.items()}
        vals = []
        for sgn in (1.0, -1.0):
            p = {k: torch.as_tensor(np.asarray(v, np.float64) + sgn * h * d[k]) for k, v in sd.items()}
            vals.append(float(C.unrolled_loss(make_step(p), tr, w, lam, rf, True, base)[0]))
        fd = (vals[0] - vals[1]) / (2 * h)
        an = sum(float((g[k] * d[k]).sum()) for k in sd)
        # truncation h^2 L''' and rounding eps L / h, both far below 1e-6 of a directional derivative of O(L)
        assert abs(fd - an) <= 1e-6 * abs(an) + 1e-9 * l, (fd, an)


def test_gradient_vs_finite_differences_flux():
    nx, B, K = 16, 2, 3
    G, traj = windows(nx, B, K)
    fd_check(lambda p: C.flux_step(p, G, B, torch.float64), small_flux(), traj, (50.0, 50.0), C.offset_ref(traj))


def test_gradient_vs_finite_differences_pure():
    nx, B, K = 16, 2, 3
    G, traj = windows(nx, B, K)
    sd = {k: np.asarray(v, np.float64) for k, v in pure_sd().items()}
    fd_check(lambda p: C.pure_step(p, G, B, torch.float64), sd, traj, (1.0, 1.0), C.offset_ref(traj))


@pytest.mark.parametrize("phys,lam", [(None, (1.0, 1.0)), (R.REF_LAMBDA, (5e3, 5e3))])
def test_gradient_vs_finite_differences_pinn(phys, lam):
    """With the residuals on (their 1 / dt^2 makes them hundreds) the lambdas are raised to keep the terms a real share."""
    nx, B, K = 5, 2, 2
    dx = 2 * math.pi / nx
    _, traj = windows(nx, B, K)
    sd = {k: np.asarray(v, np.float64) for k, v in pinn_sd(nx, 8, 2).items()}
    fd_check(C.pinn_step, sd, traj, lam, C.offset_ref(traj), C.pinn_base(phys, dx, DT, NU, nx, torch.float64))


def test_coefficients_are_the_gradient_of_the_terms():
    """The header's rank-one form: d (energy + charge) / d s = (cq, ce u, ce E)."""
    _, traj = windows(16, 3, 2)
    s = torch.as_tensor(traj[:, 1], dtype=torch.float64).requires_grad_(True)
    ref, lam, K = C.offset_ref(traj)[:, 0], (0.7, 1.3), 2
    en, ch = C.cons_terms(s, torch.as_tensor(ref), lam, K)
    (en + ch).backward()
    want = C.seed_np(s.detach().numpy(), C.cons_coef(s.detach().numpy(), ref, lam, K))
    assert np.abs(s.grad.numpy() - want).max() <= 1e-14 * np.abs(want).max()


def test_charge_has_no_gradient_through_the_hybrid_step():
    nx, B, K = 16, 2, 3
    G, traj = windows(nx, B, K)
    mk = lambda p: C.flux_step(p, G, B, torch.float64)  # noqa: E731
    zero = (0.0, 0.0, 0.0)
    _, gq, _, rows = C.loss_and_grads(mk, small_flux(), traj, zero, (0.0, 1.0), C.offset_ref(traj), torch.float64)
    _, ge, _, _ = C.loss_and_grads(mk, small_flux(), traj, zero, (1.0, 0.0), C.offset_ref(traj), torch.float64)
    assert rows[:, 3].sum() > 0
    top = max(np.abs(v).max() for v in ge.values())
    assert top > 0 and max(np.abs(v).max() for v in gq.values()) <= 1e-12 * top


# ------------------------------------------------------------------------- 2. the ABI
NAMES = ("hf_state_moments", "hf_unroll_workspace_bytes_ex", "hf_unroll_update_ex", "hf_unroll_adjoint_ex",
         "hf_pure_unroll_workspace_bytes_ex", "hf_pure_unroll_update_ex", "hf_pure_unroll_adjoint_ex",
         "hf_pinn_unroll_workspace_bytes_ex", "hf_pinn_unroll_loss_ex", "hf_pinn_unroll_adjoint_ex")


def test_symbols_exported():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(L, n), n


def test_workspace_queries():
    L = _lib.lib()
    for kind, per_ic in (("unroll", 2), ("pure_unroll", 3), ("pinn_unroll", 2)):
        plain, ex = getattr(L, f"hf_{kind}_workspace_bytes"), getattr(L, f"hf_{kind}_workspace_bytes_ex")
        for B, nx in ((1, 1), (3, 16), (4096, 64), (3, 256), (2, 1030)):
            assert ex(B, nx) >= plain(B, nx) + per_ic * 8 * B, (kind, B, nx)
        for B, nx in ((0, 64), (3, 0), (-1, 64), (3, -7)):
            assert ex(B, nx) == -1
    assert L.hf_pure_unroll_workspace_bytes_ex(3, 10000) >= L.hf_pure_unroll_workspace_bytes(3, 10000) + 3 * 10 * 24
    assert L.hf_pure_unroll_workspace_bytes_ex(2 ** 31 - 1, 1025) == -1
    assert L.hf_pure_unroll_workspace_bytes_ex(2 ** 31 - 1, 1024) > 32 * (2 ** 31 - 1)  # no int overflow


def _refused(L, rc, name, word=None):
    assert rc == _lib.HF_EINVAL, rc
    err = L.hf_last_error()
    assert name in err, err
    if word:
        assert word in err, err


def test_state_moments_validates_before_device():
    L = _lib.lib()
    name = b"hf_state_moments"
    _refused(L, L.hf_state_moments(None, 3, 16, D, None), name, b"NULL")
    _refused(L, L.hf_state_moments(D, 3, 16, None, None), name, b"NULL")
    for rows, nx in ((0, 16), (-1, 16), (3, 0), (3, -5)):
        _refused(L, L.hf_state_moments(D, rows, nx, D, None), name)
    _refused(L, L.hf_state_moments(D, 2 ** 34, 16, D, None), name)


def _calls(L):
    """kind -> (name, f(cons, ref, coef, ws, ws_short, tg, B, nx)) of the three forward _ex calls with dummy pointers."""
    def unroll(cons, ref, coef, ws, short, tg, B, nx):
        nb = int(L.hf_unroll_workspace_bytes_ex(max(B, 1), max(nx, 1))) - short
        return L.hf_unroll_update_ex(D, D, D, D, 0, B, nx, 0.1, 0.1, D2, D, tg, WP, 1.0, D, ws, nb, cons, 1.0, ref, coef,
                                     None)

    def pure(cons, ref, coef, ws, short, tg, B, nx):
        nb = int(L.hf_pure_unroll_workspace_bytes_ex(max(B, 1), max(nx, 1))) - short
        return L.hf_pure_unroll_update_ex(D, D, D, B, nx, D2, D, tg, WP, 1.0, D, ws, nb, cons, 1.0, ref, coef, None)

    def pinn(cons, ref, coef, ws, short, tg, B, nx):
        nb = int(L.hf_pinn_unroll_workspace_bytes_ex(max(B, 1), max(nx, 1))) - short
        return L.hf_pinn_unroll_loss_ex(D, None, tg, B, nx, WP, 1.0, None, 0.0, 0.0, 0.0, 0.0, None, D, ws, nb, cons, 1.0,
                                        ref, coef, None)
    return {"unroll": (b"hf_unroll_update_ex", unroll), "pure": (b"hf_pure_unroll_update_ex", pure),
            "pinn": (b"hf_pinn_unroll_loss_ex", pinn)}


@pytest.mark.parametrize("kind", ["unroll", "pure", "pinn"])
def test_forward_ex_validates_before_device(kind):
    L = _lib.lib()
    name, f = _calls(L)[kind]
    _keep, lam = lam_ptr(1.0, 0.5)
    ok = dict(cons=lam, ref=D, coef=D, ws=D, short=0, tg=D, B=3, nx=16)

    def call(**kw):
        return f(*[{**ok, **kw}[k] for k in ("cons", "ref", "coef", "ws", "short", "tg", "B", "nx")])
    for kw in ("ref", "coef", "ws", "tg"):                      # cons without what it needs
        _refused(L, call(**{kw: None}), name, b"NULL")
    for bad in ((-1.0, 0.5), (1.0, -1e-30), (float("nan"), 0.5), (1.0, float("nan"))):
        _k, p = lam_ptr(*bad)
        _refused(L, call(cons=p), name, b"lam")
    # the plain workspace size is not enough with cons, and one byte less than the _ex size is not either
    plain = {"unroll": L.hf_unroll_workspace_bytes, "pure": L.hf_pure_unroll_workspace_bytes,
             "pinn": L.hf_pinn_unroll_workspace_bytes}[kind](3, 16)
    ex = {"unroll": L.hf_unroll_workspace_bytes_ex, "pure": L.hf_pure_unroll_workspace_bytes_ex,
          "pinn": L.hf_pinn_unroll_workspace_bytes_ex}[kind](3, 16)
    _refused(L, call(short=1), name, b"workspace")
    _refused(L, call(short=ex - plain), name, b"workspace")
    _refused(L, call(cons=None, short=ex - plain + 1), name, b"workspace")  # below the plain size without cons too
    for kw in ("ref", "coef"):                                  # the buffers without cons
        _refused(L, call(cons=None, **{"ref": None, "coef": None, kw: D}), name, b"without cons")
    for B, nx in ((0, 16), (-2, 16), (3, 0), (3, -1)):
        _refused(L, call(B=B, nx=nx), name)


def test_required_pointers_of_the_ex_calls():
    L = _lib.lib()
    nb = 1 << 20
    for i in (0, 1, 2, 3, 9):  # fe, st, x, plan, state_next
        a = [D, D, D, D, 0, 3, 16, 0.1, 0.1, D2, D, D, WP, 1.0, D, D, nb, None, 0.0, None, None, None]
        a[i] = None
        _refused(L, L.hf_unroll_update_ex(*a), b"hf_unroll_update_ex", b"NULL")
    a = [D, D, D, D, 0, 3, 16, 0.1, 0.1, D, D, D, WP, 1.0, D, D, nb, None, 0.0, None, None, None]
    _refused(L, L.hf_unroll_update_ex(*a), b"hf_unroll_update_ex", b"alias")
    a = [D, D, D, D, 1, 3, 16, 0.1, 0.1, D2, D, D, WP, 1.0, D, D, nb, None, 0.0, None, None, None]
    assert L.hf_unroll_update_ex(*a) == _lib.HF_EUNSUPPORTED       # the tridiagonal mode, as the plain call
    a = [D, D, D, D, 0, 3, 6145, 0.1, 0.1, D2, D, D, WP, 1.0, D, D, nb, None, 0.0, None, None, None]
    assert L.hf_unroll_update_ex(*a) == _lib.HF_EUNSUPPORTED       # the nx limit is unchanged
    for i in (0, 1, 2, 3, 7, 13):  # st, st_next, target, weights, plan, g_fe
        a = [D, D, D, WP, 1.0, D, D, D, 0, 3, 16, 0.1, 0.1, D, D, D, None]
        a[i] = None
        _refused(L, L.hf_unroll_adjoint_ex(*a), b"hf_unroll_adjoint_ex", b"NULL")
    for i in (0, 1, 2, 5):  # delta, st, x, state_next
        a = [D, D, D, 3, 16, D2, D, D, WP, 1.0, D, D, nb, None, 0.0, None, None, None]
        a[i] = None
        _refused(L, L.hf_pure_unroll_update_ex(*a), b"hf_pure_unroll_update_ex", b"NULL")
    for i in (0, 1, 2, 8):  # st_next, target, weights, gd
        a = [D, D, WP, 1.0, D, D, 3, 16, D, D, None]
        a[i] = None
        _refused(L, L.hf_pure_unroll_adjoint_ex(*a), b"hf_pure_unroll_adjoint_ex", b"NULL")
    _refused(L, L.hf_pure_unroll_adjoint_ex(D, D, WP, 1.0, D, D, 2 ** 31 - 1, 1025, D, D, None),
             b"hf_pure_unroll_adjoint_ex")
    for i in (0, 2, 5, 13, 14):  # pred, target, weights, losses, ws
        a = [D, None, D, 3, 16, WP, 1.0, None, 0.0, 0.0, 0.0, 0.0, None, D, D, nb, None, 0.0, None, None, None]
        a[i] = None
        _refused(L, L.hf_pinn_unroll_loss_ex(*a), b"hf_pinn_unroll_loss_ex", b"NULL")
    for i in (0, 2, 7, 15):  # pred, target, weights, grad_out
        a = [D, None, D, None, None, 3, 16, WP, 1.0, None, 0.0, 0.0, 0.0, 0.0, None, D2, D, None]
        a[i] = None
        _refused(L, L.hf_pinn_unroll_adjoint_ex(*a), b"hf_pinn_unroll_adjoint_ex", b"NULL")
    a = [D, None, D, None, None, 3, 16, WP, 1.0, None, 0.0, 0.0, 0.0, 0.0, None, D2, D2, None]
    _refused(L, L.hf_pinn_unroll_adjoint_ex(*a), b"hf_pinn_unroll_adjoint_ex", b"alias")  # coef == grad_out
    a = [D, None, D, 3, 6145, WP, 1.0, None, 0.0, 0.0, 0.0, 0.0, None, D, D, nb, None, 0.0, None, None, None]
    assert L.hf_pinn_unroll_loss_ex(*a) == _lib.HF_EUNSUPPORTED


# ------------------------------------------------------------------ 3. the Python layer
def test_python_argument_errors():
    import hybridflux
    from hybridflux import training
    traj, x = torch.zeros(2, 3, 3, 16), torch.zeros(16)
    flux, pure, pinn = hybridflux.FluxGNN(4, 128, 4), hybridflux.PureGNN(4, 64, 1), hybridflux.PINN(48, 8, 1)
    calls = [lambda **kw: training.unrolled_loss(flux, traj, x, None, **kw),
             lambda **kw: training.unrolled_step(flux, None, traj, x, None, **kw),
             lambda **kw: training.pure_unrolled_loss(pure, traj, x, **kw),
             lambda **kw: training.pure_unrolled_step(pure, None, traj, x, **kw),
             lambda **kw: training.pinn_unrolled_loss(pinn, traj, **kw),
             lambda **kw: training.pinn_unrolled_step(pinn, None, traj, **kw)]
    for f in calls:
        for bad in ((1.0,), (1.0, 2.0, 3.0), (-1.0, 0.0), (0.0, float("nan"))):
            with pytest.raises(ValueError, match="conservation"):
                f(conservation=bad)
        with pytest.raises(ValueError, match="conservation_ref"):
            f(conservation=(1.0, 1.0), conservation_ref="end")
        with pytest.raises(ValueError, match="conservation_ref"):
            f(conservation=(1.0, 1.0), conservation_ref=[[0.0, 0.0]])
        with pytest.raises(ValueError, match="conservation_ref"):
            f(conservation_ref="start")  # a reference without the terms
    ref = torch.zeros(2, 2, 2, dtype=torch.float64)
    trainers = [lambda **kw: training.train_unrolled(np.zeros((2, 4, 3, 16), np.float32), x, 5e-3, 0.1, 1e-3, **kw),
                lambda **kw: training.train_pure_gnn_unrolled(np.zeros((2, 4, 3, 16), np.float32), x, **kw),
                lambda **kw: training.train_pinn_unrolled(np.zeros((2, 4, 3, 16), np.float32), 0.1, 5e-3, 1e-3, **kw)]
    for f in trainers:  # refused before anything touches a device
        with pytest.raises(ValueError, match="conservation_ref"):
            f(conservation=(1.0, 1.0), conservation_ref=ref)
        with pytest.raises(ValueError, match="conservation"):
            f(conservation=(1.0, -1.0))
