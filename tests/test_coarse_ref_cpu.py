"""The coarse-graining of fine classical rollouts, on the CPU (no device):
the numpy restatement (tests/coarse_ref.py) checked against itself and the
oracle, the coarse continuity identity, the C ABI's validation and size query
(hf_coarsen_traj, hf_run_coarse, hf_run_coarse_workspace_bytes), and the Python
layer's defaults and its non-finite check.
"""
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import coarse_ref as CR
from conftest import ROOT
from oracle import hybrid_oracle as O

NAMES = ("hf_coarsen_traj", "hf_run_coarse_workspace_bytes", "hf_run_coarse")


# ------------------------------------------------------------------ the restatement
def test_tree_equals_mean_where_every_order_is_exact():
    g = np.random.default_rng(0)
    x = g.integers(-1000, 1000, size=(3, 2, 128)).astype(np.float32)
    for r in (1, 2, 4, 8, 16, 32, 64):
        want = x.astype(np.float64).reshape(3, 2, 128 // r, r).mean(axis=-1)
        assert np.array_equal(CR.box_mean(x, r).astype(np.float64), want.astype(np.float32).astype(np.float64))
    assert np.array_equal(CR.box_mean(x, 1).view(np.uint32), x.view(np.uint32))  # r = 1 copies the bits


def test_tree_order_is_visible():
    """(2^60 + 1) + (-2^60 + 1): the pairwise tree loses both ones inside its
    pairs (0), a left-to-right float64 sum keeps the last (1)."""
    x = np.array([2.0 ** 60, 1.0, -(2.0 ** 60), 1.0], dtype=np.float32)
    tree = CR.tree_sum(x, 4)[0]
    left = 0.0
    for v in x.astype(np.float64):
        left += v
    assert tree == 0.0 and left == 1.0
    assert CR.box_mean(x, 4)[0] == 0.0
    # and a swap of two cells inside the run changes the tree's value
    y = x[[0, 2, 1, 3]]
    assert CR.tree_sum(y, 4)[0] == 2.0


def test_flux_accumulates_in_float64_in_substep_order():
    F = np.zeros((1, 4, 2), dtype=np.float32)
    F[0, :, 1] = [2.0 ** 60, 1.0, -(2.0 ** 60), 1.0]  # the right face of the one coarse cell (r = 2)
    _, fc = CR.coarsen(np.zeros((1, 5, 3, 2), np.float32), F, 2, 4)
    assert fc.shape == (1, 1, 1) and fc[0, 0, 0] == np.float32(1.0 / 4.0)  # ((2^60 + 1) - 2^60) + 1 = 1 in float64
    _, fc3 = CR.coarsen(np.zeros((1, 4, 3, 2), np.float32), np.full((1, 3, 2), 0.1, np.float32), 2, 3)
    acc = np.float64(np.float32(0.1)) * 3  # exact in float64
    assert fc3[0, 0, 0] == np.float32(acc / 3.0)


@pytest.mark.parametrize("nx,r", [(16, 16), (64, 4), (4, 64), (32, 2), (64, 1)])
def test_coarse_cell_centres(nx, r):
    gc, gf = CR.grids(nx, r, 1)
    xc = CR.tree_sum(gf.x, r) / r  # float64 cells: the same tree
    assert np.allclose(xc, gc.x, rtol=0, atol=4 * np.finfo(np.float64).eps * gc.length)


# ------------------------------------------------------------------ the identity
@pytest.fixture(scope="module")
def identity_runs():
    return {case: CR.fine_reference(*case, CR.IDENTITY_TC, CR.IDENTITY_SEEDS) for case in CR.IDENTITY_CASES}


@pytest.mark.parametrize("case", CR.IDENTITY_CASES)
def test_coarse_continuity_identity(identity_runs, case):
    """|nbar' - (nbar - f32(dt/dx)(Fbar_j - Fbar_{j-1}))| <= (3 S + 4) 2^-24 (max|n| + 2 c_f max|F|);
    measured with the oracle: at most 0.23 of the bound over these cases."""
    nx, r, S = case
    R = identity_runs[case]
    assert np.isfinite(R["fine_traj"]).all()
    assert R["traj"].shape == (3, CR.IDENTITY_TC + 1, 3, nx) and R["flux"].shape == (3, CR.IDENTITY_TC, nx)
    res = CR.continuity_residual(R["traj"], R["flux"], R["coarse"])
    bound = CR.continuity_bound(R["fine_traj"], R["fine_flux"], R["fine"], S)
    print(f"case {case}: residual {res:.3e} = {res / bound:.3f} of the bound {bound:.3e}")
    assert res <= bound


def test_E_solve_is_the_coarse_poisson_of_nbar():
    a = CR.fine_reference(16, 4, 2, 2, (0, 1), E="solve")
    b = CR.fine_reference(16, 4, 2, 2, (0, 1), E="filtered")
    assert np.array_equal(a["traj"][..., :2, :], b["traj"][..., :2, :])
    assert np.array_equal(a["traj"][..., 2, :], O.solve_poisson(a["coarse"], b["traj"][..., 0, :]))
    d = np.abs(a["traj"][..., 2, :] - b["traj"][..., 2, :]).max()
    assert 0 < d < 0.1  # the filtered fine E is another field (aliasing of the modes above the coarse Nyquist)


# ------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def L():
    from hybridflux import _lib
    return _lib.lib()


def test_declared_exported_and_bound(L):
    from hybridflux import _lib
    header = open(os.path.join(ROOT, "include", "hybridflux.h")).read()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(L, n), n
        assert re.search(rf"\b{n}\s*\(", header), f"{n} is not declared in include/hybridflux.h"


def test_size_query(L):
    q = L.hf_run_coarse_workspace_bytes
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    B, nx, T, r, S = 3, 96, 4, 2, 3
    assert q(B, nx, T, r, S) == up(12 * B * nx) + up(12 * B * nx * (T * S + 1)) + up(4 * B * nx * T * S)
    assert q(B, nx, 1, r, S) < q(B, nx, 2, r, S) < q(B, nx, T, r, S)
    assert q(B, nx, 0, r, S) == 0 and q(0, nx, T, r, S) == 0
    for fused in (16, 48, 64, 256, 512, 1024):
        assert q(B, fused, T, 2, S) == 0
    assert q(B, 128, T, 2, S) > 0 and q(B, 2048, T, 2, S) > 0
    assert q(32768, 2048, 100000, 64, 16) > 0
    for bad in ((-1, nx, T, r, S), (B, 0, T, r, S), (B, nx, -1, r, S), (B, nx, T, 0, S), (B, nx, T, 3, S),
                (B, nx, T, 128, S), (B, nx, T, 64, S), (B, nx, T, r, 0), (B, nx, T, r, -2),
                (B, nx, 2 ** 31 - 1, r, 2), (2 ** 31 - 1, nx, 1, 32, 2 ** 31 - 1)):
        assert q(*bad) == -1, bad


def _run(L, nx=128, B=3, T=4, r=2, S=3, pm=0, st=64, fin=128, plan=192, traj=256, flux=320, ws=512, wb=None):
    p = lambda v: c_void_p(v) if v else None  # noqa: E731  (dummy device addresses, never dereferenced)
    if wb is None:
        wb = max(int(L.hf_run_coarse_workspace_bytes(B, nx, T, r, S)), 0)
    return L.hf_run_coarse(p(st), p(fin), p(plan), pm, B, nx, T, r, S, 0.05, 5e-3, 1e-3, 0.01, p(traj), p(flux), p(ws),
                           wb, None)


@pytest.mark.parametrize("nx", [128, 64, 256])
def test_run_coarse_validation(L, nx):
    from hybridflux import _lib
    for kw in (dict(r=0), dict(r=3), dict(r=-2), dict(r=128), dict(S=0), dict(S=-1), dict(T=-1), dict(B=-1),
               dict(fin=0, traj=0, flux=0), dict(st=0), dict(plan=0), dict(pm=7)):
        assert _run(L, nx=nx, **kw) == _lib.HF_EINVAL, kw
        assert b"hf_run_coarse" in L.hf_last_error()
    assert _run(L, nx=96, r=64) == _lib.HF_EINVAL  # r does not divide nx_f
    assert _run(L, nx=nx, B=0, st=0) == _lib.HF_OK


def test_run_coarse_workspace_too_small(L):
    from hybridflux import _lib
    one = int(L.hf_run_coarse_workspace_bytes(3, 128, 1, 2, 3))
    assert _run(L, wb=one - 1) == _lib.HF_EINVAL and b"workspace" in L.hf_last_error()
    assert _run(L, wb=0) == _lib.HF_EINVAL


def test_coarsen_traj_validation(L):
    from hybridflux import _lib
    p = c_void_p
    ok = dict(tf=p(64), ff=p(128), B=3, nx=128, T=6, r=2, S=3, tc=p(192), fc=p(256))

    def call(**kw):
        a = dict(ok, **kw)
        return L.hf_coarsen_traj(a["tf"], a["ff"], a["B"], a["nx"], a["T"], a["r"], a["S"], a["tc"], a["fc"], None)

    for kw in (dict(r=0), dict(r=3), dict(r=128), dict(S=0), dict(T=-1), dict(T=7), dict(B=-1), dict(nx=0),
               dict(nx=97), dict(ff=None), dict(fc=None), dict(tf=None), dict(tc=None)):
        assert call(**kw) == _lib.HF_EINVAL, kw
        assert b"hf_coarsen_traj" in L.hf_last_error()
    assert call(B=0, tf=None, tc=None) == _lib.HF_OK


def test_valid_calls_reach_the_device(L):
    """Valid arguments pass validation; without a device the first device call fails (HF_EHIP)."""
    from hybridflux import _lib
    if L.hf_device_count() > 0:  # the dummy pointers would be dereferenced
        return
    for nx in (128, 96, 64, 48, 256, 1024):
        assert _run(L, nx=nx) == _lib.HF_EHIP, nx
        assert _run(L, nx=nx, T=0) == _lib.HF_EHIP, nx
    assert _run(L, wb=int(L.hf_run_coarse_workspace_bytes(3, 128, 1, 2, 3))) == _lib.HF_EHIP
    assert _run(L, pm=1) == _lib.HF_EHIP
    assert L.hf_coarsen_traj(c_void_p(64), None, 3, 128, 6, 2, 3, c_void_p(192), None, None) == _lib.HF_EHIP


# ------------------------------------------------------------------ the Python layer
class _Calls:
    """Host stand-ins for the engine entry points a default datagen call may and may not reach."""

    def __init__(self, monkeypatch):
        from hybridflux import engine
        from hybridflux.baseline_solver import BaselineSolver
        self.run = []

        def fake_run(model, grid, state0, T, traj=True, flux=False, metrics=False, out=None, ws=None):
            self.run.append((model, grid.nx, grid.dt, tuple(state0.shape), T, bool(traj), bool(flux)))
            B = state0.shape[0]
            return {"final": state0, "traj": torch.zeros(B, T + 1, 3, grid.nx) if traj else None,
                    "flux": torch.ones(B, T, grid.nx) if flux else None, "metrics": None}

        def refuse(*a, **k):
            raise AssertionError("refine = substeps = 1 must not reach the coarse-graining entry points")

        monkeypatch.setattr(engine, "run", fake_run)
        for name in ("run_coarse", "coarsen_traj", "poisson_traj"):
            monkeypatch.setattr(engine, name, refuse)
        monkeypatch.setattr(BaselineSolver, "initial_conditions",
                            lambda self, seeds, as_tensor=False, device_rng=False: torch.zeros(len(list(seeds)), 3, self.nx))
        monkeypatch.setattr(BaselineSolver, "_upload", lambda self, s: s)


def test_datagen_defaults_take_the_old_path(monkeypatch):
    from hybridflux import datagen
    c = _Calls(monkeypatch)
    st, ft, sn, x, dt, dx, nu = datagen.generate_dataset(nx=16, num_initial_conditions=2, steps_per_ic=3, out_path=None)
    assert c.run == [(None, 16, 5e-3, (2, 3, 16), 3, True, True)]
    assert st.shape == (6, 3, 16) and ft.shape == (6, 16) and sn.shape == (6, 3, 16) and x.shape == (16,)
    tr = datagen.generate_trajectories(nx=16, num_initial_conditions=2, steps_per_ic=3, refine=1, substeps=1)
    assert tr.shape == (2, 4, 3, 16) and len(c.run) == 2 and c.run[1][-2:] == (True, False)


def test_fine_reference_identity_takes_the_old_path(monkeypatch):
    from hybridflux import FineReference
    c = _Calls(monkeypatch)
    ref = FineReference(nx=16, refine=1, substeps=1)
    assert ref.identity and ref.fine.nx == 16 and ref.fine.dt == ref.coarse.dt
    s0 = ref.initial_conditions(range(2))
    r = ref.run_batch(s0, 3, traj=True, flux=True, final=True)
    assert c.run == [(None, 16, 5e-3, (2, 3, 16), 3, True, True)]
    assert r["traj"].shape == (2, 4, 3, 16) and r["flux"].shape == (2, 3, 16) and r["final_fine"] is s0
    assert ref.restrict(s0) is s0


def test_fine_reference_grids_and_arguments(capsys):
    from hybridflux import FineReference
    ref = FineReference(nx=64, refine=16, substeps=4, dt=2e-2)
    assert capsys.readouterr().out == ""  # dt_f / dx_f = 0.81: the fine grid's warning is not printed
    assert ref.fine.nx == 1024 and ref.fine.dt == 5e-3 and ref.coarse.nx == 64 and ref.coarse.dt == 2e-2
    assert np.allclose(CR.tree_sum(ref.fine.x, 16) / 16, ref.coarse.x, rtol=0, atol=1e-14)
    for kw in (dict(refine=3), dict(refine=0), dict(refine=128), dict(substeps=0), dict(E="box")):
        with pytest.raises(ValueError):
            FineReference(nx=16, **kw)


def test_first_nonfinite():
    from hybridflux.fine_reference import first_nonfinite
    t = torch.zeros(3, 5, 3, 4)
    assert first_nonfinite(t) is None
    t[2, 4, 1, 3] = float("nan")
    t[1, 3, 0, 0] = float("inf")
    t[0, 4, 2, 2] = float("nan")
    assert first_nonfinite(t) == (1, 3)


def test_datagen_refuses_a_nonfinite_fine_reference(monkeypatch):
    """nx_f = 1024 at nu = 1e-3 blows up within 32 coarse steps for seeds 2 and 3 (the oracle's
    rollout stands in for the device's): the generators name the first IC and
    coarse step instead of returning NaNs."""
    from hybridflux import datagen
    seeds, steps = [2, 3], 32
    with np.errstate(all="ignore"):
        R = CR.fine_reference(64, 16, 16, steps, seeds, E="filtered")
    bad = ~np.isfinite(R["traj"]).all(axis=(2, 3))  # [B, T+1]
    assert bad.any() and not bad[:, :10].any()
    step = int(np.argmax(bad.any(axis=0)))
    ic = int(np.argmax(bad[:, step]))

    class Fake:
        def __init__(self, **kw):
            assert kw["nx"] == 64 and kw["refine"] == 16 and kw["substeps"] == 16

        def initial_conditions(self, s, device_rng=False):
            return None

        def run_batch(self, s0, n, traj=True, flux=False, final=False):
            return {"traj": torch.from_numpy(R["traj"]), "flux": torch.from_numpy(R["flux"]), "final_fine": None}

    monkeypatch.setattr(datagen, "FineReference", Fake)
    for gen in (datagen.generate_trajectories, lambda **kw: datagen.generate_dataset(out_path=None, **kw)):
        with pytest.raises(ValueError, match=rf"IC {ic} \(seed {seeds[ic]}\), coarse step {step}\b"):
            gen(nx=64, seeds=seeds, steps_per_ic=steps, refine=16, substeps=16)
