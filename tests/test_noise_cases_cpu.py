"""The state noise of training, without a GPU: the library's host entry point
hf_gauss_host (the __host__ __device__ draw code the kernel runs,
csrc/initial_conditions.hip) equals numpy's standard_normal bit for bit, the
restatement of tests/noise_cases.py tells three wrong restatements from the
right one, hf_state_noise refuses every bad argument before any device call
with a message that names it, and the header, the exports and the ctypes table
agree."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import noise_cases as N
from conftest import ROOT
from hybridflux import _lib, engine, training


def P(v):
    return ctypes.c_void_p(v)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_declared_exported_and_built():
    with open(os.path.join(ROOT, "include", "hybridflux.h")) as f:
        header = f.read()
    L = _lib.lib()
    for n in ("hf_state_noise", "hf_gauss_host"):
        assert re.search(r"\b" + n + r"\(", header), n
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    assert int(re.search(r"#define HF_NOISE_ZERO_MEAN (\d+)", header).group(1)) == _lib.HF_NOISE_ZERO_MEAN == 1
    # the declaration's argument count is the ctypes table's
    decl = re.search(r"int hf_state_noise\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["hf_state_noise"][1]) == 13
    assert _lib.SIGNATURES["hf_gauss_host"] == (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p])
    with open(os.path.join(ROOT, "gnn-plasma-flux_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^ASAN_PROGS :=.*\bnoise\b", mk, re.M) and re.search(r"^asan-noise:", mk, re.M)
    assert os.path.exists(os.path.join(ROOT, "tests", "native", "noise_sanitize.cpp"))


def test_gauss_host_equals_numpy_bitwise():
    """standard_normal(count) in float64, every bit, for odd and even counts, one
    624-word block and many."""
    L = _lib.lib()
    for seed in sorted(set(N.SEEDS)):
        for count in N.COUNTS:
            g = np.full(count + 1, -7.0)
            _lib.check(L.hf_gauss_host(seed, count, _lib.ptr(g)))
            want = np.random.RandomState(seed).standard_normal(count)
            assert (bits64(g[:count]) == bits64(want)).all(), (seed, count)
            assert g[count] == -7.0                      # nothing past count
    assert L.hf_gauss_host(5, 0, None) == _lib.HF_OK
    for seed, count in ((-1, 4), (2 ** 32, 4), (-2 ** 63, 4), (1, -1), (1, -2 ** 63)):
        assert L.hf_gauss_host(seed, count, _lib.ptr(np.zeros(4))) == -1 and b"hf_gauss_host" in L.hf_last_error()
    assert L.hf_gauss_host(1, 4, None) == _lib.HF_EINVAL and b"NULL" in L.hf_last_error()


def test_polar_replay_equals_numpy():
    """The word-by-word statement of the protocol is numpy's (so its mutant is a
    mutant of numpy's protocol)."""
    for seed in (0, 42, 2 ** 32 - 1, 1007):
        for count in (1, 2, 3, 51, 750):
            assert (bits64(N.polar(seed, count)) == bits64(N.gauss(seed, count))).all(), (seed, count)


@pytest.mark.parametrize("nx", [16, 17, 250])
def test_restatement_is_sharp(nx):
    """Each mutant changes more than half of the values it should touch: the
    rows with noise for the swap and the block order, the n row for the mean."""
    sigma, st = (1e-2, 1e-2, 5e-3), N.states(nx)
    for k, seed in enumerate(N.SEEDS[:6]):
        right = N.reference(seed, nx, sigma, True, st[k])
        again = N.reference(seed, nx, sigma, True, st[k])
        assert (right["out"].view(np.uint32) == again["out"].view(np.uint32)).all()
        for mutant, rows in (("swap_x1_x2", slice(0, 3)), ("no_zero_mean", slice(0, 1)), ("blocks_u_n_E", slice(0, 2))):
            wrong = N.reference(seed, nx, sigma, True, st[k], mutant=mutant)
            for key in ("out", "noise"):
                a, b = right[key][rows].view(np.uint32), wrong[key][rows].view(np.uint32)
                assert (a != b).sum() > a.size // 2, (seed, nx, mutant, key)


def test_restatement_details():
    nx, seed = 17, 42
    st = N.states(nx)[0]
    r = N.reference(seed, nx, (0.0, 3e-3, 0.0), True, st)
    assert (r["out"][0].view(np.uint32) == st[0].view(np.uint32)).all() and (r["noise"][[0, 2]] == 0).all()
    g = N.gauss(seed, 3 * nx)
    assert (r["noise"][1] == np.float32(3e-3) * g[nx:2 * nx].astype(np.float32)).all()
    z = N.reference(seed, nx, (1e-2, 0.0, 0.0), True, st)
    assert abs(z["d"][0].sum()) < 1e-13 and abs(N.reference(seed, nx, (1e-2, 0, 0), False, st)["d"][0].sum()) > 1e-3
    # the fixed-order sum is a sum: within rounding of math.fsum
    import math
    for n in (1, 63, 64, 65, 250, 1024):
        v = N.gauss(7, n)
        assert abs(N.fixed_order_sum(v) - math.fsum(v)) <= 1e-13 * max(1.0, np.abs(v).sum())
    # a plan recomputes E from n' and adds no noise there
    from hybridflux import BaselineSolver
    pc = BaselineSolver(nx=nx).grid.poisson_c
    p = N.reference(seed, nx, (1e-2, 1e-2, 0.0), True, st, plan=pc)
    assert (p["noise"][2] == 0).all() and (p["out"][:2] == N.reference(seed, nx, (1e-2, 1e-2, 0), True, st)["out"][:2]).all()
    assert abs(p["out"][2].astype(np.float64).sum()) < 1e-5


def test_case_table():
    assert N.NXS == (16, 17, 64, 250, 256, 1024) and len(N.CASES) == 36
    assert any((3 * nx) % 2 for nx in N.NXS)
    assert 4 * (3 * 250 // 2) > 2 * 624          # several 624-word blocks from nx = 250 on
    assert set(N.SIGMAS) == {(1e-2, 1e-2, 0.0), (0.0, 3e-3, 0.0), (1e-2, 0.0, 5e-3)}


def test_state_noise_validates_before_device():
    L = _lib.lib()
    d = P(256)
    sig = np.array([1e-2, 1e-2, 0.0], dtype=np.float32)
    ZM = _lib.HF_NOISE_ZERO_MEAN

    def call(seeds=d, B=3, nx=64, sigma=sig, flags=ZM, sin=d, sout=d, plan=None, pm=0, x=None, nf=None, noise=None):
        return L.hf_state_noise(seeds, B, nx, _lib.ptr(sigma), flags, sin, sout, plan, pm, x, nf, noise, None)

    def refused(code, word, **kw):
        assert call(**kw) == code, kw
        msg = L.hf_last_error()
        assert b"hf_state_noise" in msg and word in msg, (kw, msg)

    for kw in (dict(B=-1), dict(nx=0), dict(nx=-5), dict(B=-2 ** 31, nx=-2 ** 31)):
        refused(_lib.HF_EINVAL, b"shape", **kw)
    for kw in (dict(seeds=None), dict(sin=None), dict(sout=None), dict(sigma=None)):
        refused(_lib.HF_EINVAL, b"NULL", **kw)
    for bad in ([-1e-2, 0, 0], [0, -1.0, 0], [0, 0, -1e-30], [np.nan, 0, 0], [0, 0, np.nan], [-np.inf, 0, 0]):
        refused(_lib.HF_EINVAL, b"sigma", sigma=np.array(bad, dtype=np.float32))
    for flags in (2, 3, -1, 1 << 30):
        refused(_lib.HF_EINVAL, b"flags", flags=flags)
    for pm in (2, -1, 99):
        refused(_lib.HF_EINVAL, b"Poisson mode", plan=d, pm=pm)
    refused(_lib.HF_EINVAL, b"sigma[2]", plan=d, sigma=np.array([1e-2, 0, 5e-3], dtype=np.float32))
    refused(_lib.HF_EINVAL, b"dev_x", nf=d)
    refused(_lib.HF_EUNSUPPORTED, b"2^24", nx=2 ** 24 + 1, flags=0)
    refused(_lib.HF_EUNSUPPORTED, b"6144", nx=6145)
    refused(_lib.HF_EUNSUPPORTED, b"16384", nx=16385, flags=0, plan=d, pm=_lib.HF_POISSON_TRIDIAG)
    assert call(seeds=None, B=0, sin=None, sout=None) == _lib.HF_OK          # an empty batch: no launch
    assert call(seeds=None, B=0, sin=None, sout=None, sigma=None) == _lib.HF_EINVAL
    if L.hf_device_count() <= 0:   # valid arguments: validation passes and the launch itself fails
        assert call() == _lib.HF_EHIP
        assert call(nx=6145, flags=0) == _lib.HF_EHIP


def test_python_surface_without_device():
    with pytest.raises(ValueError, match="sigma"):
        training.StateNoise(-1e-2, 0.0)
    with pytest.raises(ValueError, match="sigma"):
        engine.noise_sigma((1e-2, float("nan"), 0))
    with pytest.raises(ValueError, match="sigma"):
        engine.noise_sigma((1e-2, 1e-2))
    from hybridflux import BaselineSolver, StateNoise
    assert StateNoise is training.StateNoise
    grid = BaselineSolver(nx=16).grid
    with pytest.raises(ValueError, match="sigma_E must be 0"):
        training.StateNoise(1e-2, 1e-2, 5e-3, grid=grid)
    with pytest.raises(ValueError, match="sigma_E must be 0"):
        training.StateNoise(1e-2, 1e-2, 5e-3).with_grid(grid)
    n = training.StateNoise(1e-2, 3e-3, zero_mean=False).with_grid(grid)
    assert n.grid is grid and n.zero_mean is False and n.sigma.dtype == np.float32
    assert n.sigma.tolist() == [float(np.float32(1e-2)), float(np.float32(3e-3)), 0.0]
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.state_noise(np.zeros((2, 3, 16), np.float32), [1, 2], (1e-2, 1e-2, 0))
    # noise=None is the default everywhere, so every existing call is what it was
    for f in (training.train_unrolled, training.train_pure_gnn_unrolled, training.train_pinn_unrolled,
              training._train_windows, training.WindowDataset.batch, training.FluxDataset.batch):
        p = inspect.signature(f).parameters
        assert p["noise"].default is None
        assert ("noise_seed" in p and p["noise_seed"].default == 0) or p["seeds"].default is None
    d = training.WindowDataset(np.zeros((2, 4, 3, 16), np.float32), 2, device="cpu")
    with pytest.raises(ValueError, match="needs seeds"):
        d.batch([0], noise=training.StateNoise(1e-2, 1e-2))
    with pytest.raises(ValueError, match="without noise"):
        d.batch([0], seeds=[1])
