"""The initial-condition draw protocol, without a GPU: the replay of
tests/ic_cases.py equals today's host code (BaselineSolver._modes) bit for bit,
the library's host entry point hf_ic_draws_host (the same __host__ __device__
draw code the kernel runs, csrc/initial_conditions.hip) equals numpy's draws
exactly, the case table takes every path it is meant to, and bad seeds and bad
arguments are refused before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import ic_cases as C
from conftest import ROOT
from hybridflux import BaselineSolver, _lib, engine


def P(v):
    return ctypes.c_void_p(v)


@pytest.fixture(scope="module")
def solvers():
    return {nx: BaselineSolver(nx=nx) for nx in C.NXS}


@pytest.fixture(scope="module")
def replays():
    return {c: C.replay(*c) for c in set(C.CASES)}


def host_draws(seed, nx):
    t, g = np.full(C.TABLE_LEN, np.nan), np.full(nx, np.nan)
    _lib.check(_lib.lib().hf_ic_draws_host(seed, nx, _lib.ptr(t), _lib.ptr(g)))
    return t, g


def test_declared_exported_and_built():
    with open(os.path.join(ROOT, "include", "hybridflux.h")) as f:
        header = f.read()
    L = _lib.lib()
    for n in ("hf_initial_conditions", "hf_ic_draws_host"):
        assert re.search(r"\b" + n + r"\(", header), n
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    assert int(re.search(r"#define HF_IC_TABLE_LEN (\d+)", header).group(1)) == _lib.HF_IC_TABLE_LEN == C.TABLE_LEN
    with open(os.path.join(ROOT, "gnn-plasma-flux_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS :=.*\binitial_conditions\.hip\b", mk, re.M)
    assert "-ffp-contract=off" in re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1)


def test_replay_equals_host_modes_bitwise(solvers, replays):
    """The table is valid: the replay reproduces _modes in n and u, bit for bit."""
    for (seed, nx), r in replays.items():
        n, u = C.fields(r["table"], r["gauss"], solvers[nx].x)
        n_ref, u_ref = solvers[nx]._modes(seed)
        assert n.dtype == n_ref.dtype == np.float32
        assert (n.view(np.uint32) == n_ref.view(np.uint32)).all(), (seed, nx)
        assert (u.view(np.uint32) == u_ref.view(np.uint32)).all(), (seed, nx)


def test_replay_equals_numpy_draws(replays):
    """Mode draws and gauss equal numpy's exactly, and the replay stops where
    numpy does: the words numpy draws next are the stream's next."""
    for (seed, nx), r in replays.items():
        t, g, nxt = C.numpy_draws(seed, nx)
        assert (r["table"][:-1] == t[:-1]).all(), (seed, nx)
        assert (r["gauss"].astype(np.float32).view(np.uint32) == g.astype(np.float32).view(np.uint32)).all()
        w = C.stream(seed, r["words"] + 4)
        assert (w[r["words"]:] == nxt).all(), (seed, nx)


def test_host_entry_point_equals_numpy(replays):
    """hf_ic_draws_host: mode count, km, amp, ph and words consumed exactly;
    float32(gauss) bit for bit against RandomState's randn(nx) after the mode draws."""
    for (seed, nx), r in replays.items():
        t, g = host_draws(seed, nx)
        want, g_np, _ = C.numpy_draws(seed, nx)
        want[-1] = r["words"]
        assert (t == want).all(), (seed, nx, t, want)
        assert (g.astype(np.float32).view(np.uint32) == g_np.astype(np.float32).view(np.uint32)).all(), (seed, nx)
        assert (C.expected_table(seed, nx) == want).all()


def test_case_table_is_sharp(replays):
    """Computed from the replay: rejected randint tries, rejected gauss attempts,
    a case inside one 624-word block, cases that cross one block boundary,
    cases that cross at least four; odd nx; a repeated seed."""
    rs = replays
    assert sum(r["randint_rejects"] > 0 for r in rs.values()) >= 10
    assert sum(r["gauss_rejects"] > 0 for r in rs.values()) >= 10
    blocks = {c: (r["words"] - 1) // C.BLOCK for c, r in rs.items()}      # boundaries crossed
    assert all(blocks[s, 64] == 0 for s in C.SEEDS)
    for nx in (250, 256):
        assert sum(blocks[s, nx] == 1 for s in C.SEEDS) > len(C.SEEDS) // 2
    assert all(blocks[s, 1024] >= 4 for s in C.SEEDS)
    # a gauss attempt that straddles a block boundary (its four words in two blocks)
    assert any((C.BLOCK - r["mode_words"]) % 4 != 0 and r["words"] > C.BLOCK for r in rs.values())
    assert any(nx % 2 for nx in C.NXS) and len(set(C.SEEDS)) < len(C.SEEDS)
    assert {0, 1, 42, 2 ** 32 - 1} <= set(C.SEEDS) and set(range(1000, 1016)) <= set(C.SEEDS)
    assert {3, 4, 5} == {int(r["table"][0]) for r in rs.values()}


def test_seed_validation():
    for bad in ([-1], [2 ** 32], [5, 2 ** 40], np.array([-3]), range(-1, 2), [2 ** 70]):
        with pytest.raises(ValueError, match=r"Seed must be between 0 and 2\*\*32 - 1"):
            engine.ic_seeds(bad)
    for bad in (None, [None], [3, None]):
        with pytest.raises(ValueError, match="seed=None"):
            engine.ic_seeds(bad)
    with pytest.raises(TypeError):
        engine.ic_seeds([1.5])
    with pytest.raises(TypeError):
        engine.ic_seeds(np.array([1.0]))
    import torch
    for ok in (range(3), [0, 1, 2], np.arange(3, dtype=np.uint32), torch.arange(3)):
        s = engine.ic_seeds(ok)
        assert s.dtype == np.int64 and s.tolist() == [0, 1, 2]
    assert engine.ic_seeds([2 ** 32 - 1, 0]).tolist() == [2 ** 32 - 1, 0]
    assert engine.ic_seeds(np.array([2 ** 32 - 1], dtype=np.uint64)).tolist() == [2 ** 32 - 1]
    assert engine.ic_seeds([]).shape == (0,)
    # through the public surface: refused on the host, before any device work
    b = BaselineSolver(nx=16)
    with pytest.raises(ValueError, match="Seed must be between"):
        b.initial_conditions([1, -1], device_rng=True)
    with pytest.raises(ValueError, match="seed=None"):
        b.initial_condition(device_rng=True)
    with pytest.raises(ValueError, match="Seed must be between"):
        from hybridflux import datagen
        datagen.generate_trajectories(nx=16, seeds=[2 ** 32], device_rng=True)


def test_entry_points_validate_before_device():
    L = _lib.lib()
    d = P(256)
    fn = b"hf_initial_conditions"
    for B, nx in ((-1, 64), (3, 0), (3, -5), (-2 ** 31, -2 ** 31)):
        assert L.hf_initial_conditions(d, B, nx, d, d, None, None) == _lib.HF_EINVAL and fn in L.hf_last_error()
    assert L.hf_initial_conditions(d, 3, 2 ** 24 + 1, d, d, None, None) == _lib.HF_EUNSUPPORTED
    for args in ((None, 3, 64, d, d), (d, 3, 64, None, d), (d, 3, 64, d, None)):
        assert L.hf_initial_conditions(*args, None, None) == _lib.HF_EINVAL and b"NULL" in L.hf_last_error()
    assert L.hf_initial_conditions(None, 0, 64, None, None, None, None) == _lib.HF_OK      # an empty batch
    t, g = np.zeros(C.TABLE_LEN), np.zeros(4)
    fn = b"hf_ic_draws_host"
    for seed in (-1, 2 ** 32, -2 ** 63):
        assert L.hf_ic_draws_host(seed, 4, _lib.ptr(t), _lib.ptr(g)) == _lib.HF_EINVAL
        assert fn in L.hf_last_error() and b"Seed must be between 0 and 2**32 - 1" in L.hf_last_error()
    assert L.hf_ic_draws_host(1, 0, _lib.ptr(t), _lib.ptr(g)) == _lib.HF_EINVAL
    assert L.hf_ic_draws_host(1, 2 ** 24 + 1, _lib.ptr(t), _lib.ptr(g)) == _lib.HF_EUNSUPPORTED
    assert L.hf_ic_draws_host(1, 4, None, _lib.ptr(g)) == _lib.HF_EINVAL
    assert L.hf_ic_draws_host(1, 4, _lib.ptr(t), None) == _lib.HF_EINVAL and fn in L.hf_last_error()
    if L.hf_device_count() <= 0:   # valid arguments: validation passes and the launch itself fails
        assert L.hf_initial_conditions(d, 3, 64, d, d, None, None) == _lib.HF_EHIP


def test_defaults_stay_host():
    """device_rng defaults to False everywhere (the host loop, bit for bit)."""
    import inspect
    from hybridflux import datagen
    for f in (BaselineSolver.initial_condition, BaselineSolver.initial_conditions, datagen.generate_dataset,
              datagen.generate_trajectories):
        assert inspect.signature(f).parameters["device_rng"].default is False
