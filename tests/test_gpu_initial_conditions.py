"""Initial conditions drawn on the MI355X (hf_initial_conditions,
csrc/initial_conditions.hip) against numpy's RandomState and today's host path
(BaselineSolver.initial_conditions without device_rng) of the same process.

The draw table (mode count, km, amp, ph, words consumed) passes through no
sin, cos or log, so it must equal numpy's exactly.  n and u do: the device's
float64 sin, cos and log are not the host's, so bit equality is expected but
not guaranteed.  The gate has two conditions:
  every value within 5e-7 absolute (two float32 ulps at |n| < 4 are 4.8e-7;
  terms are <= 0.3), and
  at most 1e-4 of the compared values not bit-equal.
The second is a condition, not a measurement: perturbing every float64 sin,
cos and log result by +-1 ulp changes none of 262,144 float32 values on the
host, and a real defect changes nearly all of them.  The observed counts are
recorded (conftest.record; profiles/initial_conditions_parity.json).
"""
import numpy as np
import pytest
import torch

import ic_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 5e-7
UNEQUAL_FRACTION = 1e-4


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


@pytest.fixture(scope="module")
def solvers(hf):
    class Solvers(dict):     # one BaselineSolver per nx, built when first asked for
        def __missing__(self, nx):
            self[nx] = hf.BaselineSolver(nx=nx, device=DEV)
            return self[nx]
    return Solvers()


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gate(dev, host, record, name, what):
    """The two-condition gate on rows n and u; returns the per-IC bit equality."""
    d, h = dev[:, :2], host[:, :2]
    assert np.isfinite(d).all()
    err = float(np.abs(d.astype(np.float64) - h).max())
    unequal = int((bits(d) != bits(h)).sum())
    record(name, f"{what}_max_abs", err)
    record(name, f"{what}_values", d.size)
    record(name, f"{what}_not_bit_equal", unequal)
    print(f"{name} {what}: max |dev - host| = {err:.3e}, {unequal} of {d.size} values not bit-equal")
    assert err <= ATOL, f"{what}: max |dev - host| = {err:.3e}"
    assert unequal <= UNEQUAL_FRACTION * d.size, f"{what}: {unequal} of {d.size} values not bit-equal"
    return (bits(d) == bits(h)).reshape(d.shape[0], -1).all(axis=1)


@pytest.mark.parametrize("nx", C.NXS)
def test_draw_table_equals_numpy(hf, solvers, nx):
    """Mode count, (km, amp, ph) x 7 and the words consumed: exactly numpy's, for
    every case of the table (B = 21 per nx)."""
    from hybridflux import engine
    st, table = engine.initial_conditions(solvers[nx].grid, C.SEEDS, debug=True, device=DEV)
    table = table.cpu().numpy()
    assert table.shape == (len(C.SEEDS), C.TABLE_LEN) and st.shape == (len(C.SEEDS), 3, nx)
    for row, seed in zip(table, C.SEEDS):
        want = C.expected_table(seed, nx)
        assert (row == want).all(), (seed, nx, row, want)


def test_fields_against_host_path(hf, solvers, record):
    """n and u for seeds 1000..1511 at nx = 64 and for the table's cases."""
    name = "test_fields_against_host_path"
    seeds = list(range(1000, 1512))
    b = solvers[64]
    gate(b.initial_conditions(seeds, device_rng=True), b.initial_conditions(seeds), record, name, "nx64_seeds1000_1511")
    for nx in C.NXS:
        b = solvers[nx]
        gate(b.initial_conditions(C.SEEDS, device_rng=True), b.initial_conditions(C.SEEDS), record, name,
             f"table_nx{nx}")


def test_wide_case(hf, solvers, record):
    """nx = 4096, B = 4: about 11 k words per IC, many twists."""
    b = solvers[4096]
    seeds = [0, 42, 1000, 2 ** 32 - 1]
    gate(b.initial_conditions(seeds, device_rng=True), b.initial_conditions(seeds), record, "test_wide_case", "nx4096")


@pytest.mark.parametrize("nx", [17, 64, 1024])
def test_E_is_the_engines_poisson(hf, solvers, nx):
    from hybridflux import engine
    st = solvers[nx].initial_conditions(C.SEEDS, as_tensor=True, device_rng=True)
    assert st.is_cuda and st.dtype == torch.float32 and st.is_contiguous()
    E = engine.poisson(solvers[nx].grid, st[:, 0])
    assert (bits(st[:, 2]) == bits(E)).all()


@pytest.mark.parametrize("nx", [64, 250])
def test_batch_independence_bitwise(hf, solvers, nx):
    """Seed s gives the same rows alone, at any position, in batches of 1, 3, 65
    and 257, and when repeated inside a batch; two calls give the same bits."""
    b = solvers[nx]
    pool = list(range(3000, 3257))
    ref = bits(b.initial_conditions(pool, device_rng=True))
    assert (ref == bits(b.initial_conditions(pool, device_rng=True))).all()
    row = {s: ref[i] for i, s in enumerate(pool)}
    rng = np.random.default_rng(nx)
    for size in (1, 3, 65, 257):
        batch = [int(s) for s in rng.permutation(pool)[:size]]
        got = bits(b.initial_conditions(batch, device_rng=True))
        for i, s in enumerate(batch):
            assert (got[i] == row[s]).all(), (size, i, s)
    s = pool[7]
    batch = [s, pool[0], s, s] + pool[100:161] + [s]
    got = bits(b.initial_conditions(batch, device_rng=True))
    for i, t in enumerate(batch):
        assert (got[i] == row[t]).all(), (i, t)


def test_out_of_range_seed_gives_nan_not_garbage(hf, solvers):
    """The C ABI cannot validate device seeds on the host: the kernel writes NaN
    for a seed outside [0, 2^32) and leaves the others as they are."""
    from hybridflux import _lib, engine
    b = solvers[64]
    good = bits(b.initial_conditions([5, 7], device_rng=True))
    seeds = torch.tensor([5, -1, 2 ** 32, 7], dtype=torch.int64, device=DEV)
    st = torch.zeros(4, 3, 64, dtype=torch.float32, device=DEV)
    table = torch.zeros(4, C.TABLE_LEN, dtype=torch.float64, device=DEV)
    x = torch.as_tensor(b.grid.x, dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().hf_initial_conditions(_lib.ptr(seeds), 4, 64, _lib.ptr(x), _lib.ptr(st), _lib.ptr(table),
                                                engine.stream_of(torch.device(DEV))))
    st, table = st.cpu().numpy(), table.cpu().numpy()
    assert np.isnan(st[1:3, :2]).all() and (st[:, 2] == 0).all()       # row E is not this kernel's
    assert (table[1:3, 0] == -1).all() and (table[[0, 3], 0] >= 3).all()
    assert (bits(st[[0, 3], :2]) == good[:, :2]).all()


def test_public_surface(hf, solvers):
    """generate_trajectories(device_rng=True) equals the host-IC call wherever
    the ICs are bit-equal; initial_condition keeps the reference's shape and
    dtype; an empty seed list gives the empty state."""
    from hybridflux import datagen
    kw = dict(nx=64, num_initial_conditions=12, steps_per_ic=5, device=DEV)
    host = datagen.generate_trajectories(**kw)
    dev = datagen.generate_trajectories(device_rng=True, **kw)
    assert dev.shape == host.shape == (12, 6, 3, 64) and dev.dtype == np.float32
    same = (bits(dev[:, 0]) == bits(host[:, 0])).reshape(12, -1).all(axis=1)
    assert same.any(), "no IC is bit-equal to the host path's"
    assert (bits(dev[same]) == bits(host[same])).all()
    ds_h = datagen.generate_dataset(out_path=None, seeds=range(1000, 1004), steps_per_ic=3, device=DEV)
    ds_d = datagen.generate_dataset(out_path=None, seeds=range(1000, 1004), steps_per_ic=3, device=DEV, device_rng=True)
    assert ds_d[0].shape == ds_h[0].shape == (12, 3, 64)
    assert np.abs(ds_d[0][::3, :2] - ds_h[0][::3, :2]).max() <= ATOL      # the ICs: every third state_t row

    b = solvers[64]
    one = b.initial_condition(1234, device_rng=True)
    ref = b.initial_condition(1234)
    assert isinstance(one, np.ndarray) and one.shape == ref.shape == (3, 64) and one.dtype == ref.dtype == np.float32
    assert np.abs(one[:2] - ref[:2]).max() <= ATOL
    for seeds in (np.arange(1000, 1003), torch.arange(1000, 1003), range(1000, 1003)):
        got = b.initial_conditions(seeds, device_rng=True)
        assert (bits(got) == bits(b.initial_conditions([1000, 1001, 1002], device_rng=True))).all()
    empty = b.initial_conditions([], as_tensor=True, device_rng=True)
    assert empty.shape == (0, 3, 64) and empty.is_cuda and empty.dtype == torch.float32
    assert b.initial_conditions([], device_rng=True).shape == (0, 3, 64)
