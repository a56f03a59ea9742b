"""Seeded Gaussian state noise on the MI355X (hf_state_noise,
csrc/initial_conditions.hip) against the numpy restatement of
tests/noise_cases.py (numpy's own standard_normal draws).

The draws pass through the device's float64 log and sqrt, which are not the
host's, so bit equality with the restatement is expected but not guaranteed.
The gate has the two conditions of test_gpu_initial_conditions.py:
  every value within two float32 ulps of the case's largest |value| (computed
  from the restatement), and
  at most 1e-4 of the compared values not bit-equal.
The second is a condition, not a measurement: moving every float64 normal by
+-1 ulp on the host changed 0 of 268,800 float32 values, the zero-mean form
included, and a real defect changes nearly all of them.  The observed counts are
recorded (conftest.record).  Everything the entry point promises about its own
outputs (E from the engine's Poisson, node features, copies, in place, batch
independence, repeatability) is checked bit for bit.
"""
import numpy as np
import pytest
import torch

import noise_cases as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNEQUAL_FRACTION = 1e-4
B = len(N.SEEDS)


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


@pytest.fixture(scope="module")
def grids(hf):
    class Grids(dict):     # one grid per nx, built when first asked for
        def __missing__(self, nx):
            self[nx] = hf.BaselineSolver(nx=nx, device=DEV).grid
            return self[nx]
    return Grids()


@pytest.fixture(scope="module")
def start():
    class Start(dict):     # the start states per nx: (host, device), never written
        def __missing__(self, nx):
            h = N.states(nx)
            self[nx] = (h, torch.as_tensor(h, device=DEV))
            return self[nx]
    return Start()


_REF = {}


def reference(nx, sigma, zm):
    """The restatement for the table's seeds, computed once per case and shared."""
    key = (nx, sigma, zm)
    if key not in _REF:
        st = N.states(nx)
        rs = [N.reference(s, nx, sigma, zm, st[k]) for k, s in enumerate(N.SEEDS)]
        _REF[key] = {k: np.stack([r[k] for r in rs]) for k in ("out", "noise")}
    return _REF[key]


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gate(got, want, record, name, what):
    """The two-condition gate; the bound comes from the restatement's values."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and np.isfinite(got).all()
    atol = 2.0 * float(np.spacing(np.abs(want).max().astype(np.float32)))
    err = float(np.abs(got.astype(np.float64) - want).max())
    unequal = int((bits(got) != bits(want)).sum())
    record(name, f"{what}_max_abs", err)
    record(name, f"{what}_two_ulps", atol)
    record(name, f"{what}_values", got.size)
    record(name, f"{what}_not_bit_equal", unequal)
    print(f"{name} {what}: max |dev - ref| = {err:.3e} (2 ulps = {atol:.3e}), {unequal} of {got.size} not bit-equal")
    assert err <= atol, f"{what}: max |dev - ref| = {err:.3e} > {atol:.3e}"
    assert unequal <= UNEQUAL_FRACTION * got.size, f"{what}: {unequal} of {got.size} values not bit-equal"


def case_id(c):
    nx, sigma, zm = c
    return f"nx{nx}-s{N.SIGMAS.index(sigma)}-{'zm' if zm else 'raw'}"


@pytest.mark.parametrize("case", N.CASES, ids=case_id)
def test_against_restatement(hf, start, record, request, case):
    """n', u' (and E' where sigma_E > 0) and the added values, B = 21 per case."""
    from hybridflux import engine
    nx, sigma, zm = case
    ref = reference(*case)
    out, noise = engine.state_noise(start[nx][1], N.SEEDS, sigma, zero_mean=zm, return_noise=True)
    name = request.node.name
    rows = 3 if sigma[2] > 0 else 2
    gate(out[:, :rows], ref["out"][:, :rows], record, name, "state")
    gate(noise, ref["noise"], record, name, "noise")
    if sigma[2] == 0:
        assert (bits(out[:, 2]) == bits(start[nx][0][:, 2])).all()
    assert (bits(start[nx][1]) == bits(start[nx][0])).all()          # the input is not written


@pytest.mark.parametrize("nx", N.NXS)
def test_plan_recomputes_E_and_features(hf, grids, start, nx):
    """With a grid: E' is the engine's Poisson of n' bit for bit, n' and u' are
    the call's without a grid, the node features are [n', u', E', x], and the
    noise output is 0 on the E row."""
    from hybridflux import engine
    grid, (_, st) = grids[nx], start[nx]
    x = grid.on(torch.device(DEV))[0]
    sigma = (1e-2, 1e-2, 0.0)
    out, nf, noise = engine.state_noise(st, N.SEEDS, sigma, grid=grid, x=x, return_noise=True)
    plain = engine.state_noise(st, N.SEEDS, sigma)
    assert (bits(out[:, :2]) == bits(plain[:, :2])).all()
    assert (bits(out[:, 2]) == bits(engine.poisson(grid, out[:, 0]))).all()
    assert not (bits(out[:, 2]) == bits(st[:, 2])).all()
    want = torch.cat([out.permute(0, 2, 1), x[None, :, None].expand(B, nx, 1)], dim=2).reshape(B * nx, 4)
    assert nf.shape == (B * nx, 4) and (bits(nf) == bits(want)).all()
    assert (noise[:, 2] == 0).all() and (noise[:, :2] != 0).any()
    # features without a grid: E is the input's
    out2, nf2 = engine.state_noise(st, N.SEEDS, (0.0, 3e-3, 0.0), x=x)
    want2 = torch.cat([out2.permute(0, 2, 1), x[None, :, None].expand(B, nx, 1)], dim=2).reshape(B * nx, 4)
    assert (bits(nf2) == bits(want2)).all() and (bits(out2[:, 2]) == bits(st[:, 2])).all()


@pytest.mark.parametrize("nx", [17, 64, 250])
def test_sigma_zero_copies_bits(hf, start, nx):
    """A channel with sigma = 0 is copied, not added to: -0.0 and NaN payloads
    survive, and its noise is 0."""
    from hybridflux import engine
    h = start[nx][0].copy()
    w = h.view(np.uint32)
    w[:, 1, 0] = 0x80000000          # -0.0
    w[:, 1, 1] = 0x7FC12345          # quiet NaN with a payload
    w[:, 1, 2] = 0xFFC00001
    w[:, 2, nx - 1] = 0x7FA00000     # signalling NaN
    w[:, 2, 3] = 0x00000001          # a denormal
    st = torch.as_tensor(h, device=DEV)
    out, noise = engine.state_noise(st, N.SEEDS, (1e-2, 0.0, 0.0), return_noise=True)
    assert (bits(out[:, 1:]) == w[:, 1:]).all()
    assert (noise[:, 1:] == 0).all() and not (bits(out[:, 0]) == w[:, 0]).all()
    out = engine.state_noise(st, N.SEEDS, (0.0, 0.0, 0.0))
    assert (bits(out) == w).all()


@pytest.mark.parametrize("nx", [17, 64, 1024])
@pytest.mark.parametrize("zm", [True, False])
def test_in_place_repeat_and_batch_independence(hf, grids, start, nx, zm):
    """An in-place call equals an out-of-place one; two calls give the same bits;
    a sample alone equals the same sample inside a permuted batch (seed 42 is in
    the table twice, on different states).  n' and u' are so by construction.
    E' at nx = 1024 is not: the FFT Poisson transforms samples 2k and 2k+1 as one
    complex row, so a sample's float64 path depends on its pair partner (none
    when alone), and the bits agree because the rounding to float32 absorbs the
    difference.  A flip there would be hf_poisson_ex's, not the noise kernel's."""
    from hybridflux import engine
    grid, (_, st) = grids[nx], start[nx]
    x = grid.on(torch.device(DEV))[0]
    sigma = (1e-2, 3e-3, 0.0)
    for kw in (dict(), dict(grid=grid, x=x)):
        ref = engine.state_noise(st, N.SEEDS, sigma, zero_mean=zm, return_noise=True, **kw)
        again = engine.state_noise(st, N.SEEDS, sigma, zero_mean=zm, return_noise=True, **kw)
        for a, b in zip(ref, again):
            assert (bits(a) == bits(b)).all()
        buf = st.clone()
        got = engine.state_noise(buf, N.SEEDS, sigma, zero_mean=zm, out=buf, return_noise=True, **kw)
        assert got[0] is buf
        for a, b in zip(ref, got):
            assert (bits(a) == bits(b)).all()
        perm = np.random.default_rng(nx).permutation(B)
        seeds = [N.SEEDS[i] for i in perm]
        shuffled = engine.state_noise(st[perm].contiguous(), seeds, sigma, zero_mean=zm, **kw)
        shuffled = shuffled[0] if kw else shuffled
        assert (bits(shuffled) == bits(ref[0])[perm]).all()
        for k in (0, 3, B - 1):
            alone = engine.state_noise(st[k:k + 1].contiguous(), [N.SEEDS[k]], sigma, zero_mean=zm, **kw)
            alone = alone[0] if kw else alone
            assert (bits(alone)[0] == bits(ref[0])[k]).all(), k


@pytest.mark.parametrize("nx", N.NXS)
def test_zero_mean_keeps_charge(hf, start, nx):
    """|mean(n') - mean(n)| <= 2^-23 (max|n'| + sigma_n max|d|): d sums to 0 up
    to float64 rounding, so what is left is the float32 rounding of each product
    (half an ulp of sigma_n |d|) and of each sum (half an ulp of |n'|), and the
    mean of the errors is at most their largest.  Without zero mean the shift is
    the noise's own mean, far above the bound for most samples."""
    from hybridflux import engine
    sn = 1e-2
    h, st = start[nx]
    out, noise = engine.state_noise(st, N.SEEDS, (sn, 0.0, 0.0), zero_mean=True, return_noise=True)
    o, a = out.cpu().numpy().astype(np.float64), noise.cpu().numpy().astype(np.float64)
    shift = np.abs(o[:, 0].mean(axis=1) - h[:, 0].astype(np.float64).mean(axis=1))
    bound = 2.0 ** -23 * (np.abs(o[:, 0]).max(axis=1) + np.abs(a[:, 0]).max(axis=1))
    assert (shift <= bound).all(), (shift / bound).max()
    raw = engine.state_noise(st, N.SEEDS, (sn, 0.0, 0.0), zero_mean=False).cpu().numpy().astype(np.float64)
    raw_shift = np.abs(raw[:, 0].mean(axis=1) - h[:, 0].astype(np.float64).mean(axis=1))
    assert (raw_shift > bound).sum() > B // 2


def test_bad_seed_gives_nan_and_spares_neighbours(hf, grids, start):
    """Device seeds cannot be validated on the host: a seed outside [0, 2^32)
    makes that sample's rows NaN and leaves the others as they are."""
    from hybridflux import engine
    nx = 64
    grid, st = grids[nx], start[nx][1][:4].contiguous()
    good = engine.state_noise(st[[0, 3]].contiguous(), [5, 7], (1e-2, 1e-2, 5e-3))
    seeds = torch.tensor([5, -1, 2 ** 32, 7], dtype=torch.int64, device=DEV)
    out, noise = engine.state_noise(st, seeds, (1e-2, 1e-2, 5e-3), return_noise=True)
    assert torch.isnan(out[1:3]).all() and torch.isnan(noise[1:3]).all()
    assert (bits(out[[0, 3]]) == bits(good)).all()
    out = engine.state_noise(st, seeds, (1e-2, 1e-2, 0.0), grid=grid)
    assert torch.isnan(out[1:3]).all() and torch.isfinite(out[[0, 3]]).all()
    with pytest.raises(ValueError, match="Seed must be between"):
        engine.state_noise(st, [5, -1, 2 ** 32, 7], (1e-2, 1e-2, 0.0))


@pytest.mark.parametrize("nx", [250, 256, 1024])
@pytest.mark.parametrize("bad_at", [0, 1, 2, 3, 4])
def test_bad_seed_with_grid_spares_its_fft_partner(hf, grids, start, nx, bad_at):
    """At the FFT sizes the Poisson launch transforms samples 2k and 2k+1 as one
    complex row, so a NaN n row would reach the pair partner's E'.  A bad seed at
    an even and at an odd position (and last, without a partner): its own rows,
    node features and noise are NaN, every other sample is the clean call's bits."""
    from hybridflux import engine
    grid, st = grids[nx], start[nx][1][:5].contiguous()
    x = grid.on(torch.device(DEV))[0]
    sigma = (1e-2, 1e-2, 0.0)
    good_seeds = [5, 7, 11, 13, 17]
    clean = engine.state_noise(st, good_seeds, sigma, grid=grid, x=x, return_noise=True)
    for bad in (-1, 2 ** 32):
        seeds = torch.tensor(good_seeds, dtype=torch.int64, device=DEV)
        seeds[bad_at] = bad
        for out in (None, "in place"):
            buf = st.clone()
            got = engine.state_noise(buf, seeds, sigma, grid=grid, x=x, return_noise=True,
                                     out=buf if out else None)
            keep = [b for b in range(5) if b != bad_at]
            for g, c, per in zip(got, clean, (1, nx, 1)):        # the node features hold nx rows per sample
                g, c = g.reshape(5, -1), c.reshape(5, -1)
                assert torch.isnan(g[bad_at].reshape(-1, 4)[:, :3] if per == nx else g[bad_at]).all()
                assert (bits(g[keep]) == bits(c[keep])).all(), (bad, out)
            assert (bits(got[1].reshape(5, nx, 4)[bad_at, :, 3]) == bits(x)).all()
    # without node features the failed sample is sealed all the same
    seeds = torch.tensor(good_seeds, dtype=torch.int64, device=DEV)
    seeds[bad_at] = -1
    plain = engine.state_noise(st, seeds, sigma, grid=grid)
    assert torch.isnan(plain[bad_at]).all() and (bits(plain[keep]) == bits(clean[0][keep])).all()


def test_zero_mean_at_its_limit(hf, record):
    """nx = 6144, the largest row the zero-mean path holds in LDS (48 KiB), B = 3."""
    from hybridflux import engine
    nx, seeds, sigma = 6144, [0, 42, 2 ** 32 - 1], (1e-2, 1e-2, 5e-3)
    h = N.states(nx, 3)
    out, noise = engine.state_noise(torch.as_tensor(h, device=DEV), seeds, sigma, zero_mean=True, return_noise=True)
    rs = [N.reference(s, nx, sigma, True, h[k]) for k, s in enumerate(seeds)]
    gate(out, np.stack([r["out"] for r in rs]), record, "test_zero_mean_at_its_limit", "state")
    gate(noise, np.stack([r["noise"] for r in rs]), record, "test_zero_mean_at_its_limit", "noise")


def test_empty_batch_wide_rows_and_refusals(hf, grids):
    from hybridflux import _lib, engine
    empty = engine.state_noise(torch.empty(0, 3, 64, device=DEV), [], (1e-2, 1e-2, 0.0), grid=grids[64])
    assert empty.shape == (0, 3, 64) and empty.is_cuda
    # beyond the zero-mean limit: supported without zero mean, refused with it
    nx, seeds = 8192, [0, 42, 2 ** 32 - 1]
    h = N.states(nx, 3)
    st = torch.as_tensor(h, device=DEV)
    out = engine.state_noise(st, seeds, (1e-2, 1e-2, 5e-3), zero_mean=False).cpu().numpy()
    want = np.stack([N.reference(s, nx, (1e-2, 1e-2, 5e-3), False, h[k])["out"] for k, s in enumerate(seeds)])
    assert np.abs(out.astype(np.float64) - want).max() <= 2.0 * np.spacing(np.abs(want).max().astype(np.float32))
    assert (bits(out) != bits(want)).sum() <= UNEQUAL_FRACTION * out.size
    with pytest.raises(_lib.HybridFluxError) as e:
        engine.state_noise(st, seeds, (1e-2, 1e-2, 0.0), zero_mean=True)
    assert e.value.code == _lib.HF_EUNSUPPORTED
    st = torch.zeros(2, 3, 64, device=DEV)
    with pytest.raises(ValueError, match="one seed per sample"):
        engine.state_noise(st, [1, 2, 3], (1e-2, 0, 0))
    with pytest.raises(ValueError, match="sigma_E must be 0"):
        engine.state_noise(st, [1, 2], (1e-2, 0, 1e-3), grid=grids[64])
    with pytest.raises(ValueError, match="contiguous float32"):
        engine.state_noise(st.double(), [1, 2], (1e-2, 0, 0))


def test_capturable(hf, grids, start):
    """No allocation and no host synchronisation inside the call: it captures
    into a graph, and the replay gives the eager call's bits."""
    from hybridflux import _lib, engine
    nx = 64
    grid, st = grids[nx], start[nx][1]
    x, plan = grid.on(torch.device(DEV))
    sig = engine.noise_sigma((1e-2, 1e-2, 0.0))
    seeds = torch.as_tensor(np.asarray(N.SEEDS, dtype=np.int64), device=DEV)
    want = engine.state_noise(st, seeds, sig, grid=grid, x=x, return_noise=True)
    out, nf, noise = torch.zeros_like(st), torch.zeros(B * nx, 4, device=DEV), torch.zeros_like(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(_lib.lib().hf_state_noise(_lib.ptr(seeds), B, nx, _lib.ptr(sig), _lib.HF_NOISE_ZERO_MEAN,
                                             _lib.ptr(st), _lib.ptr(out), _lib.ptr(plan), grid.pmode, _lib.ptr(x),
                                             _lib.ptr(nf), _lib.ptr(noise), engine.stream_of(torch.device(DEV))))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(want, (out, nf, noise)):
        assert (bits(a) == bits(b)).all()
