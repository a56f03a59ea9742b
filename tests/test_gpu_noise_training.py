"""Training on perturbed start states (training.StateNoise, the noise= option
of WindowDataset.batch, FluxDataset.batch and the three K-step trainers) on the
MI355X.  Everything here is bit for bit: the noisy batch is the clean batch with
engine.state_noise applied to its start states, a step on it is the existing
step on that composition, a trainer with noise= repeats itself and differs from
the run without, and noise=None is the call without the keyword.

Shapes: 6 trajectories of 8 steps, K = 2, batches of 4, two epochs, nx = 16 and
64; PureGNN and PINN at hidden 64 with 3 layers (FluxGNN's trainer fixes
MODEL_CONFIG's 128 x 4)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NXS = (16, 64)
K, BATCH, EPOCHS = 2, 4, 2
MODELS = ("flux", "pure", "pinn")


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


@pytest.fixture(scope="module")
def data(hf):
    """Per nx: the solver and its classical trajectories [6,9,3,nx], made once."""
    from hybridflux import datagen

    class Data(dict):
        def __missing__(self, nx):
            tr = datagen.generate_trajectories(nx=nx, num_initial_conditions=6, steps_per_ic=8, device=DEV)
            assert tr.shape == (6, 9, 3, nx)
            self[nx] = (hf.BaselineSolver(nx, device=DEV), tr)
            return self[nx]
    return Data()


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def flat_of(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()


def noise_of(name, grid):
    """FluxGNN's trainer recomputes E on its own grid; PureGNN's noise brings a
    grid, PINN's a sigma_E."""
    from hybridflux import training
    if name == "flux":
        return training.StateNoise(1e-2, 1e-2)
    if name == "pure":
        return training.StateNoise(1e-2, 3e-3, grid=grid)
    return training.StateNoise(1e-2, 1e-2, 5e-3, zero_mean=False)


@pytest.mark.parametrize("nx", NXS)
def test_window_dataset_batch(hf, data, nx):
    from hybridflux import engine, training
    s, tr = data[nx]
    d = training.WindowDataset(tr, K, DEV)
    idx = torch.tensor([0, 5, len(d) - 1, 17, 5], device=DEV)
    seeds = torch.tensor([3, 2 ** 32 - 1, 0, 77, 3], dtype=torch.int64, device=DEV)
    clean = d.batch(idx)
    for noise in (training.StateNoise(1e-2, 1e-2, 5e-3), training.StateNoise(1e-2, 3e-3, grid=s.grid)):
        win = d.batch(idx, noise, seeds)
        assert win.shape == clean.shape == (5, K + 1, 3, nx)
        assert (bits(win[:, 1:]) == bits(clean[:, 1:])).all()
        want = engine.state_noise(clean[:, 0].contiguous(), seeds, noise.sigma, noise.zero_mean, noise.grid)
        assert (bits(win[:, 0]) == bits(want)).all()
        assert not (bits(win[:, 0, :2]) == bits(clean[:, 0, :2])).all()
        assert (bits(d.batch(idx)) == bits(clean)).all()           # the dataset itself is not written
        assert (bits(d.batch(idx, noise, seeds.cpu().tolist())) == bits(win)).all()   # host seeds: the same windows
    assert (bits(d.batch(idx, noise=None)) == bits(clean)).all()


@pytest.mark.parametrize("nx", NXS)
def test_flux_dataset_batch(hf, data, nx):
    from hybridflux import engine, training
    s, tr = data[nx]
    st, sn = tr[:, :-1].reshape(-1, 3, nx), tr[:, 1:].reshape(-1, 3, nx)
    ft = (st[:, 0] * st[:, 1]).astype(np.float32)
    d = training.FluxDataset(st, ft, sn, DEV)
    x = s.grid.on(torch.device(DEV))[0]
    idx = torch.tensor([0, 11, len(d) - 1, 11], device=DEV)
    seeds = torch.tensor([9, 1, 2 ** 32 - 1, 9], dtype=torch.int64, device=DEV)
    noise = training.StateNoise(1e-2, 1e-2, grid=s.grid)
    c_st, c_ft, c_sn, c_nf = d.batch(idx, s.x)
    n_st, n_ft, n_sn, n_nf = d.batch(idx, s.x, noise=noise, seeds=seeds)
    assert (bits(n_ft) == bits(c_ft)).all() and (bits(n_sn) == bits(c_sn)).all()
    w_st, w_nf = engine.state_noise(c_st, seeds, noise.sigma, True, s.grid, x)
    assert (bits(n_st) == bits(w_st)).all() and (bits(n_nf) == bits(w_nf)).all()
    want = torch.cat([n_st.permute(0, 2, 1), x[None, :, None].expand(4, nx, 1)], dim=2).reshape(4 * nx, 4)
    assert (bits(n_nf) == bits(want)).all() and not (bits(n_nf) == bits(c_nf)).all()
    p_st, p_ft, p_sn = d.batch(idx, noise=noise, seeds=seeds)       # without x: no node features
    assert (bits(p_st) == bits(n_st)).all() and (bits(p_ft) == bits(c_ft)).all() and (bits(p_sn) == bits(c_sn)).all()
    for a, b in zip(d.batch(idx, s.x, noise=None), (c_st, c_ft, c_sn, c_nf)):
        assert (bits(a) == bits(b)).all()


def fresh(hf, name, nx):
    from hybridflux import training
    torch.manual_seed(nx)
    m = {"flux": lambda: hf.FluxGNN(4, 128, 4), "pure": lambda: hf.PureGNN(4, 64, 3),
         "pinn": lambda: hf.PINN(3 * nx, 64, 3)}[name]()
    m = m.to(DEV).flatten_parameters_()
    return m, training.FlatAdam(m.parameters(), lr=1e-3)


def step(name, m, opt, win, s):
    from hybridflux import training
    x = s.grid.on(torch.device(DEV))[0]
    if name == "flux":
        return training.unrolled_step(m, opt, win, x, s.grid)
    if name == "pure":
        return training.pure_unrolled_step(m, opt, win, x)
    return training.pinn_unrolled_step(m, opt, win)


@pytest.mark.parametrize("nx", NXS)
@pytest.mark.parametrize("name", MODELS)
def test_step_on_noisy_batch_is_the_composition(hf, data, name, nx):
    """One *_unrolled_step on WindowDataset's noisy batch = engine.state_noise on
    the clean batch's start states, then the same step."""
    from hybridflux import engine, training
    s, tr = data[nx]
    d = training.WindowDataset(tr, K, DEV)
    noise = noise_of(name, s.grid)
    if name == "flux":
        noise = noise.with_grid(s.grid)
    idx = torch.tensor([1, 8, 20, 33], device=DEV)
    seeds = torch.tensor([4, 40, 400, 4000], dtype=torch.int64, device=DEV)
    m1, o1 = fresh(hf, name, nx)
    before = flat_of(m1)
    l1 = step(name, m1, o1, d.batch(idx, noise, seeds), s)
    manual = d.batch(idx)
    manual[:, 0] = engine.state_noise(manual[:, 0].contiguous(), seeds, noise.sigma, noise.zero_mean, noise.grid)
    m2, o2 = fresh(hf, name, nx)
    l2 = step(name, m2, o2, manual, s)
    assert l1 is not None and l2 is not None and float(l1) == float(l2)
    assert np.array_equal(flat_of(m1), flat_of(m2)) and not np.array_equal(flat_of(m1), before)
    m3, o3 = fresh(hf, name, nx)
    step(name, m3, o3, d.batch(idx), s)
    assert not np.array_equal(flat_of(m3), flat_of(m1))            # the clean step is another step


def train(name, s, tr, **kw):
    from hybridflux import training
    common = dict(K=K, epochs=EPOCHS, batch_size=BATCH, seed=0, device=DEV, save_dir=None, log=None, **kw)
    if name == "flux":
        return training.train_unrolled(tr, s.x, s.dt, s.dx, s.nu, lr=1e-4, **common)
    if name == "pure":
        return training.train_pure_gnn_unrolled(tr, s.x, hidden_dim=64, num_layers=3, **common)
    return training.train_pinn_unrolled(tr, s.dx, s.dt, s.nu, hidden_dim=64, num_layers=3, **common)


@pytest.mark.parametrize("nx", NXS)
@pytest.mark.parametrize("name", MODELS)
def test_trainers_with_noise(hf, data, name, nx):
    """noise= repeats itself bit for bit, differs from the run without it and
    from another noise_seed; noise=None is the call without the keyword."""
    s, tr = data[nx]
    noise = noise_of(name, s.grid)
    m1, h1 = train(name, s, tr, noise=noise, noise_seed=5)
    m2, h2 = train(name, s, tr, noise=noise, noise_seed=5)
    assert np.array_equal(flat_of(m1), flat_of(m2)) and h1["loss"] == h2["loss"]
    assert sorted(h1) == ["epoch", "loss", "noise", "seconds"] and h1["epoch"] == [1, 2]
    assert h1["noise"] == [float(v) for v in noise.sigma] and np.isfinite(h1["loss"]).all()
    assert np.isfinite(flat_of(m1)).all()
    m0, h0 = train(name, s, tr)
    mn, hn = train(name, s, tr, noise=None)
    assert np.array_equal(flat_of(m0), flat_of(mn)) and h0["loss"] == hn["loss"]
    assert sorted(h0) == sorted(hn) == ["epoch", "loss", "seconds"]
    assert not np.array_equal(flat_of(m1), flat_of(m0)) and h1["loss"] != h0["loss"]
    m3, _ = train(name, s, tr, noise=noise, noise_seed=6)
    assert not np.array_equal(flat_of(m3), flat_of(m1))


def test_trainer_seeds_and_refusals(hf, data):
    """The epoch's seeds come from a generator of their own: torch.randint(0,
    2**32, (len(data),), int64) seeded with noise_seed, indexed by sample."""
    from hybridflux import training
    s, tr = data[16]
    d = training.WindowDataset(tr, K, DEV)
    noise = training.StateNoise(1e-2, 1e-2, grid=s.grid)
    seen = []
    real = training.WindowDataset.batch

    def spy(self, idx, noise=None, seeds=None):
        seen.append((idx.cpu().numpy().copy(), None if seeds is None else seeds.cpu().numpy().copy()))
        return real(self, idx, noise, seeds)
    training.WindowDataset.batch = spy
    try:
        train("pure", s, tr, noise=noise, noise_seed=11)
    finally:
        training.WindowDataset.batch = real
    g, go = torch.Generator().manual_seed(11), torch.Generator().manual_seed(0)
    per_epoch = -(-len(d) // BATCH)
    assert len(seen) == EPOCHS * per_epoch
    for e in range(EPOCHS):
        order = torch.randperm(len(d), generator=go).numpy()            # the shuffle is the clean run's
        want = torch.randint(0, 2 ** 32, (len(d),), dtype=torch.int64, generator=g).numpy()
        for j in range(per_epoch):
            idx, sd = seen[e * per_epoch + j]
            assert np.array_equal(idx, order[j * BATCH:(j + 1) * BATCH]) and np.array_equal(sd, want[idx])
    with pytest.raises(ValueError, match="sigma_E must be 0"):
        train("flux", s, tr, noise=training.StateNoise(1e-2, 1e-2, 5e-3))
    with pytest.raises(ValueError, match="needs seeds"):
        d.batch([0, 1], noise)
