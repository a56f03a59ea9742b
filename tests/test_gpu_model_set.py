"""Model sets: HybridEnsemble.run_batch / compare_batch (hf_run_set /
hf_run_compare_set: M checkpoints rolled out in one launch whose workgroups
each pick their model) and evaluation.compare_models(grouped=True).

The yardstick is the single-model path, HybridSolver.run_batch / compare_batch
called once per model; every comparison is bit for bit on every returned
tensor, so there is no tolerance anywhere in this file.  A kernel that serves
every workgroup from model 0, maps workgroups to models off by one, or lets a
model's ragged last workgroup touch its neighbour's ICs fails the first test:
the models' outputs differ pairwise and permuting the models permutes the
leading axis exactly.
"""
import numpy as np
import pytest
import torch

from conftest import GOLDEN, rand_sd
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ("f32", "f16x3", "bf16")
_SOLVERS, _ICS = {}, {}


def solver(seed, layers=4, precision="f32", nx=64, poisson="spectral", dt=5e-3, device=DEV):
    """HybridSolver on rand_sd(layers, seed), shared by the tests that ask for the same one."""
    import hybridflux as hf
    key = (seed, layers, precision, nx, poisson, dt, device)
    if key not in _SOLVERS:
        _SOLVERS[key] = hf.HybridSolver(rand_sd(layers, seed), 1, nx=nx, dt=dt, device=device, precision=precision,
                                        poisson=poisson, num_layers=layers)
    return _SOLVERS[key]


def ics(nx, B, seed0=4000):
    if (nx, B, seed0) not in _ICS:
        g = O.Grid(nx)
        _ICS[nx, B, seed0] = torch.as_tensor(np.stack([O.initial_condition(g, s) for s in range(seed0, seed0 + B)]),
                                             device=DEV)
    return _ICS[nx, B, seed0]


def same(a, b, what):
    """Bit for bit (NaNs by their bits too), same shape and dtype."""
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, (what, a.shape, b.shape)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
            f"{what}: {int((a.view(torch.int32) != b.view(torch.int32)).sum())} of {a.numel()} values differ"


def loop(solvers, s0, T, scored, **kw):
    """The single-model yardstick: one call per model, stacked on a leading model axis."""
    rs = []
    for i, s in enumerate(solvers):
        si = s0 if s0.dim() == 3 else s0[i]
        rs.append(s.compare_batch(si, T, **kw) if scored else s.run_batch(si, T, **kw))
    return {k: None if rs[0][k] is None else torch.stack([r[k] for r in rs]) for k in rs[0]}


def check(got, want, what):
    assert set(got) == set(want)
    for k in want:
        same(got[k], want[k], f"{what} {k}")


UNSCORED = dict(traj=True, flux=True, metrics=True)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nx", [16, 32, 48, 64])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_unscored_small(precision, nx, B):
    """M = 3 from shared ICs: the cell-split kernels at nx 32/48/64 (15 ICs in
    all), the IC-per-wave kernel at 16.  B = 5 leaves every model a ragged last
    workgroup (4 ICs per workgroup; 2 at nx 32 and 1 at 48, 64 cell-split)."""
    import hybridflux as hf
    solvers = [solver(100 + i, precision=precision, nx=nx) for i in range(3)]
    s0, T = ics(nx, B), 3
    want = loop(solvers, s0, T, False, **UNSCORED)
    got = hf.HybridEnsemble(solvers).run_batch(s0, T, **UNSCORED)
    assert got["final"].shape == (3, B, 3, nx) and got["traj"].shape == (3, B, T + 1, 3, nx)
    assert got["flux"].shape == (3, B, T, nx) and got["metrics"].shape == (3, B, T + 1, 4)
    check(got, want, f"{precision} nx={nx} B={B}")
    # sharpness: the models really differ, and the leading axis follows the models' order
    for k in ("final", "traj", "flux", "metrics"):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert not torch.equal(want[k][i], want[k][j]), f"models {i} and {j} give the same {k}"
    perm = [2, 0, 1]
    gp = hf.HybridEnsemble([solvers[i] for i in perm]).run_batch(s0, T, **UNSCORED)
    for k in want:
        same(gp[k], want[k][perm], f"permuted {k}")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nx,poisson", [(16, "spectral"), (32, "spectral"), (48, "spectral"), (64, "spectral"),
                                        (64, "tridiagonal")])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_scored_small(precision, nx, poisson, B):
    """compare_batch: the classical twin forces the IC-per-wave kernel."""
    import hybridflux as hf
    solvers = [solver(100 + i, precision=precision, nx=nx, poisson=poisson) for i in range(3)]
    s0, T = ics(nx, B), 3
    want = loop(solvers, s0, T, True)
    got = hf.HybridEnsemble(solvers).compare_batch(s0, T)
    assert set(got) == {"final", "mse", "metrics", "metrics_classical"} and got["mse"].shape == (3, B, T + 1, 3)
    check(got, want, f"scored {precision} nx={nx} {poisson} B={B}")
    assert not torch.equal(want["mse"][0], want["mse"][1]) and not torch.equal(want["mse"][1], want["mse"][2])
    same(hf.HybridEnsemble(solvers).compare_batch(s0, T, metrics=False)["mse"], want["mse"], "mse without metrics")


def test_unscored_wave_kernel_by_size():
    """M = 3, B = 345 at nx = 64: 1035 ICs reach the IC-per-wave kernel unscored.
    chain_rollout_prefers_cells sees the launch's total: on 256 CUs 1035 ICs are
    5 rounds of one-IC cell-split workgroups at 1.6 units against 2 rounds of
    four-IC workgroups at 4, 8.0 against 8.0, and a tie goes to the wave
    kernel (one model's 345 ICs alone take the cell-split kernel: 2 x 1.6 < 1 x 4).
    345 = 86*4 + 1, so every model ends in a workgroup with one live wave."""
    import hybridflux as hf
    solvers = [solver(100 + i) for i in range(3)]
    s0 = ics(64, 5).repeat(69, 1, 1) * torch.linspace(0.97, 1.03, 345, device=DEV)[:, None, None]
    want = loop(solvers, s0, 2, False, **UNSCORED)
    check(hf.HybridEnsemble(solvers).run_batch(s0, 2, **UNSCORED), want, "B=345")


def test_trained_weights():
    """The four trained checkpoints of tests/golden as one set, scored and unscored."""
    import hybridflux as hf
    paths = [f"{GOLDEN}/weights_{n}.npz" for n in ("W0", "W1_r1", "W1_r2", "W1_r3")]
    ens = hf.HybridEnsemble.from_checkpoints(paths, radius=1, device=DEV)
    assert len(ens) == 4 and ens[3].radius == 1
    s0 = ics(64, 5)
    check(ens.run_batch(s0, 3, **UNSCORED), loop(ens.solvers, s0, 3, False, **UNSCORED), "trained")
    check(ens.compare_batch(s0, 3), loop(ens.solvers, s0, 3, True), "trained scored")


def test_ics_per_model():
    """states0 [M,B,3,nx] with different states per model, out of place and in place."""
    import hybridflux as hf
    solvers = [solver(100 + i, nx=48) for i in range(2)]
    ens = hf.HybridEnsemble(solvers)
    s0 = torch.stack([ics(48, 5), ics(48, 5, seed0=4100)])
    assert not torch.equal(s0[0], s0[1])
    for scored, kw in ((False, UNSCORED), (True, {})):
        want = loop(solvers, s0, 3, scored, **kw)
        call = ens.compare_batch if scored else ens.run_batch
        check(call(s0, 3, **kw), want, f"per-model ICs scored={scored}")
        st = s0.clone()
        got = call(st, 3, out=st, **kw)
        assert got["final"] is st
        check(got, want, f"per-model ICs in place scored={scored}")
    # the same ICs for every model, given per model, equal the shared call
    rep = ics(48, 5).expand(2, -1, -1, -1).contiguous()
    check(ens.run_batch(rep, 3, **UNSCORED), ens.run_batch(ics(48, 5), 3, **UNSCORED), "shared vs repeated")


def test_mixed_depth():
    """layers (2, 4, 1) in one launch: each workgroup streams its own model's chunk count."""
    import hybridflux as hf
    solvers = [solver(200 + i, layers=L) for i, L in enumerate((2, 4, 1))]
    ens, s0 = hf.HybridEnsemble(solvers), ics(64, 5)
    check(ens.run_batch(s0, 3, **UNSCORED), loop(solvers, s0, 3, False, **UNSCORED), "mixed depth")
    check(ens.compare_batch(s0, 3), loop(solvers, s0, 3, True), "mixed depth scored")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_model_set(precision):
    import hybridflux as hf
    s, s0 = solver(100, precision=precision), ics(64, 5)
    ens = hf.HybridEnsemble([s])
    check(ens.run_batch(s0, 3, **UNSCORED), loop([s], s0, 3, False, **UNSCORED), "M=1")
    check(ens.compare_batch(s0, 3), loop([s], s0, 3, True), "M=1 scored")


def test_unfused_nx_runs_model_after_model():
    import hybridflux as hf
    solvers = [solver(100 + i, nx=20) for i in range(2)]
    ens, s0 = hf.HybridEnsemble(solvers), ics(20, 3)
    check(ens.run_batch(s0, 3, **UNSCORED), loop(solvers, s0, 3, False, **UNSCORED), "nx=20")
    check(ens.run_batch(s0, 3, traj=False), loop(solvers, s0, 3, False, traj=False), "nx=20 no traj")
    check(ens.compare_batch(s0, 3), loop(solvers, s0, 3, True), "nx=20 scored")


def test_summaries_take_the_model_axis():
    """multi_ic_mse and long_rollout on an ensemble: every result with a leading model axis."""
    import hybridflux as hf
    from hybridflux import evaluation
    solvers = [solver(100 + i) for i in range(3)]
    ens, s0 = hf.HybridEnsemble(solvers), ics(64, 5)
    mean, r, d = evaluation.multi_ic_mse(ens, s0, 4)
    assert mean.shape == (3, 5) and r["mse"].shape == (3, 5, 5, 3)
    lr = evaluation.long_rollout(ens, s0, 4)
    assert lr["energy_drift_pred"].shape == (3, 5, 5) and lr["exploded"].shape == (3, 5)
    for i, s in enumerate(solvers):
        m1, _, d1 = evaluation.multi_ic_mse(s, s0, 4)
        same(mean[i], m1, "mean mse")
        l1 = evaluation.long_rollout(s, s0, 4)
        for k in d1:
            same(d[k][i], d1[k], k)
        for k in ("energy_drift_pred", "metrics", "final_energy_drift"):
            same(lr[k][i], l1[k], k)


def test_compare_models_grouped_equals_loop():
    import hybridflux as hf
    from hybridflux import evaluation
    torch.manual_seed(5)
    pure = evaluation.ModelRollout(hf.PureGNN(4, 64, 2).to(DEV), hf.BaselineSolver(nx=64, device=DEV))
    models = {"h0": solver(100), "pure": pure, "h1": solver(101), "bf16": solver(102, precision="bf16"),
              "h2": solver(103, layers=2)}
    assert evaluation.ensemble_groups(models) == [["h0", "h1", "h2"]]
    s0 = ics(64, 6)
    grouped = evaluation.compare_models(models, s0, 5)
    assert grouped == evaluation.compare_models(models, s0, 5, grouped=False)
    assert list(grouped) == list(models) and len(grouped["h1"]["mse_per_ic"]) == 6
    assert len({grouped[k]["mean_mse"] for k in models}) == 5


def test_capture_and_replay():
    import hybridflux as hf
    solvers = [solver(100 + i) for i in range(3)]
    ens, s0 = hf.HybridEnsemble(solvers), ics(64, 5).clone()
    want = ens.run_batch(s0, 3, traj=False, metrics=True)      # eager; also builds the set's table
    out, met = torch.empty(3, 5, 3, 64, device=DEV), torch.empty(3, 5, 4, 4, device=DEV)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    out.zero_()
    met.zero_()
    torch.cuda.synchronize(DEV)
    with torch.cuda.graph(g, stream=stream):
        ens.run_batch(s0, 3, traj=False, metrics=met, out=out)
    for _ in range(2):
        out.zero_()
        met.zero_()
        g.replay()
        torch.cuda.synchronize(DEV)
        same(out, want["final"], "replayed final")
        same(met, want["metrics"], "replayed metrics")


def test_errors_before_any_launch():
    import hybridflux as hf
    a = solver(100)
    for other, field in ((solver(101, nx=32), "nx"), (solver(101, dt=2e-3), "dt"),
                         (solver(101, precision="f16x3"), "precision"), (solver(101, device="cpu"), "device")):
        with pytest.raises(ValueError, match=f"solver 1 has {field} = "):
            hf.HybridEnsemble([a, other])
    ens = hf.HybridEnsemble([a, solver(101)])
    big = torch.zeros(2, 5, 3, 64, device=DEV)
    for call in (ens.run_batch, ens.compare_batch):
        with pytest.raises(ValueError, match="share memory"):
            call(big[0], 2, out=big)                                  # shared ICs rolled out in place
        for bad in (torch.zeros(3, 64, device=DEV), torch.zeros(1, 2, 5, 3, 64, device=DEV),
                    torch.zeros(3, 5, 3, 64, device=DEV), torch.zeros(5, 3, 32, device=DEV)):
            with pytest.raises(ValueError, match="states0 must be"):
                call(bad, 2)
        with pytest.raises(ValueError, match="preallocated output"):
            call(big[0].clone(), 2, out=torch.zeros(5, 3, 64, device=DEV))   # out without the model axis
    assert not big.any()                                              # nothing ran
    from hybridflux import engine
    with pytest.raises(ValueError, match="shares one precision"):
        engine.DeviceModelSet([a._dm(), solver(101, precision="bf16")._dm()])
    mset = ens._model_set()
    with pytest.raises(ValueError, match="state must be float32"):
        engine.run_set(mset, ens.grid, torch.zeros(5, 3, 64, device=DEV, dtype=torch.float64), 2)
