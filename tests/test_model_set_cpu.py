"""HybridEnsemble's compatibility checks and shape handling, and which entries of
compare_models share a launch, without a device: the solvers live on "cpu"
(nothing is computed there) and engine.run_set / run_compare_set are replaced
by stubs that record what the ensemble hands the engine."""
import numpy as np
import pytest
import torch

from conftest import rand_sd
import hybridflux
from hybridflux import HybridEnsemble, HybridSolver, engine, evaluation


def solver(seed=0, layers=4, **kw):
    kw.setdefault("device", "cpu")
    return HybridSolver(rand_sd(layers, seed), 1, num_layers=layers, **kw)


class Recorder:
    def __init__(self, monkeypatch, ens):
        self.calls = []
        monkeypatch.setattr(ens, "_model_set", lambda: "the-set")
        monkeypatch.setattr(engine, "run_set", self._rec("run"))
        monkeypatch.setattr(engine, "run_compare_set", self._rec("compare"))

    def _rec(self, kind):
        def f(mset, grid, s0, T, **kw):
            self.calls.append((kind, mset, grid, s0, T, kw))
            return {"final": s0}
        return f


def test_public_surface():
    assert "HybridEnsemble" in hybridflux.__all__ and hybridflux.HybridEnsemble is HybridEnsemble
    for n in ("DeviceModelSet", "run_set", "run_compare_set"):
        assert hasattr(engine, n)
    assert "mean(0)" in HybridEnsemble.__doc__ and "std(0)" in HybridEnsemble.__doc__   # the ensemble statistic shown


def test_members_and_indexing():
    a, b, c = solver(1), solver(2, layers=2), solver(3, layers=1)   # depths may differ
    ens = HybridEnsemble([a, b, c])
    assert len(ens) == 3 and ens[0] is a and ens[2] is c and ens[-1] is c
    assert ens.grid is a.grid and ens.device == torch.device("cpu")
    with pytest.raises(ValueError, match="at least one"):
        HybridEnsemble([])
    assert isinstance(HybridEnsemble.from_checkpoints([rand_sd(4, 5), rand_sd(4, 6)], radius=2, device="cpu", nx=32)[1],
                      HybridSolver)
    e2 = HybridEnsemble.from_checkpoints([rand_sd(4, 5), rand_sd(4, 6)], radius=2, device="cpu", nx=32)
    assert len(e2) == 2 and e2.grid.nx == 32 and e2[0].radius == 2


@pytest.mark.parametrize("kw,field", [
    (dict(nx=32), "nx"), (dict(length=3.0), "length"), (dict(dt=1e-3), "dt"),
    (dict(poisson="tridiagonal"), "poisson"), (dict(precision="bf16"), "precision"), (dict(device="meta"), "device"),
])
def test_first_mismatch_is_named(kw, field):
    with pytest.raises(ValueError, match=rf"solver 2 has {field} = "):
        HybridEnsemble([solver(1), solver(2), solver(3, **kw), solver(4, nx=16)])


def test_first_of_two_mismatches_is_named():
    # nx comes before precision in HybridEnsemble.SIGNATURE
    with pytest.raises(ValueError, match="solver 1 has nx = 48"):
        HybridEnsemble([solver(1), solver(2, nx=48, precision="f16x3")])


def test_nu_is_part_of_the_signature():
    a, b = solver(1), solver(2)
    b.baseline.grid = engine.Grid(nx=64, dt=5e-3, nu=2e-3)
    with pytest.raises(ValueError, match="solver 1 has nu = 0.002"):
        HybridEnsemble([a, b])


def test_shapes_and_arguments_reach_the_engine(monkeypatch):
    ens = HybridEnsemble([solver(1), solver(2), solver(3)])
    rec = Recorder(monkeypatch, ens)
    shared = np.zeros((5, 3, 64))                       # numpy float64, as the reference's callers pass
    own = torch.zeros(3, 5, 3, 64)
    out = torch.empty(3, 5, 3, 64)
    ens.run_batch(shared, 7, traj=False, metrics=True, out=out)
    ens.run_batch(own, 2, flux=True, out=own)           # in place with ICs per model
    ens.compare_batch(own, 4, metrics=False)
    (k0, set0, g0, s0, T0, kw0), (k1, _, _, s1, T1, kw1), (k2, _, _, s2, T2, kw2) = rec.calls
    assert (k0, k1, k2) == ("run", "run", "compare") and set0 == "the-set" and g0 is ens.grid
    assert s0.shape == (5, 3, 64) and s0.dtype == torch.float32 and T0 == 7
    assert kw0 == dict(traj=False, flux=False, metrics=True, out=out, ws=None)
    assert s1 is own and T1 == 2 and kw1["out"] is own and kw1["flux"] is True and kw1["traj"] is True
    assert s2 is own and T2 == 4 and kw2 == dict(metrics=False, out=None, ws=None)


@pytest.mark.parametrize("shape", [(3, 64), (5, 3, 32), (5, 4, 64), (2, 5, 3, 64), (4, 5, 3, 64), (1, 3, 5, 3, 64)])
def test_wrong_states_are_refused_before_the_engine(monkeypatch, shape):
    ens = HybridEnsemble([solver(1), solver(2), solver(3)])
    rec = Recorder(monkeypatch, ens)
    for call in (ens.run_batch, ens.compare_batch):
        with pytest.raises(ValueError, match=r"states0 must be \[B,3,64\]"):
            call(torch.zeros(shape), 3)
    assert rec.calls == []


def test_shared_ics_in_place_are_refused_before_the_engine(monkeypatch):
    ens = HybridEnsemble([solver(1), solver(2)])
    rec = Recorder(monkeypatch, ens)
    big = torch.zeros(2, 5, 3, 64)
    shared = big[0]
    for call in (ens.run_batch, ens.compare_batch):
        with pytest.raises(ValueError, match="share memory"):
            call(shared, 3, out=big)
    assert rec.calls == []


def test_grouping_of_compare_models():
    f32 = [solver(i) for i in range(3)]
    bf = [solver(10 + i, precision="bf16") for i in range(2)]
    odd_nx = solver(20, nx=32)
    deep = solver(21, layers=2)                        # another depth shares the launch
    rollout = evaluation.ModelRollout(object(), f32[0].baseline)
    models = {"a": f32[0], "pure": rollout, "b16a": bf[0], "b": f32[1], "nx32": odd_nx, "c": f32[2], "b16b": bf[1],
              "deep": deep}
    assert evaluation.ensemble_groups(models) == [["a", "b", "c", "deep"], ["b16a", "b16b"]]
    assert evaluation.ensemble_groups({"a": f32[0], "pure": rollout, "nx32": odd_nx, "b16": bf[0]}) == []
    assert evaluation.ensemble_groups({}) == []


def test_compare_models_groups_and_keeps_the_order(monkeypatch):
    """grouped=True runs each group as one HybridEnsemble and everything else on
    its own; the rows come back under their names, in the dict's order."""
    f32 = [solver(i) for i in range(3)]
    bf = solver(10, precision="bf16")
    models = {"x": f32[0], "lonely": bf, "y": f32[1], "z": f32[2]}
    seen = []

    def fake_multi_ic_mse(s, states0, n_steps):
        seen.append(s)
        if isinstance(s, HybridEnsemble):
            return torch.stack([torch.full((2,), float(id(m) % 997)) for m in s.solvers]), None, None
        return torch.full((2,), float(id(s) % 997)), None, None

    monkeypatch.setattr(evaluation, "multi_ic_mse", fake_multi_ic_mse)
    got = evaluation.compare_models(models, None, 3)
    assert len(seen) == 2 and isinstance(seen[0], HybridEnsemble) and seen[0].solvers == f32 and seen[1] is bf
    assert list(got) == list(models)
    for k, m in models.items():
        assert got[k]["mse_per_ic"] == [float(id(m) % 997)] * 2 and got[k]["std_mse"] == 0.0
    seen.clear()
    assert evaluation.compare_models(models, None, 3, grouped=False) == got
    assert seen == list(models.values())
