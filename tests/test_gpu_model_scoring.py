"""Scored one-launch rollouts of the comparison models (PureGNN, PINN):
hf_pure_gnn_run_scored / hf_pinn_run_scored behind PureGNN.rollout /
PINN.rollout(metrics=, compare=), evaluation.ModelRollout and
evaluation.compare_models (scripts/evaluation/evaluate_multi_ic.py:21-136,
evaluate_long_rollout.py:18-81).

What is gated, and by what:
 * bit for bit (NaNs equal): final / traj against the unscored rollout;
   metrics against engine.traj_metrics of the recorded trajectory;
   metrics_classical against BaselineSolver.run_batch(metrics=True); mse against
   engine.traj_mse of the two recorded trajectories — on the one-launch shapes
   and on the shapes that sequence the existing kernels.
 * independently of the engine's scoring code: numpy float64 MSE and metrics
   from the float32 trajectories, rtol 2e-7 (one float32 rounding of a float64
   sum, 2^-24, with a margin of 3 for the summation order), atol 0.
 * against the reference's own trajectories (tests/golden/baselines.npz), per
   IC, step and channel: |got - ref| <= 2 sqrt(ref) eps + eps^2 + 2e-7 ref with
   eps = 1e-5 (1 + max |value in the row|): the trajectory gate of
   test_gpu_baselines.py (|traj - gold| <= 1e-5 + 1e-5 |gold|) pushed through
   mean((a + d)^2) - mean(a^2) by Cauchy-Schwarz, plus the rounding above.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = (0, 1, 5)
PURE_FUSED = [(64, 16, 1, 1), (64, 48, 2, 3), (128, 64, 4, 4), (128, 32, 0, 5)]
PURE_UNFUSED = [(64, 20, 2, 2), (32, 32, 1, 2)]
GUARD = 7.25


def eq(a, b, what=""):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b, equal_nan=True), f"{what}: {int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())} differ"


def _ics(nx, B, seed0=7000):
    grid = O.Grid(nx)
    return torch.as_tensor(np.stack([O.initial_condition(grid, s) for s in range(seed0, seed0 + B)]), device=DEV)


def _pure(H, L, seed=0):
    import hybridflux as hf
    torch.manual_seed(100 + H + L + seed)
    return hf.PureGNN(4, H, L).to(DEV)


def _pinn(D, H, L):
    import hybridflux as hf
    torch.manual_seed(200 + D + H + L)
    return hf.PINN(D, H, L).to(DEV)


def _rollout(model, base, s0, T, **kw):
    import hybridflux as hf
    if isinstance(model, hf.PureGNN):
        return model.rollout(s0, T, base.x, **kw)
    return model.rollout(s0, T, **kw)


def _metrics_np(traj):
    """[B,T1,3,nx] float32 -> [B,T1,4] float64: the reference's energy and charge
    (evaluate_all.py:135-143), the finite flag and max |n - 1| (float32 subtraction)."""
    t64 = traj.astype(np.float64)
    n, u, E = t64[:, :, 0], t64[:, :, 1], t64[:, :, 2]
    dev = np.abs(traj[:, :, 0] - np.float32(1.0)).max(-1).astype(np.float64)
    return np.stack([0.5 * (u * u + E * E).mean(-1), n.mean(-1), np.ones_like(dev), dev], -1)


def _check_scored(model, base, s0, T, got):
    """Checks 1-3 of one scored call (metrics and twin both asked) against the recorded path."""
    from hybridflux import engine
    plain = _rollout(model, base, s0, T)
    cl = base.run_batch(s0, T, traj=True, metrics=True)
    eq(got["final"], plain["final"], "final")
    eq(got["traj"], plain["traj"], "traj")
    eq(got["metrics"], engine.traj_metrics(plain["traj"]), "metrics")
    eq(got["metrics_classical"], cl["metrics"], "metrics_classical")
    eq(got["mse"], engine.traj_mse(plain["traj"], cl["traj"]), "mse")
    # numpy float64 from the float32 trajectories
    tm, tc = plain["traj"].cpu().numpy(), cl["traj"].cpu().numpy()
    want = ((tm.astype(np.float64) - tc.astype(np.float64)) ** 2).mean(-1)
    np.testing.assert_allclose(got["mse"].cpu().numpy(), want, rtol=2e-7, atol=0)
    assert (got["mse"][:, 0] == 0).all()
    np.testing.assert_allclose(got["metrics"].cpu().numpy(), _metrics_np(tm), rtol=2e-7, atol=0)
    np.testing.assert_allclose(got["metrics_classical"].cpu().numpy(), _metrics_np(tc), rtol=2e-7, atol=0)


def _direct(model, base, s0, T, alias=False, traj=True, metrics=True, mse=True, mcl=True, ws_short=0):
    """The C entry point on buffers with a guard row on either side of every
    output; returns the outputs' interiors after checking the guards."""
    import hybridflux as hf
    from hybridflux import engine
    from hybridflux._lib import check, lib, ptr
    B, _, nx = s0.shape
    grid = base.grid
    plan = grid.on(s0.device)[1]

    def buf(*shape):
        return torch.full((B + 2,) + shape, GUARD, device=DEV)

    state = buf(3, nx)
    state[1:B + 1] = s0
    fin = state if alias else buf(3, nx)
    tr = buf(T + 1, 3, nx) if traj else None
    me = buf(T + 1, 4) if metrics else None
    ms = buf(T + 1, 3) if mse else None
    mc = buf(T + 1, 4) if mcl else None
    pure = isinstance(model, hf.PureGNN)
    if pure:
        nb = int(lib().hf_pure_gnn_score_workspace_bytes(model.hidden_dim, B, nx, T))
    else:
        nb = int(lib().hf_pinn_score_workspace_bytes(model.input_dim, model.hidden_dim, B, T))
    assert nb >= 0
    ws = torch.full((nb + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    p = lambda t: ptr(t[1:B + 1]) if t is not None else None  # noqa: E731
    flat = model._flat.get(model, s0.device)
    tail = (grid.c32, grid.dt32, grid.nu32, grid.dx2_32, p(tr), p(me), p(ms), p(mc), ptr(ws[256:]), nb - ws_short,
            engine.stream_of(s0.device))
    with torch.cuda.device(s0.device):
        if pure:
            xd = torch.as_tensor(base.x, dtype=torch.float32, device=DEV)
            check(lib().hf_pure_gnn_run_scored(ptr(flat), model.hidden_dim, model.num_layers, p(state), p(fin), ptr(xd),
                                               ptr(plan), grid.pmode, B, nx, T, *tail))
        else:
            check(lib().hf_pinn_run_scored(ptr(flat), model.input_dim, model.hidden_dim, model.num_layers, p(state),
                                           p(fin), ptr(plan), grid.pmode, B, T, *tail))
    torch.cuda.synchronize()
    for name, t in (("final", fin), ("traj", tr), ("metrics", me), ("mse", ms), ("metrics_classical", mc)):
        if t is not None:
            assert (t[0] == GUARD).all() and (t[B + 1] == GUARD).all(), f"{name}: guard row written"
    if not alias:
        eq(state[1:B + 1], s0, "state0 changed")
    assert (ws[:256] == 0x5A).all() and (ws[256 + nb:] == 0x5A).all(), "workspace overrun"
    cut = lambda t: t[1:B + 1].clone() if t is not None else None  # noqa: E731
    return {"final": cut(fin), "traj": cut(tr), "metrics": cut(me), "mse": cut(ms), "metrics_classical": cut(mc)}


def _both_ways(model, base, s0):
    for T in STEPS:
        got = _rollout(model, base, s0, T, metrics=True, compare=base)
        assert set(got) == {"final", "traj", "metrics", "mse", "metrics_classical"}
        _check_scored(model, base, s0, T, got)
        d = _direct(model, base, s0, T)
        for k in got:
            eq(d[k], got[k], f"direct {k}")


@pytest.mark.parametrize("H,nx,L,B", PURE_FUSED + PURE_UNFUSED)
def test_pure_gnn_scored_equals_recorded_path(H, nx, L, B):
    import hybridflux as hf
    _both_ways(_pure(H, L), hf.BaselineSolver(nx, device=DEV), _ics(nx, B))


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("B", [1, 17, 33])
def test_pinn_scored_equals_recorded_path(L, B):
    """B = 17, 33 leave a partial last workgroup: its missing ICs write no series row (guards)."""
    import hybridflux as hf
    _both_ways(_pinn(192, 256, L), hf.BaselineSolver(64, device=DEV), _ics(64, B))


def test_pinn_unfused_scored_equals_recorded_path():
    import hybridflux as hf
    _both_ways(_pinn(48, 32, 3), hf.BaselineSolver(16, device=DEV), _ics(16, 3))


@pytest.mark.parametrize("which", ["pure_gnn", "pinn"])
def test_tridiagonal_twin(which):
    import hybridflux as hf
    base = hf.BaselineSolver(64, device=DEV, poisson="tridiagonal")
    model = _pure(128, 2) if which == "pure_gnn" else _pinn(192, 256, 3)
    s0 = _ics(64, 3)
    for T in STEPS:
        _check_scored(model, base, s0, T, _rollout(model, base, s0, T, metrics=True, compare=base))


@pytest.fixture(scope="module")
def ref_models():
    """The reference's checkpoints and trajectories (tests/golden/baselines.npz)."""
    import hybridflux as hf
    b = golden("baselines.npz")
    pg = hf.PureGNN(4, 128, 4)
    pg.load_state_dict({k[9:]: torch.from_numpy(b[k]) for k in b.files if k.startswith("pure_gnn.")})
    pn = hf.PINN(3 * 64, 256, 4)
    pn.load_state_dict({k[5:]: torch.from_numpy(b[k]) for k in b.files if k.startswith("pinn.")})
    return hf, pg.to(DEV), pn.to(DEV), b


@pytest.mark.parametrize("which", ["pure_gnn", "pinn"])
def test_scores_vs_reference_trajectories(ref_models, which):
    """The reference's own trajectories (seeds 1000-1003, T = 10) scored in
    float64 against the oracle's classical rollout of the same ICs, and
    evaluate_model_on_ic's number (evaluate_multi_ic.py:88-94)."""
    hf, pg, pn, b = ref_models
    from hybridflux import evaluation
    base = hf.BaselineSolver(64, device=DEV)
    ics, T = b["ics"], 10
    grid = O.Grid(64)
    gold = b[f"{which}_traj"].astype(np.float64)
    cl = O.classical_run(grid, ics, T)[0].astype(np.float64)                 # batched: [B,T+1,3,nx]
    ref = ((gold - cl) ** 2).mean(-1)                                        # [B,T+1,3]
    eps = 1e-5 * (1.0 + np.abs(gold).max(-1))
    bound = 2 * np.sqrt(ref) * eps + eps ** 2 + 2e-7 * ref
    roll = evaluation.ModelRollout(pg if which == "pure_gnn" else pn, base)
    mean_mse, r, _ = evaluation.multi_ic_mse(roll, ics, T)
    got = r["mse"].cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    print(f"{which}: max |mse - ref| / bound = {(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    want = ref.sum(-1).mean(-1)                                               # mean over time of mse_total
    lim = bound.sum(-1).mean(-1) + 4e-7 * want                                # + the float32 sums of the summary
    assert (np.abs(mean_mse.cpu().numpy() - want) <= lim).all()


@pytest.mark.parametrize("which", ["pure_gnn", "pinn"])
def test_non_finite_ics(which):
    """An IC with one inf cell and one with a NaN: the finite flag is 0 from row
    0, field 3 is NaN, the series are the recorded path's, and long_rollout
    reports what rollout_summary gives for the recorded series."""
    import hybridflux as hf
    from hybridflux import engine, evaluation
    base = hf.BaselineSolver(64, device=DEV)
    model = _pure(128, 4) if which == "pure_gnn" else _pinn(192, 256, 4)
    s0 = _ics(64, 4)
    s0[1, 0, 5] = float("inf")
    s0[2, 1, 7] = float("nan")
    T = 5
    got = _rollout(model, base, s0, T, metrics=True, compare=base)
    plain = _rollout(model, base, s0, T)
    cl = base.run_batch(s0, T, traj=True, metrics=True)
    want_m = engine.traj_metrics(plain["traj"])
    eq(got["traj"], plain["traj"], "traj")
    eq(got["metrics"], want_m, "metrics")
    eq(got["metrics_classical"], cl["metrics"], "metrics_classical")
    eq(got["mse"], engine.traj_mse(plain["traj"], cl["traj"]), "mse")
    m = got["metrics"].cpu().numpy()
    assert (m[[1, 2], :, 2] == 0).all() and np.isnan(m[[1, 2], :, 3]).all()
    assert (m[[0, 3], :, 2] == 1).all() and np.isfinite(m[[0, 3]]).all()
    d = evaluation.long_rollout(evaluation.ModelRollout(model, base), s0, T)
    summ = evaluation.summary_dict(engine.rollout_summary(want_m)[0])
    eq(d["exploded_at"], summ["exploded_at"], "exploded_at")
    eq(d["actual_steps"], summ["actual_steps"], "actual_steps")
    assert d["exploded"].tolist() == [False, True, True, False]
    eq(d["metrics"], want_m, "long_rollout metrics")


@pytest.mark.parametrize("which", ["pure_gnn", "pinn", "pure_gnn_unfused"])
def test_partial_requests(which):
    """Only metrics: no twin (mse None); only compare: no model metrics."""
    import hybridflux as hf
    nx = 20 if which == "pure_gnn_unfused" else 64
    base = hf.BaselineSolver(nx, device=DEV)
    model = {"pure_gnn": lambda: _pure(64, 2), "pinn": lambda: _pinn(192, 256, 2),
             "pure_gnn_unfused": lambda: _pure(64, 2)}[which]()
    s0, T = _ics(nx, 3), 5
    full = _rollout(model, base, s0, T, metrics=True, compare=base)
    m = _rollout(model, base, s0, T, traj=False, metrics=True)
    assert m["mse"] is None and m["metrics_classical"] is None and m["traj"] is None
    eq(m["metrics"], full["metrics"], "metrics only")
    eq(m["final"], full["final"], "final")
    c = _rollout(model, base, s0, T, traj=False, compare=base)
    assert c["metrics"] is None and c["metrics_classical"] is None
    eq(c["mse"], full["mse"], "compare only")
    plain = _rollout(model, base, s0, T, traj=False)
    assert set(plain) == {"final", "traj"}                 # the defaults are the unscored call
    d = _direct(model, base, s0, T, traj=False, metrics=False, mcl=False)
    eq(d["mse"], full["mse"], "direct, mse only")


@pytest.mark.parametrize("which", ["pure_gnn", "pinn", "pinn_unfused", "pure_gnn_unfused"])
def test_aliasing_batch_invariance_and_refusals(which):
    import hybridflux as hf
    from hybridflux._lib import HF_EINVAL, HybridFluxError
    nx = {"pure_gnn": 48, "pinn": 64, "pinn_unfused": 16, "pure_gnn_unfused": 20}[which]
    base = hf.BaselineSolver(nx, device=DEV)
    model = {"pure_gnn": lambda: _pure(64, 2), "pinn": lambda: _pinn(192, 256, 3),
             "pinn_unfused": lambda: _pinn(48, 32, 3), "pure_gnn_unfused": lambda: _pure(64, 2)}[which]()
    s0, T = _ics(nx, 3), 5
    full = _rollout(model, base, s0, T, metrics=True, compare=base)
    a = _direct(model, base, s0, T, alias=True)              # state_final aliases state0
    for k in full:
        eq(a[k], full[k], f"alias {k}")
    one = _rollout(model, base, s0[1:2], T, metrics=True, compare=base)
    for k in full:
        eq(one[k][0], full[k][1], f"alone {k}")
    # nothing to score; the twin's metrics without the twin; a workspace one byte short
    for kw in ({"metrics": False, "mse": False, "mcl": False}, {"mse": False}, {"ws_short": 1}):
        with pytest.raises(HybridFluxError) as e:
            _direct(model, base, s0, T, **kw)
        assert e.value.code == HF_EINVAL, kw


def test_python_refusals():
    import hybridflux as hf
    from hybridflux._lib import HF_EINVAL, HybridFluxError
    base = hf.BaselineSolver(16, device=DEV)
    with pytest.raises(HybridFluxError) as e:                # PINN: dim % 3 != 0
        hf.PINN(50, 32, 3).to(DEV).rollout(torch.zeros(2, 50, device=DEV), 2, metrics=True)
    assert e.value.code == HF_EINVAL
    with pytest.raises(ValueError):                          # PureGNN: [n,u,E,x] node features only
        hf.PureGNN(5, 64, 1).to(DEV).rollout(_ics(16, 1), 2, base.x, metrics=True)
    with pytest.raises(ValueError):                          # the twin's grid must be the states'
        _pure(64, 1).rollout(_ics(32, 1), 2, hf.BaselineSolver(32, device=DEV).x, compare=base)
    from hybridflux import evaluation
    with pytest.raises(ValueError):                          # no face flux
        evaluation.ModelRollout(_pure(64, 1), base).run_batch(_ics(16, 1), 2, flux=True)


def test_three_model_types_in_one_call(ref_models):
    """multi_ic_mse, long_rollout, gather_rollout and compare_models on a hybrid
    solver, a PureGNN and a PINN; the hybrid's entry is multi_ic_mse(solver)'s."""
    hf, pg, pn, b = ref_models
    import os
    from conftest import GOLDEN
    from hybridflux import engine, evaluation, rollout
    solver = hf.HybridSolver(os.path.join(GOLDEN, "weights_W1_r1.npz"), radius=1, device=DEV)
    base = solver.baseline
    models = {"hybrid": solver, "pure_gnn": evaluation.ModelRollout(pg, base), "pinn": evaluation.ModelRollout(pn, base)}
    ics, T = torch.as_tensor(b["ics"], device=DEV), 10
    res = evaluation.compare_models(models, ics, T)
    assert list(res) == list(models)
    for name, m in models.items():
        mean_mse, r, d = evaluation.multi_ic_mse(m, ics, T)
        per_ic = mean_mse.cpu().numpy()
        assert res[name]["mse_per_ic"] == [float(v) for v in per_ic]            # the same bits
        assert res[name]["mean_mse"] == float(np.mean(per_ic.astype(np.float64)))
        assert res[name]["std_mse"] == float(np.std(per_ic.astype(np.float64)))
        assert set(r) == {"final", "mse", "metrics", "metrics_classical"}
        lr = evaluation.long_rollout(m, ics, T)
        eq(lr["metrics"], r["metrics"], f"{name} long_rollout metrics")
        assert not lr["exploded"].any() and (lr["actual_steps"] == T).all()
        g = rollout.gather_rollout(r, ics.shape[0])
        eq(g["summary"][:, 5], mean_mse, f"{name} gathered mean_mse")
        eq(g["mse"], r["mse"], f"{name} gathered mse")
    # every model is scored against the same classical rollout
    eq(evaluation.multi_ic_mse(models["pure_gnn"], ics, T)[1]["metrics_classical"],
       evaluation.multi_ic_mse(solver, ics, T)[1]["metrics_classical"], "classical twin")
    # the recorded-trajectory composition gives the same per-IC numbers
    tr = pg.rollout(ics, T, base.x)["traj"]
    cl = base.run_batch(ics, T, traj=True)["traj"]
    summ, _ = engine.rollout_summary(engine.traj_metrics(tr), engine.traj_mse(tr, cl))
    assert res["pure_gnn"]["mse_per_ic"] == [float(v) for v in summ[:, 5].cpu().numpy()]
