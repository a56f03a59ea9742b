"""The radius-R kernels away from the corner tests/test_gpu_radius.py started at.

The regime rows of tests/radius_cases.py (depths 0..8, the window-count
boundaries, the tightest window, chains shorter than a window, long chains, a
second pass of the persistent loop in the EXACT and in the windowed form,
per-step rollouts at nx = 100 / 1024) run through test_gpu_radius.py's own
parametrised tests.  This file holds what is not a row of that table; all of it
is bit for bit, there is no tolerance in this file:

  model sets      tests/test_gpu_model_set.py's grid with graph_radius = 2, 3: a set
                  of M = 3 against one single-model call per model, scored and
                  unscored, mixed depths, per-model ICs, an unfused nx, the
                  tridiagonal mode; the models differ pairwise, a permutation of
                  the models permutes the leading axis, and the radius shows
  compare_batch   = run_batch + the classical run + traj_mse, at nx = 16 and 100
  small batches   B = 3 alone = the same ICs inside B = 300 at nx = 100
  lanes           hf_run's lane streams with a radius model: ICs at the lane
                  edges alone = inside the batch, in every output
  the order       of the neighbour sum, on float32 inputs where it shows
                  (radius_cases.order_sd): the fused kernels' edges and faces,
                  FluxGNN.forward on the tagged radius graph (hf_graph_flux_radius)
                  and the float32 reference in DESIGN.md's order are the same
                  bits.  Every other sum of that forward has at most two nonzero
                  terms, which any accumulation order rounds alike; a neighbour
                  sum taken pairwise or in reverse changes 10 % to 38 % of each
                  case's fluxes (tests/test_radius_cases_cpu.py holds it to 5 %).
"""
import numpy as np
import pytest
import torch

import radius_cases as RC
from conftest import golden, rand_sd
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADII = pytest.mark.parametrize("R", [2, 3])
UNSCORED = dict(traj=True, flux=True, metrics=True)
_SOLVERS, _ICS = {}, {}


def solver(seed, R, layers=4, nx=64, poisson="spectral"):
    """HybridSolver(graph_radius=R) on rand_sd(layers, seed), shared by the tests that ask for the same one."""
    import hybridflux as hf
    key = (seed, R, layers, nx, poisson)
    if key not in _SOLVERS:
        _SOLVERS[key] = hf.HybridSolver(rand_sd(layers, seed), R, nx=nx, device=DEV, poisson=poisson,
                                        num_layers=layers, graph_radius=R)
    return _SOLVERS[key]


def trained(R, nx):
    import hybridflux as hf
    w = golden(f"weights_W1_r{R}.npz")
    return hf.HybridSolver({k: torch.from_numpy(w[k]) for k in w.files}, R, nx=nx, device=DEV, graph_radius=R)


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


# ------------------------------------------------------------------- model sets
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nx", [16, 32, 48, 64])
@RADII
def test_set_unscored(R, nx, B):
    """M = 3 from shared ICs.  A radius model never takes the cell-split kernels, so
    every nx runs the IC-per-wave rollout; B = 5 leaves each model a ragged last
    workgroup of one live wave, B = 1 a single wave per model."""
    import hybridflux as hf
    solvers = [solver(100 + i, R, nx=nx) for i in range(3)]
    s0, T = ics(nx, B), 3
    want = loop(solvers, s0, T, False, **UNSCORED)
    got = hf.HybridEnsemble(solvers).run_batch(s0, T, **UNSCORED)
    assert got["final"].shape == (3, B, 3, nx) and got["traj"].shape == (3, B, T + 1, 3, nx)
    assert got["flux"].shape == (3, B, T, nx) and got["metrics"].shape == (3, B, T + 1, 4)
    check(got, want, f"R={R} nx={nx} B={B}")
    # sharpness: the models really differ, and the leading axis follows the models' order
    for k in ("final", "traj", "flux", "metrics"):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert not torch.equal(want[k][i], want[k][j]), f"models {i} and {j} give the same {k}"
    perm = [2, 0, 1]
    gp = hf.HybridEnsemble([solvers[i] for i in perm]).run_batch(s0, T, **UNSCORED)
    for k in want:
        same(gp[k], want[k][perm], f"permuted {k}")
    # ... and the radius shows: the same weights on the +-1 chain give other fluxes, for every model
    ones = [hf.HybridSolver(rand_sd(4, 100 + i), 1, nx=nx, device=DEV, num_layers=4) for i in range(3)]
    r1 = hf.HybridEnsemble(ones).run_batch(s0, T, **UNSCORED)
    for i in range(3):
        assert not torch.equal(r1["flux"][i], got["flux"][i]) and not torch.equal(r1["final"][i], got["final"][i]), i


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nx,poisson", [(16, "spectral"), (32, "spectral"), (48, "spectral"), (64, "spectral"),
                                        (64, "tridiagonal")])
@RADII
def test_set_scored(R, nx, poisson, B):
    import hybridflux as hf
    solvers = [solver(100 + i, R, nx=nx, poisson=poisson) for i in range(3)]
    s0, T = ics(nx, B), 3
    want = loop(solvers, s0, T, True)
    got = hf.HybridEnsemble(solvers).compare_batch(s0, T)
    assert set(got) == {"final", "mse", "metrics", "metrics_classical"} and got["mse"].shape == (3, B, T + 1, 3)
    check(got, want, f"scored R={R} nx={nx} {poisson} B={B}")
    assert not torch.equal(want["mse"][0], want["mse"][1]) and not torch.equal(want["mse"][1], want["mse"][2])
    same(hf.HybridEnsemble(solvers).compare_batch(s0, T, metrics=False)["mse"], want["mse"], "mse without metrics")


@RADII
def test_set_mixed_depth(R):
    """layers (2, 4, 1) in one launch: each workgroup streams its own model's chunk count."""
    import hybridflux as hf
    solvers = [solver(200 + i, R, layers=L) for i, L in enumerate((2, 4, 1))]
    ens, s0 = hf.HybridEnsemble(solvers), ics(64, 5)
    check(ens.run_batch(s0, 3, **UNSCORED), loop(solvers, s0, 3, False, **UNSCORED), f"R={R} mixed depth")
    check(ens.compare_batch(s0, 3), loop(solvers, s0, 3, True), f"R={R} mixed depth scored")


@RADII
def test_set_ics_per_model(R):
    """states0 [M,B,3,nx] with different states per model, out of place and in place."""
    import hybridflux as hf
    solvers = [solver(100 + i, R, nx=48) for i in range(2)]
    ens = hf.HybridEnsemble(solvers)
    s0 = torch.stack([ics(48, 5), ics(48, 5, seed0=4100)])
    assert not torch.equal(s0[0], s0[1])
    for scored, kw in ((False, UNSCORED), (True, {})):
        want = loop(solvers, s0, 3, scored, **kw)
        call = ens.compare_batch if scored else ens.run_batch
        check(call(s0, 3, **kw), want, f"R={R} per-model ICs scored={scored}")
        st = s0.clone()
        got = call(st, 3, out=st, **kw)
        assert got["final"] is st
        check(got, want, f"R={R} per-model ICs in place scored={scored}")


@RADII
def test_set_unfused_nx_runs_model_after_model(R):
    import hybridflux as hf
    solvers = [solver(100 + i, R, nx=20) for i in range(2)]
    ens, s0 = hf.HybridEnsemble(solvers), ics(20, 3)
    check(ens.run_batch(s0, 3, **UNSCORED), loop(solvers, s0, 3, False, **UNSCORED), f"R={R} nx=20")
    check(ens.run_batch(s0, 3, traj=False), loop(solvers, s0, 3, False, traj=False), f"R={R} nx=20 no traj")
    check(ens.compare_batch(s0, 3), loop(solvers, s0, 3, True), f"R={R} nx=20 scored")


# ----------------------------------------------------------------- compare_batch
@pytest.mark.parametrize("nx", [16, 100])
def test_compare_batch_bitwise(nx):
    """R = 3 at the smallest fused nx (one persistent launch with the classical
    twin) and at an unfused one (per step)."""
    from hybridflux import engine
    T, B = 5, 7
    s, st = trained(3, nx), ics(nx, B, seed0=2000)
    c = s.compare_batch(st, T, metrics=True)
    r = s.run_batch(st, T, traj=True, metrics=True)
    cl = s.baseline.run_batch(st, T, traj=True, metrics=True)
    same(c["final"], r["final"], "final")
    same(c["metrics"], r["metrics"], "metrics")
    same(c["metrics_classical"], cl["metrics"], "classical metrics")
    same(c["mse"], engine.traj_mse(r["traj"], cl["traj"]), "mse")
    assert float(c["mse"][:, -1].max()) > 0


# ----------------------------------------------------------------- small batches
def test_small_batch_equals_large_batch_unfused():
    """nx = 100, R = 3 (3 windows per IC): 3 ICs are 9 items in 3 groups; inside
    B = 300 the same ICs share groups with other neighbours (900 items)."""
    s = trained(3, 100)
    st = ics(100, 300, seed0=2000)
    big = s.run_batch(st, 4, traj=True, flux=True)
    small = s.run_batch(st[:3].contiguous(), 4, traj=True, flux=True)
    same(small["traj"], big["traj"][:3].contiguous(), "traj")
    same(small["flux"], big["flux"][:3].contiguous(), "flux")
    a, Fa, _ = s.step_batch(st[:3].contiguous(), return_flux=True)
    same(a, big["traj"][:3, 1].contiguous(), "step")
    same(Fa, big["flux"][:3, 0].contiguous(), "step flux")
    assert not torch.equal(big["flux"][0], big["flux"][1])


# ------------------------------------------------------------------------ lanes
def test_run_lanes_with_a_radius_model():
    """hf_run's lanes (capi.cpp run_lanes) with a radius-2 model: 3075 ICs x 1024
    cells are 3 lanes, cut evenly for a float32 model (its flux kernel's units are
    not modelled): [0,1025) [1025,2050) [2050,3075).  ICs at the batch's ends and
    around the cuts (1023..1027 spans the first, 2048..2052 the second) run alone
    equal the batch in every output, and state0 aliasing state_final gives the
    same final state."""
    from hybridflux import engine
    dev = torch.device(DEV)
    B, nx, T = 3075, 1024, 2
    assert RC.lanes(nx, B) == (3, [0, 1025, 2050, 3075])
    grid = engine.Grid(nx, dt=3.125e-4)
    m = engine.DeviceModel(rand_sd(1, 77), dev, "f32", 2)
    G = O.Grid(nx, dt=3.125e-4)
    base = np.stack([O.initial_condition(G, s) for s in range(4000, 4004)])
    st = torch.as_tensor(np.tile(base, (B // 4 + 1, 1, 1))[:B], device=dev, dtype=torch.float32)
    st = st * (1 + 1e-3 * torch.arange(B, device=dev, dtype=torch.float32)[:, None, None] / B)
    full = engine.run(m, grid, st, T, traj=True, flux=True, metrics=True)
    for lo, hi in ((0, 3), (1023, 1027), (2048, 2052), (3072, 3075)):
        one = engine.run(m, grid, st[lo:hi].contiguous(), T, traj=True, flux=True, metrics=True)
        for k in ("final", "traj", "flux", "metrics"):
            assert torch.equal(one[k], full[k][lo:hi]), (lo, k)
    assert not torch.equal(full["final"][1023], full["final"][1027])
    one = engine.DeviceModel(rand_sd(1, 77), dev, "f32", 1)                    # the radius shows here too
    assert not torch.equal(engine.run(one, grid, st[:3].contiguous(), T)["final"], full["final"][:3])
    alias = st.clone()
    engine.run(m, grid, alias, T, traj=False, out=alias)
    assert torch.equal(alias, full["final"])


# -------------------------------------------------------- the neighbour-sum order
def _order_report(got, b, case):
    """Against which order the mismatching bits would have matched (the failure message)."""
    out = []
    for o in RC.ORDERS:
        ref = RC.forward32_order(b.sd, b.nf, case.B, case.nx, case.R, o)
        out.append(f"{o}: {float(np.mean(got != ref)):.3f}")
    return "fraction of fluxes that differ from the order " + ", ".join(out)


@pytest.mark.parametrize("case", RC.ORDER_CASES, ids=lambda c: c.name)
def test_neighbour_sum_order_bitwise(case):
    """DESIGN.md 3.20's one order, ((((h[i+1] + h[i-1]) + h[i+2]) + h[i-2]) +
    h[i+3]) + h[i-3], in the fused kernels (nx = 16, 64: nb_sum_radius in the
    EXACT form; nx = 100: in 64-cell windows) and in hf_graph_flux_radius (the
    edge list's own order), on float32 inputs where another order changes the bits."""
    import hybridflux as hf
    from hybridflux import engine
    from hybridflux.graph_constructor import chain_edge_index
    b = RC.find_order_case(case)
    B, nx, R = case.B, case.nx, case.R
    dev = torch.device(DEV)
    nf = torch.from_numpy(b.nf).to(dev)
    fe, ff = engine.chain_flux(engine.DeviceModel(b.sd, dev, "f32", R), nf, B, nx, flux_face=True)
    fused = fe.cpu().numpy().reshape(B, 2 * nx)
    m = hf.FluxGNN(4, 128, case.layers)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in b.sd.items()})
    with torch.no_grad():
        tagged = m.to(dev)(nf, chain_edge_index(nx, B, DEV, radius=R))
    assert tagged.shape == (B * 2 * R * nx,)
    tagged = tagged.cpu().numpy().reshape(B, 2 * R * nx)
    want_all = RC.forward32_order(b.sd, b.nf, B, nx, R, "fixed", all_edges=True)
    assert fused.dtype == tagged.dtype == b.flux.dtype == np.float32
    assert np.array_equal(fused, tagged[:, :2 * nx]), \
        f"fused and generic paths differ on {int((fused != tagged[:, :2 * nx]).sum())} of {fused.size} fluxes; fused: " \
        f"{_order_report(fused, b, case)}; generic: {_order_report(tagged[:, :2 * nx], b, case)}"
    assert np.array_equal(fused, b.flux), f"fused kernel: {_order_report(fused, b, case)}"
    assert np.array_equal(tagged, want_all), f"generic kernels, every edge: {int((tagged != want_all).sum())} differ"
    faces = np.float32(0.5) * (b.flux[:, :nx] + b.flux[:, nx:])
    assert faces.dtype == np.float32 and np.array_equal(ff.cpu().numpy(), faces), "face fluxes"
