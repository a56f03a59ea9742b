"""Coarse-grained fine classical rollouts on the device (include/hybridflux.h:
hf_coarsen_traj, hf_run_coarse) and the Python layer on top (FineReference,
datagen's refine / substeps, evaluation.compare_to_fine).

* hf_coarsen_traj on hf_run's own fine trajectory and flux equals the numpy
  restatement (tests/coarse_ref.py) bit for bit;
* hf_run_coarse (the one-launch kernels at nx_f <= 64 and nx_f in {256, 512,
  1024}, the chunked sequencing elsewhere) equals hf_coarsen_traj(hf_run) bit
  for bit, for every output on its own, both Poisson modes, any chunking;
* a rollout continued from the returned fine state equals one long rollout;
* the time-averaged flux drives the hybrid update to the next coarse density
  within the CPU test's bound.
"""
import numpy as np
import pytest
import torch

import coarse_ref as CR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def setup(nx_f, B, S, poisson="spectral"):
    """(fine engine grid, fine ICs [B,3,nx_f]) at a step that keeps a few steps finite at every nx_f."""
    import hybridflux
    from hybridflux import engine
    dt_f = 5e-3 * 64.0 / max(nx_f, 64) / S
    grid = engine.Grid(nx_f, dt=dt_f, poisson=poisson)
    ics = hybridflux.BaselineSolver(nx_f, dt=dt_f, device=DEV, poisson=poisson).initial_conditions(
        range(1000, 1000 + B), as_tensor=True)
    return engine, grid, ics


def definition(engine, grid, ics, T_c, r, S):
    """hf_coarsen_traj(hf_run(traj, flux)) and hf_run's final fine state."""
    f = engine.run(None, grid, ics, T_c * S, traj=True, flux=True)
    tc, fc = engine.coarsen_traj(f["traj"], f["flux"], r, S)
    return f, tc, fc


@pytest.mark.parametrize("nx_f,r,S,T_c,B", [(64, 4, 4, 2, 5), (48, 4, 3, 2, 3), (256, 64, 3, 2, 3), (1024, 16, 2, 1, 3),
                                            (96, 2, 3, 2, 3), (100, 1, 2, 2, 2), (2048, 32, 1, 1, 2)])
def test_coarsen_traj_is_the_definition(nx_f, r, S, T_c, B):
    engine, grid, ics = setup(nx_f, B, S)
    f, tc, fc = definition(engine, grid, ics, T_c, r, S)
    want_t, want_f = CR.coarsen(f["traj"].cpu().numpy(), f["flux"].cpu().numpy(), r, S)
    assert np.isfinite(want_t).all()
    assert same_bits(tc, want_t) and same_bits(fc, want_f)
    tc_only, none = engine.coarsen_traj(f["traj"], None, r, S)
    assert none is None and same_bits(tc_only, want_t)
    if r == 1:
        assert same_bits(tc, f["traj"][:, ::S])


def check_fused(nx_f, r, S, T_c, B, poisson="spectral", ws=None):
    engine, grid, ics = setup(nx_f, B, S, poisson)
    f, tc, fc = definition(engine, grid, ics, T_c, r, S)
    got = engine.run_coarse(grid, ics, T_c, r, S, traj=True, flux=True, final=True, ws=ws)
    what = (nx_f, r, S, T_c, B, poisson)
    assert torch.isfinite(tc).all(), what
    assert same_bits(got["traj"], tc), what
    assert same_bits(got["flux"], fc), what
    assert same_bits(got["final_fine"], f["final"]), what
    return engine, grid, ics, f, tc, fc


@pytest.mark.parametrize("nx_f,r", [(256, 2), (256, 64), (512, 8), (1024, 16), (1024, 1)])
def test_fft_kernel_equals_definition(nx_f, r):
    """B = 3: the unpaired last wave; B = 9: a second workgroup."""
    for B in (3, 9):
        for S in (1, 3):
            for T_c in (0, 2):
                check_fused(nx_f, r, S, T_c, B)


@pytest.mark.parametrize("nx_f,r", [(64, 1), (64, 4), (48, 4), (16, 16)])
def test_small_kernel_equals_definition(nx_f, r):
    """B = 5: a second workgroup (4 waves each)."""
    for T_c in (0, 2):
        check_fused(nx_f, r, 4, T_c, 5)


@pytest.mark.parametrize("nx_f,r", [(128, 2), (96, 2)])
def test_chunked_path_does_not_depend_on_the_chunking(nx_f, r):
    B, S, T_c = 3, 3, 3
    from hybridflux import engine
    one = engine.run_coarse_workspace(B, nx_f, 1, r, S)
    two = engine.run_coarse_workspace(B, nx_f, 2, r, S)
    full = engine.run_coarse_workspace(B, nx_f, T_c, r, S)
    assert 0 < one < two < full
    for nbytes in (one, two, full, full + 4096):  # 3 chunks of 1, chunks of 2 + 1, one chunk, a larger workspace
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        check_fused(nx_f, r, S, T_c, B, ws=ws)
    check_fused(nx_f, r, S, T_c, B)  # the engine's own workspace
    check_fused(nx_f, r, S, 0, B)
    _, grid, ics = setup(nx_f, B, S)
    with pytest.raises(Exception, match="workspace"):
        engine.run_coarse(grid, ics, T_c, r, S, ws=torch.empty(one - 1, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("nx_f,r", [(256, 2), (64, 4), (128, 2)])
def test_tridiagonal_mode(nx_f, r):
    check_fused(nx_f, r, 3, 2, 3, poisson="tridiagonal")


@pytest.mark.parametrize("nx_f,r", [(256, 2), (1024, 16), (64, 4), (128, 2)])
def test_each_output_on_its_own(nx_f, r):
    B, S, T_c = 3, 3, 2
    engine, grid, ics, f, tc, fc = check_fused(nx_f, r, S, T_c, B)
    a = engine.run_coarse(grid, ics, T_c, r, S, traj=True, flux=False, final=False)
    assert a["flux"] is None and a["final_fine"] is None and same_bits(a["traj"], tc)
    a = engine.run_coarse(grid, ics, T_c, r, S, traj=False, flux=True, final=False)
    assert a["traj"] is None and a["final_fine"] is None and same_bits(a["flux"], fc)
    a = engine.run_coarse(grid, ics, T_c, r, S, traj=False, flux=False, final=True)
    assert a["traj"] is None and a["flux"] is None and same_bits(a["final_fine"], f["final"])
    with pytest.raises(ValueError):
        engine.run_coarse(grid, ics, T_c, r, S, traj=False, flux=False, final=False)


@pytest.mark.parametrize("nx_f,r", [(256, 4), (64, 4), (128, 2)])
def test_continuation(nx_f, r):
    B, S, a, b = 3, 2, 1, 2
    engine, grid, ics = setup(nx_f, B, S)
    whole = engine.run_coarse(grid, ics, a + b, r, S, traj=True, flux=True, final=True)
    first = engine.run_coarse(grid, ics, a, r, S, traj=True, flux=True, final=True)
    second = engine.run_coarse(grid, first["final_fine"], b, r, S, traj=True, flux=True, final=True)
    assert same_bits(first["traj"], whole["traj"][:, :a + 1]) and same_bits(second["traj"], whole["traj"][:, a:])
    assert same_bits(first["flux"], whole["flux"][:, :a]) and same_bits(second["flux"], whole["flux"][:, a:])
    assert same_bits(second["final_fine"], whole["final_fine"])


def test_time_averaged_flux_drives_the_hybrid_update():
    """Fbar as both edge directions of flux_edge: hf_unroll_update's n' on the
    coarse grid is nbar_{t+1} within the coarse continuity identity's bound."""
    import hybridflux
    from hybridflux import engine
    B, nx, r, S, T_c = 3, 16, 4, 4, 2
    ref = hybridflux.FineReference(nx=nx, refine=r, substeps=S, device=DEV, E="solve")
    s0 = ref.initial_conditions(range(B))
    fine = engine.run(None, ref.fine.grid, s0, T_c * S, traj=True, flux=True)
    R = ref.run_batch(s0, T_c, traj=True, flux=True)
    gf = CR.grids(nx, r, S)[1]
    bound = CR.continuity_bound(fine["traj"].cpu().numpy(), fine["flux"].cpu().numpy(), gf, S)
    for t in range(T_c):
        Fbar = R["flux"][:, t]
        fe = torch.cat([Fbar, Fbar], dim=1).contiguous().reshape(-1)
        nxt, _, _ = engine.unroll_update(ref.coarse.grid, fe, R["traj"][:, t].contiguous(), want_nf=False)
        err = float((nxt[:, 0].double() - R["traj"][:, t + 1, 0].double()).abs().max())
        print(f"step {t}: |n' - nbar'| = {err:.3e} = {err / bound:.3f} of the bound {bound:.3e}")
        assert err <= bound


def test_fine_reference_E_options():
    import hybridflux
    from hybridflux import engine
    B, nx, r, S, T_c = 3, 64, 4, 2, 2
    solve = hybridflux.FineReference(nx=nx, refine=r, substeps=S, device=DEV, E="solve")
    filt = hybridflux.FineReference(nx=nx, refine=r, substeps=S, device=DEV, E="filtered")
    s0 = solve.initial_conditions(range(B))
    a, b = solve.run_batch(s0, T_c), filt.run_batch(s0, T_c)
    assert a["flux"] is None and a["final_fine"] is None
    assert same_bits(a["traj"][:, :, :2], b["traj"][:, :, :2])
    want = engine.poisson(solve.coarse.grid, b["traj"][:, :, 0].reshape(-1, nx)).reshape(B, T_c + 1, nx)
    assert same_bits(a["traj"][:, :, 2], want)
    d = float((a["traj"][:, :, 2] - b["traj"][:, :, 2]).abs().max())
    assert 0 < d < 0.1
    assert same_bits(solve.restrict(s0), a["traj"][:, 0]) and same_bits(filt.restrict(s0), b["traj"][:, 0])
    # the oracle's coarse-grained rollout from the same fine ICs (another FFT, another summation order in E)
    O = CR.fine_reference(nx, r, S, T_c, range(B), E="solve")
    assert np.abs(a["traj"].cpu().numpy() - O["traj"]).max() < 1e-5


def test_generate_trajectories_from_the_fine_reference():
    import hybridflux
    from hybridflux import datagen
    tr = datagen.generate_trajectories(nx=16, refine=4, substeps=2, num_initial_conditions=3, steps_per_ic=3, device=DEV)
    assert tr.shape == (3, 4, 3, 16) and tr.dtype == np.float32
    ref = hybridflux.FineReference(nx=16, refine=4, substeps=2, device=DEV)
    R = ref.run_batch(ref.initial_conditions(range(3)), 3, traj=True, flux=True)
    assert same_bits(tr, R["traj"])
    st, ft, sn, x, dt, dx, nu = datagen.generate_dataset(nx=16, refine=4, substeps=2, num_initial_conditions=3,
                                                         steps_per_ic=3, out_path=None, device=DEV)
    assert st.shape == (9, 3, 16) and ft.shape == (9, 16) and sn.shape == (9, 3, 16)
    assert st.dtype == ft.dtype == sn.dtype == x.dtype == np.float32
    assert same_bits(st, R["traj"][:, :-1].reshape(9, 3, 16)) and same_bits(sn, R["traj"][:, 1:].reshape(9, 3, 16))
    assert same_bits(ft, R["flux"].reshape(9, 16))
    assert dt == 5e-3 and dx == ref.coarse.dx and np.array_equal(x, ref.coarse.x.astype(np.float32))


def test_compare_to_fine():
    import hybridflux
    from hybridflux import engine, evaluation
    B, nx, T = 3, 64, 4
    base = hybridflux.BaselineSolver(nx, device=DEV)
    ident = hybridflux.FineReference(nx=nx, device=DEV)
    s0 = ident.initial_conditions(range(B))
    r = evaluation.compare_to_fine(base, ident, s0, T)
    assert set(r) == {"final", "mse", "metrics", "metrics_classical"}
    assert r["mse"].shape == (B, T + 1, 3) and float(r["mse"].abs().max()) == 0.0
    assert same_bits(r["metrics"], r["metrics_classical"])
    evaluation.summary_dict(engine.rollout_summary(r["metrics"], r["mse"], r["metrics_classical"])[0])
    fine = hybridflux.FineReference(nx=nx, substeps=4, device=DEV)
    r4 = evaluation.compare_to_fine(base, fine, s0, T)
    a = base.run_batch(s0, T, traj=True)["traj"]
    b = fine.run_batch(s0, T, traj=True)["traj"]
    assert float(r4["mse"][:, 1:].min()) > 0 and same_bits(r4["mse"], engine.traj_mse(a, b))
    assert float(r4["mse"][:, 0].abs().max()) == 0.0
    for bad in (hybridflux.BaselineSolver(32, device=DEV), hybridflux.BaselineSolver(nx, dt=1e-3, device=DEV),
                hybridflux.BaselineSolver(nx, length=1.0, device=DEV)):
        with pytest.raises(ValueError):
            evaluation.compare_to_fine(bad, fine, s0, T)


def test_datagen_defaults_unchanged():
    """generate_dataset's defaults still produce hf_run's bits."""
    import hybridflux
    from hybridflux import datagen, engine
    N, T, nx = 4, 5, 64
    st, ft, sn, x, dt, dx, nu = datagen.generate_dataset(num_initial_conditions=N, steps_per_ic=T, out_path=None,
                                                         device=DEV)
    base = hybridflux.BaselineSolver(nx, device=DEV)
    f = engine.run(None, base.grid, base.initial_conditions(range(N), as_tensor=True), T, traj=True, flux=True)
    assert same_bits(st, f["traj"][:, :-1].reshape(N * T, 3, nx)) and same_bits(sn, f["traj"][:, 1:].reshape(N * T, 3, nx))
    assert same_bits(ft, f["flux"].reshape(N * T, nx))
    tr = datagen.generate_trajectories(num_initial_conditions=N, steps_per_ic=T, device=DEV)
    assert same_bits(tr, f["traj"])
