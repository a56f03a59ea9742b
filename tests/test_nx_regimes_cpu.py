"""tests/nx_regimes.py against the sources and against itself, and the float64
references test_gpu_nx_regimes.py introduces against the ones the suite
already trusts.  No GPU.

  boundaries ........ the table's constants equal kFvLdsMaxNx, kFftMinNx, kFftMaxNx,
      kLossFusedMaxNx, kPuTile (and kFvSmallMaxNx, kFftWaves) as csrc/ defines them: a
      moved threshold fails here until the table, and the sizes around it, move too
  straddling ........ every boundary has a case on each side; the far side of the LDS
      limit is a refusal, which the CPU ABI tests cover (nx = 6145)
  poisson_t ......... the torch FFT solve the wide references use equals the oracle's
      solve (to the oracle's float32 output) and a dense product with the engine's
      circulant column (atol 1e-12) at nx = 2048 and 6144
  ablation_terms64 .. the float64 restatement from flux_edge equals O.ablation_loss per
      sample at nx = 16 for every ABLATION_CONFIGS entry (all have rollout_steps <= 3)
"""
import os
import re

import numpy as np
import pytest
import torch

import nx_regimes as N
import pinn_unroll_ref as R
from conftest import PKG_DIR, rand_sd
from oracle import hybrid_oracle as O

CSRC = os.path.join(PKG_DIR, "csrc")


def constant(name):
    """The value of `constexpr int <name> = <integer>;` in csrc/, which must define it once."""
    found = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".hip", ".cpp")):
            with open(os.path.join(CSRC, f)) as fh:
                found += re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, fh.read())
    assert len(found) == 1, (name, found)
    return int(found[0])


@pytest.mark.parametrize("name,value", [("kFvLdsMaxNx", N.FV_LDS_MAX_NX), ("kFftMinNx", N.FFT_MIN_NX),
                                        ("kFftMaxNx", N.FFT_MAX_NX), ("kLossFusedMaxNx", N.LOSS_FUSED_MAX_NX),
                                        ("kPuTile", N.PURE_TILE), ("kFvSmallMaxNx", N.SMALL_MAX_NX),
                                        ("kFftWaves", N.FFT_WAVES)])
def test_boundaries_match_the_sources(name, value):
    assert constant(name) == value


def test_fft_sizes_are_the_dispatched_ones():
    """FFT_SIZES is what poisson_uses_fft accepts, and each has a `case N:` arm in both unroll launchers."""
    assert tuple(nx for nx in range(1, 3 * N.FFT_MAX_NX) if N.uses_fft(nx)) == N.FFT_SIZES
    with open(os.path.join(CSRC, "unroll.hip")) as fh:
        src = fh.read()
    for nx in N.FFT_SIZES:
        assert len(re.findall(r"case %d: return update_fft_launch<%d>" % (nx, nx), src)) == 1
        assert len(re.findall(r"case %d: return adjoint_fft_launch<%d>" % (nx, nx), src)) == 1
    assert not re.search(r"case (?!256|512|1024|2048)\d+: return (update|adjoint)_fft_launch", src)


def test_every_boundary_is_straddled():
    import test_gpu_pure_unrolled_training as P
    import test_gpu_unrolled_training as U
    unroll = set(U.SHAPES) | set(N.UNROLL_WIDE)
    nxs = {nx for nx, _ in unroll}
    # FFT sizes: each one, the size just past the first, a non-power of two between two of
    # them, a power of two past the last
    assert set(N.FFT_SIZES) <= nxs and N.FFT_MIN_NX + 1 in nxs
    assert any(N.FFT_MIN_NX < nx < N.FFT_MAX_NX and not N.uses_fft(nx) for nx in nxs)
    assert any(nx > N.FFT_MAX_NX and nx & (nx - 1) == 0 for nx in nxs)
    assert any(nx < N.FFT_MIN_NX for nx in nxs)
    # a pair of ICs per wave, FFT_WAVES pairs per workgroup: a lone IC, an odd count, one
    # IC past a workgroup; the 2048 kernel (one workgroup per CU) with two workgroups
    per_wg = 2 * N.FFT_WAVES
    fft_B = {B for nx, B in unroll if N.uses_fft(nx)}
    assert 1 in fft_B and per_wg + 1 in fft_B and any(B % 2 for B in fft_B - {1, per_wg + 1})
    assert (N.FFT_MAX_NX, per_wg + 1) in unroll
    # the LDS limit: reached by every circulant training kernel's cases; refused beyond
    # (test_abi_unroll_cpu.py, test_abi_pinn_train_cpu.py, test_abi_pinn_unroll_cpu.py: 6145)
    assert N.FV_LDS_MAX_NX in nxs and N.FV_LDS_MAX_NX in N.PINN_WIDE and max(nxs) == N.FV_LDS_MAX_NX
    assert N.FV_LDS_MAX_NX in {nx for nx, _ in N.UPDATE_BITWISE_WIDE}
    assert N.FV_LDS_MAX_NX in {nx for nx, _ in N.UNROLLED_GRAD_WIDE}
    assert set(N.FFT_SIZES[1:]) <= {nx for nx, _ in N.UPDATE_BITWISE_WIDE}
    assert any(N.uses_fft(nx) for nx, _ in N.UNROLLED_GRAD_WIDE)
    # the ablation loss: one launch up to LOSS_FUSED_MAX_NX except at FFT sizes, then
    # poisson_kernel up to the LDS limit, poisson_tiled_kernel beyond
    one_launch = [nx for nx in N.LOSS_WIDE if not N.uses_fft(nx) and nx <= N.LOSS_FUSED_MAX_NX]
    assert N.uses_fft(N.LOSS_FUSED_MAX_NX) and max(one_launch) == N.LOSS_FUSED_MAX_NX - 1
    assert N.LOSS_FUSED_MAX_NX + 1 in N.LOSS_WIDE and N.FV_LDS_MAX_NX in N.LOSS_WIDE
    assert any(nx > N.FV_LDS_MAX_NX for nx in N.LOSS_WIDE)
    assert set(N.FFT_SIZES[1:]) <= set(N.LOSS_WIDE)
    assert any(N.uses_fft(nx) for nx in N.LOSS_WIDE_FULL) and any(not N.uses_fft(nx) for nx in N.LOSS_WIDE_FULL)
    assert all(N.uses_fft(nx) or nx > N.LOSS_FUSED_MAX_NX for nx in N.LOSS_WIDE_FULL)  # three launches
    # PureGNN tiles: one whole tile, a few cells and one cell into the next, several tiles
    pure = {nx for nx, _ in P.SHAPES}
    assert {N.PURE_TILE, 2 * N.PURE_TILE + 1} <= pure and any(N.PURE_TILE < nx < 2 * N.PURE_TILE for nx in pure)
    assert any(nx % N.PURE_TILE == 0 and nx > 2 * N.PURE_TILE for nx in pure)
    # the time step: the reference's up to SMALL_MAX_NX, the same dt / dx beyond
    assert N.dt_of(N.SMALL_MAX_NX) == 5e-3 and N.dt_of(1) == 5e-3
    for nx in N.all_sizes():
        assert abs(N.dt_of(nx) * nx - 5e-3 * 64) <= 1e-15


@pytest.mark.parametrize("nx", [2048, 6144])
def test_poisson_t_vs_oracle_and_dense_circulant(nx):
    from test_gpu_unrolled_training import poisson_t
    G = O.Grid(nx, dt=N.dt_of(nx))
    g = np.random.default_rng(nx)
    n = 1.0 + 0.3 * np.sin(3 * G.x + 0.5) + 0.1 * g.standard_normal((3, nx))  # float64
    got = poisson_t(torch.as_tensor(n), torch.as_tensor(G.k)).numpy()
    assert got.dtype == np.float64
    # the oracle on the same float64 densities: its own float64 FFT, rounded to float32 once
    want32 = O.solve_poisson(G, n)
    assert np.abs(got - want32).max() <= 2.0 ** -24 * np.abs(got).max()
    # the dense product with the engine's column: M[i][j] = col[(i - j) mod nx]
    col = R.poisson_column(nx, G.length)
    rr = np.concatenate([col[::-1], col[::-1]])
    M = np.lib.stride_tricks.sliding_window_view(rr, nx)[:nx][::-1]
    assert M[5, 2] == col[3] and M[2, 5] == col[nx - 3] and M[0, 0] == col[0]
    dense = (n - 1.0) @ np.ascontiguousarray(M).T
    assert np.abs(got - dense).max() <= 1e-12


def _sample16(seed):
    G = O.Grid(16)
    st = O.initial_condition(G, seed)
    S, F = O.classical_run(G, st[None], 3)
    return G, S[0, 2], F[0, 2], S[0, 3]


def test_ablation_terms64_vs_oracle_per_sample():
    """ablation_terms64 on the edge fluxes of O.flux_gnn_forward equals O.ablation_loss
    (the reference's float32 per-sample loss, model forwards in its rollout loop
    included) for every configuration, on three samples: loss and flux loss to rtol
    1e-5 (the oracle is float32: means of 16 squares of float32 differences, a few
    ulp each, against a gate of 80 ulp)."""
    import hybridflux
    from test_gpu_nx_regimes import ablation_terms64
    sd = rand_sd(2, 3)
    p = O.params_from(sd)
    assert all(c["rollout_steps"] <= 3 for c in hybridflux.ABLATION_CONFIGS.values())
    for name, cfg in hybridflux.ABLATION_CONFIGS.items():
        for seed in (1, 2, 3):
            G, st, ft, sn = _sample16(seed)
            with torch.no_grad():
                want, want_f = O.ablation_loss(p, G, st, ft, sn, cfg)
                fe = O.flux_gnn_forward(p, O.node_features(G, st[None]), O.chain_edges(16, 1)).double()[None]
            got, got_f = ablation_terms64(fe, st[None], ft[None], sn[None], G.dt / G.dx, G.dt, G.dx, G.k, cfg)
            assert abs(float(got[0]) - float(want)) <= 1e-5 * abs(float(want)), (name, seed)
            assert abs(float(got_f[0]) - float(want_f)) <= 1e-5 * abs(float(want_f)), (name, seed)


def test_ablation_terms64_terms_are_all_there():
    """Each lambda changes the restated loss (no term silently dropped), and the batch
    form is per sample: two samples stacked give the two single values."""
    import hybridflux
    from test_gpu_nx_regimes import ablation_terms64
    full = hybridflux.ABLATION_CONFIGS["full"]
    G, st, ft, sn = _sample16(4)
    g = np.random.default_rng(0)
    fe = torch.as_tensor(g.normal(0, 0.1, (1, 32)))
    args = (st[None], ft[None], sn[None] + 0.01, G.dt / G.dx, G.dt, G.dx, G.k)
    base = float(ablation_terms64(fe, *args, full)[0])
    for key in ("lambda_state", "lambda_poisson", "lambda_energy_one", "lambda_energy_multi"):
        assert float(ablation_terms64(fe, *args, dict(full, **{key: 0.0}))[0]) < base, key
    G2, st2, ft2, sn2 = _sample16(5)
    fe2 = torch.as_tensor(g.normal(0, 0.1, (1, 32)))
    both, _ = ablation_terms64(torch.cat([fe, fe2]), np.stack([st, st2]), np.stack([ft, ft2]),
                               np.stack([sn + 0.01, sn2]), G.dt / G.dx, G.dt, G.dx, G.k, full)
    one2 = float(ablation_terms64(fe2, st2[None], ft2[None], sn2[None], G.dt / G.dx, G.dt, G.dx, G.k, full)[0])
    assert float(both[0]) == pytest.approx(base, rel=1e-14) and float(both[1]) == pytest.approx(one2, rel=1e-14)
