"""tests/optim_cases.py against the sources and against itself.  No GPU.

  constants ... THREADS, TILE, MAX_BLOCKS equal kOptThreads, kOptTile, kOptMaxBlocks as
      csrc/ defines them: a changed grid fails here until the table follows
  straddling .. the table has a length on each side of every regime change
  sizes ....... the model sizes are the libraries' parameter counts, and the workspace
      query holds one float64 per workgroup of the table's grid
"""
import pytest

import optim_cases as C
from hybridflux import _lib
from test_nx_regimes_cpu import constant


@pytest.mark.parametrize("name,value", [("kOptThreads", C.THREADS), ("kOptTile", C.TILE),
                                        ("kOptMaxBlocks", C.MAX_BLOCKS)])
def test_constants_match_the_sources(name, value):
    assert constant(name) == value


def test_every_regime_is_straddled():
    ns = set(C.LENGTHS)
    assert {1, C.THREADS - 1, C.THREADS, C.THREADS + 1, C.TILE - 1, C.TILE, C.TILE + 1} <= ns
    assert C.MAX_BLOCKS * C.TILE - 1 in ns and C.blocks(C.MAX_BLOCKS * C.TILE - 1) == C.MAX_BLOCKS
    # past the cap: some workgroup takes a second pass, and a ragged one
    over = [n for n in ns if n > C.MAX_BLOCKS * C.TILE]
    assert over and all(n % C.THREADS for n in over) and all(C.blocks(n) == C.MAX_BLOCKS for n in over)
    assert set(C.MODEL_SIZES.values()) <= ns
    # the models sit in the many-workgroup, one-pass regime, with a ragged last workgroup
    assert all(1 < C.blocks(n) < C.MAX_BLOCKS and n % C.TILE for n in C.MODEL_SIZES.values())
    assert C.blocks(1) == 1 and C.blocks(C.TILE) == 1 and C.blocks(C.TILE + 1) == 2


def test_model_sizes_are_the_parameter_counts():
    lib = _lib.lib()
    assert C.MODEL_SIZES["FluxGNN(4,128,4)"] == lib.hf_model_param_count(4, 128, 4)
    assert C.MODEL_SIZES["PureGNN(4,128,4)"] == lib.hf_pure_gnn_param_count(4, 128, 4)
    assert C.MODEL_SIZES["PINN(192,256,4)"] == lib.hf_pinn_param_count(192, 256, 4)


def test_workspace_is_one_double_per_workgroup():
    lib = _lib.lib()
    for n in C.LENGTHS:
        assert lib.hf_adam_flat_workspace_bytes(n) == 8 * C.blocks(n)


def test_gradients_are_seeded_and_scaled():
    p0, gs = C.gradients(1000, 6)
    p1, gs1 = C.gradients(1000, 6)
    assert (p0 == p1).all() and all((a == b).all() for a, b in zip(gs, gs1))
    rms = [float((g.astype("f8") ** 2).mean() ** 0.5) for g in gs]
    for k, r in enumerate(rms):
        assert 0.8 * 10.0 ** (k % 3 - 1) < r < 1.2 * 10.0 ** (k % 3 - 1)
