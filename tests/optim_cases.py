"""The lengths n of the flat buffer at which the optimizer kernels (csrc/optim.hip)
change regime, and the seeded gradients the optimizer tests share.

Both kernels run THREADS threads per workgroup over a grid sized for TILE values
per workgroup, MAX_BLOCKS workgroups at most; beyond MAX_BLOCKS * TILE values a
workgroup strides into a second pass.  test_optim_cases_cpu.py holds the three
constants against the sources.
"""
import numpy as np

THREADS = 256
TILE = 1024
MAX_BLOCKS = 2048

# the parameter counts of the three models the trainers build
MODEL_SIZES = {"FluxGNN(4,128,4)": 165249, "PureGNN(4,128,4)": 149123, "PINN(192,256,4)": 230336}

LENGTHS = (
    1,                             # one thread of one workgroup
    THREADS - 1, THREADS, THREADS + 1,   # a wave short of / exactly / one past a workgroup's first row
    TILE - 1, TILE,                # one workgroup, its last row ragged / full
    TILE + 1,                      # a second workgroup with one value
    MAX_BLOCKS * TILE - 1,         # the whole grid, the last workgroup ragged
    MAX_BLOCKS * TILE + TILE + 1,  # the grid's cap: workgroups 0 .. 4 stride into a second pass
) + tuple(MODEL_SIZES.values())


def blocks(n):
    """Workgroups of both kernels for n values (= the norm's partials)."""
    return min(max(-(-n // TILE), 1), MAX_BLOCKS)


def gradients(n, steps, seed=0):
    """`steps` float32 gradients [n], step k scaled 10^(k mod 3 - 1) (the scales
    of the existing Adam test), and initial parameters [n]."""
    g = np.random.default_rng(seed)
    p0 = g.standard_normal(n, dtype=np.float32)
    gs = [g.standard_normal(n, dtype=np.float32) * np.float32(10.0 ** (k % 3 - 1)) for k in range(steps)]
    return p0, gs
