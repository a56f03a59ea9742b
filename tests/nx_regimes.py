"""The chain lengths at which the training-side kernels change regime, and the
(nx, B) cases that put a test on each side of every boundary.  A shared table,
not a test: test_nx_regimes_cpu.py ties the boundaries to the constants in
csrc/, test_gpu_nx_regimes.py runs the cases.  When a threshold moves in the
sources, move it here and add the sizes next to its new place.

The launchers (launch_unroll_update / launch_unroll_adjoint, launch_ablation_loss,
launch_pinn_loss, the PINN and PureGNN unroll launchers) dispatch on nx into
  circulant LDS kernels .. one workgroup per IC, dynamic LDS ~ nx: every nx in
      1..FV_LDS_MAX_NX that is not an FFT size
  FFT kernels ............ one wave per pair of ICs, FFT_SIZES
  hf_ablation_loss ....... one launch for non-FFT nx <= LOSS_FUSED_MAX_NX, else three
      launches around launch_poisson (FFT sizes: poisson_fft_kernel; nx <=
      FV_LDS_MAX_NX: poisson_kernel; beyond: poisson_tiled_kernel)
  PureGNN unroll ......... tiles of PURE_TILE cells
"""

SMALL_MAX_NX = 64          # kFvSmallMaxNx; up to here the tests' dt is the reference's 5e-3
FFT_MIN_NX = 256           # kFftMinNx
FFT_MAX_NX = 2048          # kFftMaxNx
FV_LDS_MAX_NX = 6144       # kFvLdsMaxNx: the circulant kernels' LDS limit, refused beyond
LOSS_FUSED_MAX_NX = 2048   # kLossFusedMaxNx: hf_ablation_loss's one-launch kernel
PURE_TILE = 1024           # kPuTile
FFT_WAVES = 4              # kFftWaves: IC pairs per workgroup of the FFT kernels
FFT_SIZES = (256, 512, 1024, 2048)


def uses_fft(nx):
    """poisson_uses_fft of csrc/hf_internal.h."""
    return FFT_MIN_NX <= nx <= FFT_MAX_NX and nx & (nx - 1) == 0


def dt_of(nx):
    """The time step of the wide cases: the reference's 5e-3 at its CFL number
    dt / dx of nx = 64 (as test_gpu_tridiag.py's dt_of)."""
    return 5e-3 * min(1.0, 64.0 / nx)


# (nx, B, why) for hf_unroll_update / hf_unroll_adjoint
UNROLL_WIDE_WHY = [
    (257, 3, "first size past an FFT size: circulant, one thread owns two cells"),
    (512, 1, "FFT 512, a lone IC: the pair's second half is empty"),
    (512, 9, "FFT 512, one IC more than a workgroup's four pairs"),
    (1024, 3, "FFT 1024, an odd IC count"),
    (2048, 2, "FFT 2048: 136 KiB of static LDS, 32 double2 per lane"),
    (2048, 9, "FFT 2048, two workgroups at one per CU"),
    (1000, 2, "circulant between the FFT sizes"),
    (4096, 2, "a power of two that is not an FFT size: circulant"),
    (6144, 3, "the LDS limit: 122,912 B (update) and 122,880 B (adjoint) of dynamic LDS"),
]
UNROLL_WIDE = [(nx, B) for nx, B, _ in UNROLL_WIDE_WHY]
# where hf_step is the flux kernel followed by fv_step_kernel<true> / fv_step_fft_kernel<true>
UPDATE_BITWISE_WIDE = [(257, 3), (512, 3), (1024, 3), (2048, 2), (6144, 2)]
# (nx, B) for the K-step FluxGNN gradients: FluxGNN(4, 64, 2), K = 2
UNROLLED_GRAD_WIDE = [(512, 3), (2048, 2), (6144, 1)]

# (nx, why) for hf_ablation_loss, B = LOSS_WIDE_B each
LOSS_WIDE_WHY = [
    (512, "FFT: three launches around poisson_fft_kernel"),
    (1024, "FFT: three launches"),
    (2048, "FFT: three launches, the largest FFT size"),
    (2047, "the largest one-launch size (loss_step_kernel)"),
    (2049, "the first three-launch circulant size (poisson_kernel)"),
    (6144, "poisson_kernel at its LDS limit"),
    (6160, "poisson_tiled_kernel"),
]
LOSS_WIDE = [nx for nx, _ in LOSS_WIDE_WHY]
LOSS_WIDE_B = 5
LOSS_WIDE_FULL = [512, 2049]  # the in-kernel rollout energy term in both three-launch paths

# hf_pinn_loss and the PINN unroll loss / adjoint (always circulant): B = PINN_WIDE_B
PINN_WIDE = [2048, 4097, 6144]
PINN_WIDE_B = 3

# (nx, B, why) for the PureGNN unroll update / adjoint
PURE_WIDE_WHY = [
    (1024, 2, "exactly one tile"),
    (2049, 2, "a one-cell tail tile"),
    (6144, 1, "six whole tiles"),
]
PURE_WIDE = [(nx, B) for nx, B, _ in PURE_WIDE_WHY]


def long_wave(nx, B):
    """[B, nx] float64: 0.4 sin(x + b) + 0.2 sin(3 x + 2 b) on the unit circle's cell
    centres.  The wide cases add it to their random densities: the spectral Poisson
    operator divides mode q by q, so white noise of amplitude a alone gives an E of
    about a sqrt(3.3 / nx), 2e-3 at nx = 6144 and lost next to the other terms of a
    loss, while this wave gives an E of amplitude 0.4 at any nx."""
    import numpy as np
    x = 2 * np.pi * (np.arange(nx) + 0.5) / nx
    b = np.arange(B)[:, None]
    return 0.4 * np.sin(x + b) + 0.2 * np.sin(3 * x + 2 * b)


def all_sizes():
    """Every nx of the table."""
    return sorted({nx for nx, _ in UNROLL_WIDE + UPDATE_BITWISE_WIDE + UNROLLED_GRAD_WIDE + PURE_WIDE}
                  | set(LOSS_WIDE) | set(PINN_WIDE))
