"""The exact-input cases (tests/exact_cases.py) on the CPU: every case that
tests/test_gpu_exact_structure.py runs on the kernels is shown here to be

  * valid for each precision it runs in (every GEMM input representable, every
    float32 partial sum exact in any order), the backward too where gradients
    are compared;
  * tied to the pinned oracles: oracle.flux_gnn_forward in float32, the bf16
    emulation oracle.hybrid_flux_edge_bf16 and float32 CPU autograd all give
    the float64 reference's bits on these inputs;
  * non-vacuous (conditions, not measurements): fluxes nonzero and distinct,
    one cell's features reach the faces of its receptive field, every ReLU
    layer has pre-activations that are exactly 0;
  * sharp: CPU mutants of the reference (a stale seam slot, swapped k-columns,
    a ReLU' mask of z >= 0, halo cells read from the next IC) each change at
    least one flux or gradient.  No wrong kernel is ever built.
"""
import types

import numpy as np
import pytest
import torch

import exact_cases as X
from oracle import hybrid_oracle as O

ALL = pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)


def params(b):
    return O.params_from(b.sd)


def edge_index(b):
    c = b.case
    return torch.from_numpy(b.ei) if b.ei is not None else O.chain_edges(c.nx, c.B)


@ALL
def test_case_is_valid_and_sharp(case):
    b = X.find_case(case)      # raises when no seed of exact_cases.SEEDS qualifies
    for p in case.precisions:
        assert b.rec.valid(p), (p, b.rec.repr_ok, b.rec.max_bound(), b.rec.m)
    if b.grec is not None:
        assert b.grec.valid("f32"), (b.grec.max_bound(), b.grec.m)
        assert b.grec.max_bound() * 2.0 ** b.grec.m < 2.0 ** 24
    assert X.nonvacuous(case, b.sd, b.nf, b.flux, b.rec) == []
    if case.name.startswith("persist"):   # a second round of the persistent loop on a 256-CU device
        assert X.sw_count(case.layers, case.B, case.nx) > 256


@ALL
def test_oracle_f32_equals_forward64(case):
    b = X.find_case(case)
    if case.kind == "rollout":
        st = case.state0(b.nf)
        fe = O.hybrid_flux_edge(params(b), O.Grid(case.nx), st)         # the grid's real x, weight 0
        assert fe.dtype == np.float32 and np.array_equal(fe.astype(np.float64), b.flux)
        _, F = O.hybrid_update(O.Grid(case.nx), st, fe)
        assert F.dtype == np.float32 and np.array_equal(F.astype(np.float64), b.faces)
        return
    with torch.no_grad():
        fe = O.flux_gnn_forward(params(b), torch.from_numpy(b.nf), edge_index(b)).numpy()
    assert fe.dtype == np.float32
    assert np.array_equal(fe.astype(np.float64).reshape(b.flux.shape), b.flux)


@pytest.mark.parametrize("case", [c for c in X.CASES if "bf16" in c.precisions], ids=lambda c: c.name)
def test_oracle_bf16_emulation_equals_forward64(case):
    """bf16 and float32 arithmetic give the same bits on these inputs.  The
    emulation takes one x column per call: the rollout cases share the grid's
    (weight 0); the others are checked IC by IC (the first 8)."""
    b = X.find_case(case)
    nx = case.nx
    if case.kind == "rollout":
        st = case.state0(b.nf)[:8]
        fe = O.hybrid_flux_edge_bf16(params(b), O.Grid(nx), st)
        assert np.array_equal(fe.astype(np.float64), b.flux[:8])
        return
    nf = b.nf.reshape(case.B, nx, 4)
    for ic in range(min(case.B, 8)):
        grid = types.SimpleNamespace(nx=nx, x=nf[ic, :, 3].astype(np.float64))
        st = np.ascontiguousarray(nf[ic:ic + 1, :, :3].transpose(0, 2, 1))
        fe = O.hybrid_flux_edge_bf16(params(b), grid, st)
        assert np.array_equal(fe.astype(np.float64), b.flux[ic:ic + 1]), ic


@pytest.mark.parametrize("case", [c for c in X.CASES if c.grads], ids=lambda c: c.name)
def test_autograd_f32_equals_grads64(case):
    b = X.find_case(case)
    p = {k: v.clone().requires_grad_(True) for k, v in params(b).items()}
    nf = torch.from_numpy(b.nf).clone().requires_grad_(True)
    fe = O.flux_gnn_forward(p, nf, edge_index(b))
    (fe * torch.from_numpy(b.gup)).sum().backward()
    assert np.array_equal(fe.detach().numpy().astype(np.float64), b.flux.reshape(-1))
    assert np.array_equal(nf.grad.numpy().astype(np.float64), b.grads["node_features"])
    for k, v in p.items():
        assert v.grad.dtype == torch.float32
        assert np.array_equal(v.grad.numpy().astype(np.float64), b.grads[k]), k


def _sub(case, b):
    nb = X.sub_batch(case)
    return nb, b.nf[:nb * case.nx]


@pytest.mark.parametrize("case", [c for c in X.CASES if c.graph is None], ids=lambda c: c.name)
def test_forward_mutants_are_detected(case):
    b = X.find_case(case)
    nx, L = case.nx, case.layers
    nb, nf = _sub(case, b)
    base, _ = X.forward64(b.sd, nf, nb, nx, record=False)
    assert np.array_equal(base, b.flux[:nb])
    applied = []
    stream = np.arange(nb)[:, None] * X.sw_segment(nx, L) + L + np.arange(nx)[None, :]
    if L >= 2 and nx >= 2 and np.any(stream % X.SW_STRIDE == 0):
        seam, _ = X.forward64(b.sd, nf, nb, nx, record=False, seam_mutant=True)
        assert not np.array_equal(seam, base), "stale seam slot not detected"
        applied.append("seam")
    if L >= 1:
        swapped, _ = X.forward64(X.swap_k_mutant(b.sd), nf, nb, nx, record=False)
        assert not np.array_equal(swapped, base), "swapped k-columns not detected"
        applied.append("swap_k")
    if nb >= 2:
        halo = X.halo_mutant_forward64(b.sd, nf, nb, nx)
        assert not np.array_equal(halo, base), "halo cells of the next IC not detected"
        applied.append("halo")
    assert applied


@pytest.mark.parametrize("case", [c for c in X.CASES if c.graph is not None], ids=lambda c: c.name)
def test_graph_mutant_is_detected(case):
    b = X.find_case(case)
    swapped, _ = X.forward64(X.swap_k_mutant(b.sd), b.nf, case.B, case.nx, edge_index=b.ei, record=False)
    assert not np.array_equal(swapped, b.flux)


@pytest.mark.parametrize("case", [c for c in X.CASES if c.grads], ids=lambda c: c.name)
def test_relu_mask_mutant_is_detected(case):
    """ReLU' = (z >= 0) instead of (z > 0): some gradient moves, the flux does not."""
    b = X.find_case(case)
    flux, grads, _ = X.grads64(b.sd, b.nf, case.B, case.nx, b.gup, edge_index=b.ei, mask_ge=True)
    assert np.array_equal(flux, b.flux.reshape(-1))
    assert any(not np.array_equal(grads[k], b.grads[k]) for k in grads)


def test_representability_checks():
    """The record's own predicates on known values."""
    assert X.bf16_exact([0, 1, 255, 256, 258, -0.5]) and not X.bf16_exact([257.0])
    assert X.f16x3_exact([2049.0, 4097.0, 0.5]) and not X.f16x3_exact([70000.0])
    assert not X.f16x3_exact([2.0 ** 23 + 1.0 - 2.0 ** 30])
    assert X.f16_exact([2048.0]) and not X.f16_exact([2049.0])
    assert X.dyadic_bits([1.0, 0.5], [0.25]) == 2
    sd = X.make_sd(2, 0)
    nf = X.features(2, 9, 0)
    nf[0, 0] = 257.0                      # not a bf16 value: the record must say so
    _, rec = X.forward64(sd, nf, 2, 9)
    assert not rec.valid("bf16") and rec.valid("f32")


def test_mismatch_report_names_ic_edge_and_seam():
    want = np.zeros((3, 200))
    got = want.copy()
    assert X.mismatch(got, want, 100) is None
    got[1, 163] = 1.0
    msg = X.mismatch(got, want, 100)
    assert "(1, 163)" in msg and "1 of 600" in msg and "[0]" in msg   # face 63: 63 mod 63 = 0
