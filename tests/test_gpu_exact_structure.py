"""Bitwise structural tests of the FluxGNN kernels on exact inputs.

Every case of tests/exact_cases.py (shown valid, tied to the pinned oracles and
sharp by tests/test_exact_cases_cpu.py) through the kernels: inputs and weights
are small integers chosen so that every GEMM input is representable in f32,
f16x3 and bf16 and every float32 partial sum is exact in any order, so every
kernel family must give the float64 reference's bits.  Every assertion is
array equality; there is no tolerance.  The features are i.i.d. per cell, so a
wrong neighbour at a seam, a stale parity slot or an index off by one is an
O(1) mismatch, and the failure message names the first (IC, edge), the count
and the face index mod 63 (the bf16 super-window kernel's wave stride).

Kernel families reached (case names of exact_cases.CASES):
  fused_*      nx = 16 MT: B = 5 the cell-split flux kernels, B = 2048 the
               IC-per-wave chain_flux_kernel, in f32 / f16x3 / bf16
  tiny_* seg_* win_* swface_* long_* persist_*
               any other nx: bf16 chain_flux_sw_kernel (several ICs per wave,
               segment = wave stride, segment = faces of a super-window, a second
               round of the persistent loop), f32 / f16x3 64-cell windows
  dense_*      8 nonzeros per weight row, f32 / f16x3
  graph_*      the generic CSR kernels (graph.hip) at widths 32..256
  rollout_*    the rollout cores' face flux (engine.run and engine.step),
               nx = 100 / 1024 the flux kernels' face-flux store path
  train_*      the chain training path (fused forward with tape, GEMM forward,
               stencil / split-K weight gradients, generic CSR at width 16)
"""
import numpy as np
import pytest
import torch

import exact_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    return hybridflux


def same(got, want, nx=None, what=""):
    if hasattr(got, "detach"):
        got = got.detach().cpu().numpy()
    msg = X.mismatch(got, want, nx)
    assert msg is None, f"{what}: {msg}"


def pairs(kind):
    return [pytest.param(c, p, id=f"{c.name}-{p}") for c in X.cases(kind) for p in c.precisions]


def load(hf, b, precision="f32"):
    c = b.case
    m = hf.FluxGNN(4, c.hidden, c.layers, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in b.sd.items()})
    return m.to(DEV)


# ------------------------------------------------------------------- a. flux kernels
@pytest.mark.parametrize("case,precision", pairs("flux"))
def test_chain_flux_bitwise(hf, case, precision):
    from hybridflux import engine
    b = X.find_case(case)
    if case.name.startswith("persist"):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert X.sw_count(case.layers, case.B, case.nx) > cus, "no second round of the persistent loop"
    m = engine.DeviceModel(b.sd, torch.device(DEV), precision)
    fe = engine.chain_flux(m, torch.from_numpy(b.nf).to(DEV), case.B, case.nx)
    same(fe.reshape(case.B, 2 * case.nx), b.flux, case.nx, f"{case.name} {precision}")


FORWARD_CASES = ["fused_nx64_B5_L4", "fused_nx64_B2048_L4", "fused_nx48_B5_L8", "tiny_nx7_B300_L4",
                 "win_nx100_B6_L4", "long_nx1024_B3_L4"]


@pytest.mark.parametrize("precision", X.PRECS)
@pytest.mark.parametrize("name", FORWARD_CASES)
def test_module_forward_bitwise(hf, name, precision):
    """FluxGNN.forward under no_grad on the tagged graph, one case per family."""
    from hybridflux.graph_constructor import chain_edge_index
    case = X.BY_NAME[name]
    b = X.find_case(case)
    m = load(hf, b, precision)
    with torch.no_grad():
        fe = m(torch.from_numpy(b.nf).to(DEV), chain_edge_index(case.nx, case.B, DEV))
    same(fe.reshape(case.B, 2 * case.nx), b.flux, case.nx, f"{name} {precision}")


def test_untagged_chains_generic_path_bitwise(hf):
    """The same chains as an untagged copy of the edge index: hf_graph_flux."""
    from hybridflux import engine
    from hybridflux.graph_constructor import chain_edge_index
    case = X.BY_NAME["win_nx100_B6_L4"]
    b = X.find_case(case)
    nf = torch.from_numpy(b.nf).to(DEV)
    ei = chain_edge_index(case.nx, case.B, DEV).clone()
    with torch.no_grad():
        fe = load(hf, b)(nf, ei)
    same(fe.reshape(case.B, 2 * case.nx), b.flux, case.nx, "FluxGNN.forward, untagged")
    fe = engine.graph_flux(engine.DeviceModel(b.sd, torch.device(DEV), "f32"), nf, ei)
    same(fe.reshape(case.B, 2 * case.nx), b.flux, case.nx, "engine.graph_flux")


@pytest.mark.parametrize("case", X.cases("graph"), ids=lambda c: c.name)
def test_generic_graph_bitwise(hf, case):
    """Degree-4 circulant, and a graph with isolated and degree-1 nodes (degrees
    0, 1, 2, 4 only: the mean is dyadic as a division or as a reciprocal), at
    every width."""
    b = X.find_case(case)
    with torch.no_grad():
        fe = load(hf, b)(torch.from_numpy(b.nf).to(DEV), torch.from_numpy(b.ei).to(DEV))
    same(fe, b.flux, None, case.name)


# ----------------------------------------------------------------- b. rollout cores
@pytest.mark.parametrize("case,precision", pairs("rollout"))
def test_rollout_face_flux_bitwise(hf, case, precision):
    """The rollout cores (other instantiations of the flux cores) and, at
    nx = 100 / 1024, the flux kernels' face-flux store: the first step's face
    flux of engine.run and of engine.step.  Nothing is asserted about the state
    after the step (the finite-volume and Poisson arithmetic is not exact)."""
    from hybridflux import engine
    b = X.find_case(case)
    dev = torch.device(DEV)
    m = engine.DeviceModel(b.sd, dev, precision)
    grid = engine.Grid(case.nx)
    st = torch.from_numpy(case.state0(b.nf)).to(dev)
    out = engine.run(m, grid, st, 1, traj=False, flux=True)
    same(out["flux"][:, 0], b.faces, case.nx, f"{case.name} {precision} run")
    _, F, _ = engine.step(m, grid, st, flux_face=True)
    same(F, b.faces, case.nx, f"{case.name} {precision} step")


# ------------------------------------------------------------ c. chain training path
def _backward(m, nf_np, ei, gup):
    m.zero_grad()
    nf = torch.from_numpy(nf_np).to(DEV).requires_grad_(True)
    flux = m(nf, ei)
    (flux * torch.from_numpy(gup).to(DEV)).sum().backward()
    g = {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    g["node_features"] = nf.grad.detach().cpu().numpy().copy()
    return flux.detach().cpu().numpy(), g


def _check_grads(b, flux, g, what):
    same(flux, b.flux.reshape(-1), None, f"{what} flux")
    assert set(g) == set(b.grads)
    for k in g:
        same(g[k], b.grads[k], None, f"{what} d {k}")


@pytest.mark.parametrize("case", X.cases("train"), ids=lambda c: c.name)
def test_chain_training_path_bitwise(hf, case):
    """FluxGNN.forward under autograd on tagged chains, backward() with an
    integer upstream gradient: flux, every parameter gradient and the
    node-feature gradient equal float64 autograd bitwise (ReLU' at a
    pre-activation of exactly 0 included), and two passes are identical."""
    from hybridflux.graph_constructor import chain_edge_index
    b = X.find_case(case)
    m = load(hf, b)
    ei = chain_edge_index(case.nx, case.B, DEV)
    flux, g = _backward(m, b.nf, ei, b.gup)
    _check_grads(b, flux, g, case.name)
    flux2, g2 = _backward(m, b.nf, ei, b.gup)
    assert np.array_equal(flux, flux2) and all(np.array_equal(g[k], g2[k]) for k in g)


def test_untagged_training_path_bitwise(hf):
    """An untagged copy of the chains: the generic CSR forward and backward."""
    from hybridflux.graph_constructor import chain_edge_index
    case = X.BY_NAME["train_nx64_B5_L4_H128"]
    b = X.find_case(case)
    flux, g = _backward(load(hf, b), b.nf, chain_edge_index(case.nx, case.B, DEV).clone(), b.gup)
    _check_grads(b, flux, g, "untagged")


def test_graph_backward_degree4_bitwise(hf):
    """hf_graph_backward on the degree-4 circulant graph."""
    case = X.BY_NAME["graph_circ4_H128"]
    b = X.find_case(case)
    m = load(hf, b)
    ei = torch.from_numpy(b.ei).to(DEV)
    flux, g = _backward(m, b.nf, ei, b.gup)
    _check_grads(b, flux, g, case.name)
    flux2, g2 = _backward(m, b.nf, ei, b.gup)
    assert np.array_equal(flux, flux2) and all(np.array_equal(g[k], g2[k]) for k in g)
