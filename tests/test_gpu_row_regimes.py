"""PureGNN, PINN and generic-graph training over the row regimes of their
GEMMs (tests/row_regimes.py has the regimes, the boundaries and the cases;
test_row_regimes_cpu.py ties them to csrc/ and shows that the gates below
reject a dropped split, dropped ragged rows, a misplaced row tile and an
unwritten output tile on these very inputs).

(a) against float64: delta / out / flux, every parameter gradient and the input
    gradient against the oracle restatement evaluated in float64 on the CPU, at
    the project's gates: forward atol 2e-6 + rtol 1e-5, gradients
    |got - ref| <= 2e-5 max|ref| + 1e-9 per tensor.  PureGNN runs tagged (the chain
    GEMMs, or the generic kernels with arithmetic neighbours where nx does not
    divide 128) and, for PURE_UNTAGGED, as an untagged clone (CSR buckets).
    Every error is recorded as a fraction of max|ref|.
(b) row invariance, bitwise: the forward and data-gradient GEMMs reduce over H or
    2H in one split, so a row's value cannot depend on where its tile sits in the
    grid.  A batch that repeats one 128-row base tile must give outputs periodic
    in that tile and equal to a run of the base alone, bit for bit, the prefix in
    a partial last tile included.  Any misplaced, duplicated or unwritten tile of
    the remapped grids fails exactly.
(c) sliding block, bitwise, for the weight gradients tgemm and tgemm_batch
    compute: with an upstream gradient that is non-zero on one block of whole
    chains or samples inside one split (row_regimes.slide_blocks), every other row
    contributes exact zeros, the other splits' partials are exact zeros, and the
    reduction 0 + ... + p + 0 ... is p: the big batch's weight and bias gradients
    must equal those of the block run alone as its own batch.  That pins every
    split's placement, the stage pairs and the odd last stage, the zeroed ragged
    rows and EX against clamped arithmetic with no tolerance.  It rests on a
    split's stages running in row order from the split's first row whatever the
    split's position and the stage's parity, and on a block that starts on a stage
    boundary meeting the MFMA steps as it does from row 0 (tgemm_tile: `stage`
    differs between parities only in the LDS buffer it reads; read, not measured).
    PureGNN's input_mlp.0 and output_mlp.2 gradients come from gemm_wgrad
    (graph.hip), whose splits are cut every split_rows(N) rows from row 0, not
    where tgemm cuts.  The same reading holds there (gemm_tile runs a split's
    32-row chunks in order from its first row; wgrad_reduce_kernel adds the
    partials in four fixed lanes, all but one of them zeros), so they are compared
    too whenever the block also lies inside one of gemm_wgrad's splits; a block
    that straddles two of them gives p_a + p_b, not the one-split sum, and those
    four tensors are then left to (a).  At N = 16448 the 32-row last split is half
    a chain, which no block of whole chains inside one split covers; the ragged
    last stage is pinned at N = 16368 instead.
(d) two backward passes of one capped case per model give the same bits.
"""
import functools

import numpy as np
import pytest
import torch

import row_regimes as R
from conftest import close
from oracle import hybrid_oracle as O
from test_gpu_pure_gnn_training import grad_gate, run_backward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


def load(m, sd):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def pure_case(H, nx, L, B):
    """(sd, nf, up, float64 reference (delta, grads, nf grad)), computed once."""
    sd, nf, up = R.pure_inputs(H, nx, L, B)
    return sd, nf, up, R.oracle_run(O.pure_gnn_forward, sd, nf, up, torch.float64, O.chain_edges(nx, B))


@functools.lru_cache(maxsize=None)
def pinn_case(D, H, L, B):
    sd, st, up = R.pinn_inputs(D, H, L, B)
    return sd, st, up, R.oracle_run(O.pinn_forward, sd, st, up, torch.float64)


def pinn_backward(m, st, up, state_grad=True):
    """(out, {param: grad}, state grad) of training.pinn_forward under autograd."""
    from hybridflux.training import pinn_forward
    m.zero_grad()
    s = torch.as_tensor(st, device=DEV).requires_grad_(state_grad)
    out = pinn_forward(m, s)
    (out * torch.as_tensor(up, device=DEV)).sum().backward()
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    return out.detach().cpu().numpy(), grads, s.grad.cpu().numpy() if state_grad else None


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    assert np.isfinite(got).all(), what
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (what, int(bad.size), int(bad[0]))


def same_values(got, want, what):
    """Equal as values (a zero of either sign is the same zero)."""
    assert got.shape == want.shape and np.isfinite(got).all(), what
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), float(np.abs(got - want).max()))


def periodic_bits(got, base, what):
    """got [rows, ...] repeats base [128, ...] bit for bit, a partial last tile its prefix."""
    assert len(base) == R.TILE_M
    same_bits(got, R.periodic(base, len(got)), what)


# ------------------------------------------------------------------ (a) against float64
@pytest.mark.parametrize("H,nx,L,B", R.PURE_CHAIN + R.PURE_GENERIC)
def test_pure_vs_float64(hf, record, request, H, nx, L, B):
    sd, nf, up, (wd, wg, wnf) = pure_case(H, nx, L, B)
    m = load(hf.PureGNN(R.PURE_IN_DIM, H, L), sd)
    eit = hf.chain_edge_index(nx, B, DEV)
    runs = [("tagged", eit)] + ([("untagged", eit.clone())] if (H, nx, L, B) in R.PURE_UNTAGGED else [])
    failed = []
    for tag, ei in runs:
        d, grads, gnf = run_backward(m, nf, ei, torch.from_numpy(up))
        for what, got, want in [(f"{tag}_nf", gnf, wnf)] + [(f"{tag}_{k}", grads[k], wg[k]) for k in wg]:
            try:
                grad_gate(record, request, what, got, want, R.REL)
            except AssertionError as e:  # every tensor is measured before the test fails
                failed.append(str(e))
        close(d, wd, 2e-6, 1e-5, what=f"{tag}_delta")
    assert not failed, failed


@pytest.mark.parametrize("D,H,L,B", R.PINN_GEMM + R.PINN_GENERIC)
def test_pinn_vs_float64(hf, record, request, D, H, L, B):
    sd, st, up, (wo, wg, ws) = pinn_case(D, H, L, B)
    m = load(hf.PINN(D, H, L), sd)
    out, grads, gs = pinn_backward(m, st, up)
    failed = []
    for what, got, want in [("state", gs, ws)] + [(k, grads[k], wg[k]) for k in wg]:
        try:
            grad_gate(record, request, what, got, want, R.REL)
        except AssertionError as e:
            failed.append(str(e))
    close(out, wo, 2e-6, 1e-5, what="out")
    assert not failed, failed


def test_flux_general_graph_vs_float64(hf, record, request):
    """FluxGNN(4, 32, 2) under autograd on the 2500-node, 40,000-edge graph (three scan
    chunks, capped edge-row weight gradients, duplicate edges, self-loops, isolated
    nodes), kink-free weights."""
    sd, nf, ei, up = R.flux_graph_inputs()
    wf, wg, wnf = R.oracle_run(O.flux_gnn_forward, sd, nf, up, torch.float64, torch.from_numpy(ei))
    m = load(hf.FluxGNN(*R.FLUX_GRAPH["dims"]), sd)
    x = torch.as_tensor(nf, device=DEV).requires_grad_(True)
    flux = m(x, torch.as_tensor(ei, device=DEV))
    (flux * torch.as_tensor(up, device=DEV)).sum().backward()
    failed = []
    for what, got, want in [("nf", x.grad, wnf)] + [(k, p.grad, wg[k]) for k, p in m.named_parameters()]:
        try:
            grad_gate(record, request, what, got, want, R.REL)
        except AssertionError as e:
            failed.append(str(e))
    assert float(x.grad[R.FLUX_GRAPH["first_isolated"]:].abs().max()) == 0.0
    close(flux, wf, 2e-6, 1e-5, what="flux")
    assert not failed, failed


# ------------------------------------------------------------ (b) row invariance, bitwise
@pytest.mark.parametrize("H,nx,L,B", R.PURE_CHAIN)
def test_pure_rows_do_not_depend_on_their_tile(hf, H, nx, L, B):
    sd, nf, up = R.pure_inputs(H, nx, L, B)
    m = load(hf.PureGNN(R.PURE_IN_DIM, H, L), sd)
    N, B0 = B * nx, R.TILE_M // nx
    nf0, up0 = nf[:R.TILE_M], up[:R.TILE_M]
    big_nf, big_up = R.periodic(nf0, N), R.periodic(up0, N)
    ei = hf.chain_edge_index(nx, B, DEV)
    d, _, gnf = run_backward(m, big_nf, ei, torch.from_numpy(big_up))
    d0, _, gnf0 = run_backward(m, nf0, hf.chain_edge_index(nx, B0, DEV), torch.from_numpy(up0))
    periodic_bits(d, d0, "delta")
    periodic_bits(gnf, gnf0, "d nf")
    with torch.no_grad():  # hf_pure_gnn_forward, the inference forward
        infer = m(torch.as_tensor(big_nf, device=DEV), ei).cpu().numpy()
    same_bits(infer, d, "training forward against hf_pure_gnn_forward")
    if N % R.TILE_M:
        tail = N % R.TILE_M
        same_bits(d[-tail:], d0[:tail], "the partial last tile")
        same_bits(gnf[-tail:], gnf0[:tail], "the partial last tile, d nf")


@pytest.mark.parametrize("D,H,L,B", R.PINN_GEMM)
def test_pinn_rows_do_not_depend_on_their_tile(hf, D, H, L, B):
    sd, st, up = R.pinn_inputs(D, H, L, B)
    m = load(hf.PINN(D, H, L), sd)
    st0, up0 = st[:R.TILE_M], up[:R.TILE_M]
    out, _, gs = pinn_backward(m, R.periodic(st0, B), R.periodic(up0, B))
    out0, _, gs0 = pinn_backward(m, st0, up0)
    periodic_bits(out, out0, "out")
    periodic_bits(gs, gs0, "d state")
    if B % R.TILE_M:
        tail = B % R.TILE_M
        same_bits(out[-tail:], out0[:tail], "the partial last tile")
        same_bits(gs[-tail:], gs0[:tail], "the partial last tile, d state")


# ------------------------------------------------------------- (c) sliding block, bitwise
PURE_TGEMM_GRADS = ("update_mlps.", "output_mlp.0.")  # input_mlp.0 and output_mlp.2: gemm_wgrad's own splits


def check_blocks(grads_of, x, up, blocks, compared=lambda k, start, rows: True):
    """grads_of(x, up) -> {param: grad}.  For every block: the gradients of the whole
    batch with the upstream gradient zeroed outside the block equal those of the
    block's rows run as their own batch.  Returns the number of tensors compared."""
    n = 0
    for start, rows, why in blocks:
        sl = slice(start, start + rows)
        big_up = np.zeros_like(up)
        big_up[sl] = up[sl]
        big, alone = grads_of(x, big_up), grads_of(x[sl], up[sl])
        for k in big:
            if compared(k, start, rows):
                assert np.abs(alone[k]).max() > 0, (k, why)
                same_values(big[k], alone[k], (k, start, rows, why))
                n += 1
    return n


def pure_grads_of(hf, m, nx):
    return lambda nf, up: run_backward(m, nf, hf.chain_edge_index(nx, len(nf) // nx, DEV), torch.from_numpy(up))[1]


@pytest.mark.parametrize("H,nx,L,B", R.PURE_SLIDE)
def test_pure_weight_gradients_of_a_sliding_block(hf, H, nx, L, B):
    sd, nf, up = R.pure_inputs(H, nx, L, B)
    m = load(hf.PureGNN(R.PURE_IN_DIM, H, L), sd)
    blocks = R.pure_slide_blocks(H, nx, L, B)
    Rg = R.split_rows(B * nx)
    one_generic_split = lambda start, rows: start // Rg == (start + rows - 1) // Rg  # noqa: E731
    n = check_blocks(pure_grads_of(hf, m, nx), nf, up, blocks,
                     lambda k, start, rows: k.startswith(PURE_TGEMM_GRADS) or one_generic_split(start, rows))
    assert n == sum(2 * L + (6 if one_generic_split(s, r) else 2) for s, r, _ in blocks)


@pytest.mark.parametrize("D,H,L,B", R.PINN_SLIDE)
def test_pinn_weight_gradients_of_a_sliding_block(hf, D, H, L, B):
    sd, st, up = R.pinn_inputs(D, H, L, B)
    m = load(hf.PINN(D, H, L), sd)
    blocks = R.pinn_slide_blocks(D, H, L, B)
    assert check_blocks(lambda s, u: pinn_backward(m, s, u)[1], st, up, blocks) == 2 * L * len(blocks)


def test_generic_weight_gradients_of_a_sliding_block(hf):
    """The same on the generic path past split_rows' cap, where gemm_wgrad computes
    every weight gradient: PureGNN (64, 48, 2, 700), 117 splits of 288 rows, and
    PINN (15, 16, 2, 40000), 125 splits of 320."""
    H, nx, L, B = R.PURE_GENERIC[1]
    sd, nf, up = R.pure_inputs(H, nx, L, B)
    m = load(hf.PureGNN(R.PURE_IN_DIM, H, L), sd)
    blocks = R.slide_blocks(B * nx, R.split_rows(B * nx), nx, [])
    assert check_blocks(pure_grads_of(hf, m, nx), nf, up, blocks) == (2 * L + 6) * len(blocks) >= 4
    D, H, L, B = R.PINN_GENERIC[0]
    sd, st, up = R.pinn_inputs(D, H, L, B)
    m = load(hf.PINN(D, H, L), sd)
    blocks = R.slide_blocks(B, R.split_rows(B), 1, [])
    assert check_blocks(lambda s, u: pinn_backward(m, s, u)[1], st, up, blocks) == 2 * L * len(blocks) >= 4


# ---------------------------------------------------------------------- (d) determinism
def test_two_backward_passes_give_the_same_bits(hf):
    H, nx, L, B = R.PURE_TWICE
    sd, nf, up = R.pure_inputs(H, nx, L, B)
    m = load(hf.PureGNN(R.PURE_IN_DIM, H, L), sd)
    ei = hf.chain_edge_index(nx, B, DEV)
    a, b = (run_backward(m, nf, ei, torch.from_numpy(up)) for _ in range(2))
    same_bits(a[0], b[0], "delta")
    same_bits(a[2], b[2], "d nf")
    for k in a[1]:
        same_bits(a[1][k], b[1][k], k)
    D, H, L, B = R.PINN_TWICE
    sd, st, up = R.pinn_inputs(D, H, L, B)
    m = load(hf.PINN(D, H, L), sd)
    a, b = (pinn_backward(m, st, up) for _ in range(2))
    same_bits(a[0], b[0], "out")
    same_bits(a[2], b[2], "d state")
    for k in a[1]:
        same_bits(a[1][k], b[1][k], k)
