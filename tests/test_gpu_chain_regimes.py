"""FluxGNN chain training over its batch and row regimes (tests/chain_regimes.py
has the regimes and the cases; test_chain_regimes_cpu.py ties them to csrc/ and
shows on these very inputs that the gates below reject the chains of a later
fused pass or of the ragged group dropped, a halo row taken from the neighbouring
chain, a split's last stage dropped and a mask word read from the chain 4 CUs back).

(a) exact inputs, bit for bit: small-integer features, sparse integer weights and a
    quarter-dense integer upstream gradient make every float32 partial sum exact in
    any order (exact_cases.py), so the flux, every parameter gradient and the
    node-feature gradient must equal the float64 reference's bits at any batch
    size: persistent passes, trips of the edge kernels, stages, splits and slices
    cannot matter.  The fused passes depend on the device's CU count; the cases were
    sized for 256 and the test asserts the passes again with the real count.
(b) chain invariance, bit for bit, with the golden trained weights (dense
    arithmetic, realistic masks): a chain's flux, tape and node-feature gradient do
    not depend on the other chains of the batch, so a batch that repeats a base of 8
    chains (upstream gradient likewise) must give flux and node-feature gradient
    periodic in the base and equal to the base run alone.  The base run itself is
    compared with float64 autograd of the oracle at the project's gates (flux 1e-5
    of max|ref|, gradients 2e-5 of max|ref| + 1e-9 per tensor).
(c) two backward passes give the same bits in every gradient.
"""
import numpy as np
import pytest
import torch

import chain_regimes as C
import exact_cases as X
import row_regimes as R
from conftest import golden, rand_sd
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def load(hf, sd, dims):
    m = hf.FluxGNN(*dims)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV)


def backward(m, nf, ei, gup):
    """(flux, {param: grad, "node_features": grad}) of FluxGNN.forward under autograd."""
    m.zero_grad()
    x = torch.as_tensor(nf, device=DEV).clone().requires_grad_(True)
    flux = m(x, ei)
    (flux * torch.as_tensor(gup, device=DEV)).sum().backward()
    g = {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    g["node_features"] = x.grad.detach().cpu().numpy().copy()
    return flux.detach().cpu().numpy(), g


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    assert np.isfinite(got).all(), what
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (what, int(bad.size), int(bad[0]))


def reaches_its_passes(case, cus):
    """The passes the case's `why` counts on 256 CUs happen on this device too."""
    if C.fused_chain(case.in_dim, case.hidden, case.layers, case.nx):
        want = C.fused_passes(case.B)
        got = C.fused_passes(case.B, cus)
        assert got >= want, f"{case.name}: {got} fused passes on {cus} CUs, sized for {want} on {C.CUS}"
        if want > 1 and case.B % C.NW:   # the ragged group is the last group of a later pass
            assert C.cdiv(case.B, C.NW) - 1 >= C.train_blocks(case.B, cus)


# ------------------------------------------------------------- (a) exact inputs, bitwise
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_regime_bitwise(hf, cus, case):
    reaches_its_passes(case, cus)
    b = X.find_case(case)
    assert b.seed == case.seed0
    m = load(hf, b.sd, (case.in_dim, case.hidden, case.layers))
    flux, g = backward(m, b.nf, hf.chain_edge_index(case.nx, case.B, DEV), b.gup)
    failed = []
    msg = X.mismatch(flux.reshape(case.B, 2 * case.nx), b.flux, case.nx)
    if msg:
        failed.append(f"flux: {msg}")
    assert set(g) == set(b.grads)
    for k in sorted(g):   # every tensor is compared before the test fails
        msg = X.mismatch(g[k], b.grads[k])
        if msg:
            failed.append(f"d {k}: {msg}")
    assert not failed, (case.name, failed)


# -------------------------------------------------------- (b) chain invariance, bitwise
def golden_model(hf):
    w = golden("weights_W1_r2.npz")
    sd = {k: w[k] for k in w.files}
    return sd, load(hf, sd, (4, 128, 4))


_BASE = {}


def base_run(hf, nx):
    """The base of 8 chains at nx: (states, upstream [8, 2nx], nf, flux, grads), run once."""
    if nx not in _BASE:
        G = O.Grid(nx, dt=5e-3)
        states = np.stack([O.initial_condition(G, s) for s in range(60, 60 + C.INVARIANCE_BASE)])
        up = torch.randn(C.INVARIANCE_BASE, 2 * nx, generator=torch.Generator().manual_seed(1000 + nx)).numpy()
        _, m = golden_model(hf)
        nf, ei = hf.build_chain_graph_batch(states, G.x, DEV)
        flux, g = backward(m, nf, ei, up.reshape(-1))
        _BASE[nx] = (G, states, up, nf.detach().cpu().numpy(), flux, g)
    return _BASE[nx]


@pytest.mark.parametrize("nx", sorted({nx for nx, _ in C.INVARIANCE}))
def test_invariance_base_vs_float64(hf, nx):
    G, states, up, nf, flux, g = base_run(hf, nx)
    sd, _ = golden_model(hf)
    wf, wg, wnf = R.oracle_run(O.flux_gnn_forward, sd, nf, up.reshape(-1), torch.float64,
                               O.chain_edges(nx, C.INVARIANCE_BASE))
    failed = []
    for what, got, want, rel in [("flux", flux, wf, 1e-5), ("node_features", g["node_features"], wnf, R.REL)] + \
            [(k, g[k], wg[k], R.REL) for k in wg]:
        err, scale = float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(want).max())
        print(f"nx {nx} {what}: err {err:.3e} of max|ref| {scale:.3e} = {err / scale:.2e} (gate {rel:.0e})")
        assert np.isfinite(got).all() and scale > 0, what
        if err > rel * scale + 1e-9:
            failed.append((what, err, scale))
    assert not failed, failed


@pytest.mark.parametrize("nx,B", C.INVARIANCE)
def test_chains_do_not_depend_on_their_batch(hf, cus, nx, B):
    G, states, up, nf0, flux0, g0 = base_run(hf, nx)
    if C.fused_chain(4, 128, 4, nx):
        assert C.fused_passes(B, cus) >= C.fused_passes(B) >= 2
    else:
        assert C.cdiv(B * nx, R.TILE_M) >= R.REMAP_GROUP
    _, m = golden_model(hf)
    big_states, big_up = R.periodic(states, B), R.periodic(up, B)
    nf, ei = hf.build_chain_graph_batch(big_states, G.x, DEV)
    same_bits(nf.detach().cpu().numpy(), R.periodic(nf0.reshape(C.INVARIANCE_BASE, nx, 4), B).reshape(B * nx, 4), "nf")
    flux, g = backward(m, nf, ei, big_up.reshape(-1))
    same_bits(flux.reshape(B, 2 * nx), R.periodic(flux0.reshape(C.INVARIANCE_BASE, 2 * nx), B), "flux")
    same_bits(g["node_features"].reshape(B, nx, 4),
              R.periodic(g0["node_features"].reshape(C.INVARIANCE_BASE, nx, 4), B), "d node_features")
    assert np.abs(g0["node_features"]).max() > 0 and np.abs(flux0).max() > 0


# ---------------------------------------------------------------------- (c) determinism
@pytest.mark.parametrize("nx,B,L,H", C.TWICE)
def test_two_backward_passes_give_the_same_bits(hf, nx, B, L, H):
    """Random dense weights and normal features: the float32 sums round, so equal bits
    mean a fixed order of every split, slice and per-wave accumulation."""
    assert H == 128 and (nx, B, L, H) in C.SHAPES
    rng = np.random.default_rng(nx + B)
    m = load(hf, rand_sd(L, nx + B), (4, H, L))
    nf = rng.normal(0, 1, (B * nx, 4)).astype(np.float32)
    gup = rng.normal(0, 1, B * 2 * nx).astype(np.float32)
    ei = hf.chain_edge_index(nx, B, DEV)
    (f1, g1), (f2, g2) = (backward(m, nf, ei, gup) for _ in range(2))
    same_bits(f1, f2, "flux")
    for k in g1:
        assert np.abs(g1[k]).max() > 0, k
        same_bits(g1[k], g2[k], k)
