"""Bitwise structural tests of the PureGNN and PINN kernels on saturating inputs.

Every case of tests/saturating_cases.py (shown valid, tied to the pinned
oracles and sharp by tests/test_saturating_cases_cpu.py) through the kernels:
weights in S * {small integers} before every tanh and integer inputs make every
tanh input 0 or at least S = 16 in size, so every activation is exactly -1, 0
or +1, every state, delta and gradient is an integer and every float32 partial
sum is exact in any order.  Every kernel must then give the float64
reference's values; every assertion is array equality (-0.0 == +0.0), there is
no tolerance.  Inputs are i.i.d. per cell, so a wrong neighbour, a wrong row of
a partial tile, a seam between two chains of one 128-row tile or a dropped
half-K partial is an O(1) mismatch, and the failure message names the first
index (IC / row, ..., unit) and the count.

The premise that the device libm tanhf (tgemm.h, graph.hip, pure_train.hip and
the generic paths) returns exactly 0 and +-1 at 0 and at multiples of S is the
first test here; it held at S = 16.  tanh_fast's saturation is shown on the CPU.

Kernel families reached (kinds of saturating_cases.CASES):
  pure_fwd   PureGNN.forward under no_grad and the training forward: tagged
             chains on the chain GEMMs with the message epilogue (a full and a
             partial 128-row tile, seams inside a tile, nx = 1, 2, 128, H = 192),
             tagged chains on the generic kernels, untagged clones and a random
             graph (duplicate edges, self-loops, isolated nodes) on CSR buckets,
             in_dim = 3
  pure_roll  the one-launch rollout at H in {64, 128} x nx in {16, 32, 48, 64},
             L in {0, 1, 4, 8} on packed weights and L = 10 on nn.Linear rows,
             B in {1, 5, 600}; the per-step kernels at (64, 100) and (32, 16);
             traj, final, traj=False, T = 0, the scored call
  pinn_roll  the one-launch PINN at (192, 256), L in {2, 3, 4, 8}, B in
             {1, 15, 16, 17, 33}, T = 1 and 6, forward(); the per-layer GEMMs at
             (96, 64) and the generic kernels at (63, 40); the scored call
  pure_bwd   PureGNN under autograd at the shapes of test_gpu_pure_gnn_training's
             CHAIN_CASES with L <= 2 (the residual path mixes gradients of 16^l:
             deeper cases leave float32's 24 bits), tagged, untagged, random graph
  pinn_bwd   training.pinn_forward at (192,256,4,32), (192,256,2,5), (96,64,3,130)
             and (144,96,3,7); L = 8 is left out: the record forbids it (the
             backward's absolute sums reach 2^31 units)
"""
import numpy as np
import pytest
import torch

import saturating_cases as C
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = C.T_STEPS


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    return hybridflux


def same(got, want, what=""):
    if hasattr(got, "detach"):
        got = got.detach().cpu().numpy()
    assert got.dtype == np.float32, (what, got.dtype)
    msg = C.mismatch(got, want)
    assert msg is None, f"{what}: {msg}"


def by_kind(kind):
    return pytest.mark.parametrize("case", C.cases(kind), ids=lambda c: c.name)


def load(hf, b):
    c = b.case
    m = hf.PureGNN(c.in_dim, c.H, c.L) if c.pure else hf.PINN(c.D, c.H, c.L)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in b.sd.items()})
    return m.to(DEV)


def edge_indices(hf, b):
    """(what, edge_index) pairs: chains tagged and as an untagged clone; the graph."""
    c = b.case
    if c.graph:
        return [("graph", torch.from_numpy(b.ei).to(DEV))]
    eit = hf.chain_edge_index(c.nx, c.B, DEV)
    return [("tagged", eit), ("untagged", eit.clone())]


# ------------------------------------------------------------------------ premise
def test_premise_libm_tanh_saturates(hf):
    """One tanh layer on the generic path, PINN(18, 9, 2): unit j of the hidden
    layer is tanh(S * state[j]) and lands alone on output row 9 + j, whose own
    state is 0.  At 0, +-16, +-32, +-48, +-160 the device tanhf must return
    exactly 0 and +-1.  A failure here is a finding about the premise of this
    file (double S), not a kernel bug."""
    v = np.array([0, 1, -1, 2, -2, 3, -3, 10, -10], np.float32)
    assert np.array_equal(v * np.float32(C.S), np.float32([0, 16, -16, 32, -32, 48, -48, 160, -160]))
    W0 = np.zeros((9, 18), np.float32)
    W0[np.arange(9), np.arange(9)] = C.S
    W1 = np.zeros((18, 9), np.float32)
    W1[9 + np.arange(9), np.arange(9)] = 1
    m = hf.PINN(18, 9, 2)
    m.load_state_dict({"net.0.weight": torch.from_numpy(W0), "net.0.bias": torch.zeros(9),
                       "net.2.weight": torch.from_numpy(W1), "net.2.bias": torch.zeros(18)})
    state = np.zeros((2, 3, 6), np.float32)
    state.reshape(2, 18)[0, :9] = v
    state.reshape(2, 18)[1, :9] = -v
    with torch.no_grad():
        out = m.to(DEV)(torch.from_numpy(state).to(DEV)).cpu().numpy().reshape(2, 18)
    print("tanhf at", (v * C.S).tolist(), "->", out[0, 9:].tolist())
    assert np.array_equal(out[:, :9], state.reshape(2, 18)[:, :9])
    assert np.array_equal(out[0, 9:], np.sign(v)) and np.array_equal(out[1, 9:], -np.sign(v)), out[:, 9:]


# ---------------------------------------------------------------- PureGNN forward
@by_kind("pure_fwd")
def test_pure_forward_bitwise(hf, case):
    """PureGNN.forward under no_grad, and with grad enabled the training forward
    (pure_train.hip: the same launches with a tape), on every edge index."""
    b = C.find_case(case)
    m = load(hf, b)
    nf = torch.from_numpy(b.nf).to(DEV)
    for what, ei in edge_indices(hf, b):
        with torch.no_grad():
            d = m(nf, ei)
        same(d, b.out, f"{case.name} {what}")
        dt = m(nf, ei)
        assert dt.requires_grad
        same(dt, b.out, f"{case.name} {what}, training forward")


# ---------------------------------------------------------------- PureGNN rollout
def check_metrics(got, traj64):
    """The scored call's metric rows [B,T+1,4] (energy, charge, finite flag, .)
    against oracle.rollout_metrics of the exact trajectory, at the gate of
    test_gpu_model_scoring.py (rtol 2e-7: one float32 rounding of a float64 sum)."""
    energy, charge, finite = O.rollout_metrics(traj64.astype(np.float32))
    me = got.cpu().numpy()
    np.testing.assert_allclose(me[..., 0], energy, rtol=2e-7, atol=0)
    np.testing.assert_allclose(me[..., 1], charge, rtol=2e-7, atol=0)
    assert finite.all() and (me[..., 2] == 1).all()


@by_kind("pure_roll")
def test_pure_rollout_bitwise(hf, case):
    b = C.find_case(case)
    m = load(hf, b)
    s0 = torch.from_numpy(b.state0).to(DEV)
    out = m.rollout(s0, T, b.x)
    same(out["traj"], b.out, f"{case.name} traj")
    same(out["final"], b.out[:, -1], f"{case.name} final")
    only = m.rollout(s0, T, b.x, traj=False)
    assert only["traj"] is None
    same(only["final"], b.out[:, -1], f"{case.name} final, traj=False")
    same(m.rollout(s0, 0, b.x)["final"], b.state0, f"{case.name} T = 0")
    sc = m.rollout(s0, T, b.x, metrics=True)
    same(sc["traj"], b.out, f"{case.name} scored traj")
    same(sc["final"], b.out[:, -1], f"{case.name} scored final")
    check_metrics(sc["metrics"], b.out)
    for nb in (1, 5):                       # a sub-batch: the same values
        if nb < case.B:
            sub = m.rollout(s0[:nb].contiguous(), T, b.x)
            same(sub["traj"], b.out[:nb], f"{case.name} first {nb} ICs alone")


# ------------------------------------------------------------------------- PINN
def pinn_pairs():
    out = []
    for c in C.cases("pinn_roll"):
        for nb in ((1, 15, 16, 17, 33) if (c.D, c.H) == (192, 256) else (c.B,)):
            out.append(pytest.param(c, nb, id=f"{c.name[:-len(str(c.B))]}{nb}"))
    return out


@pytest.mark.parametrize("case,nb", pinn_pairs())
def test_pinn_rollout_bitwise(hf, case, nb):
    """PINN.rollout at T = 6 and T = 1, forward() (one step), T = 0 and the
    scored call on the first nb ICs of the case (B = 15, 17, 33 leave a partial
    group of 16)."""
    b = C.find_case(case)
    assert nb <= case.B
    m = load(hf, b)
    s0 = torch.from_numpy(b.state0[:nb]).to(DEV)
    want = b.out[:nb]
    r = m.rollout(s0, T)
    same(r["traj"], want, f"{case.name} B={nb} traj")
    same(r["final"], want[:, -1], "final")
    r1 = m.rollout(s0, 1)
    same(r1["traj"], want[:, :2], f"{case.name} B={nb} T = 1")
    same(m.rollout(s0, T, traj=False)["final"], want[:, -1], "final, traj=False")
    same(m.rollout(s0, 0)["final"], b.state0[:nb], "T = 0")
    with torch.no_grad():
        f = m(s0)
    same(f, want[:, 1], f"{case.name} B={nb} forward()")
    sc = m.rollout(s0, T, metrics=True)
    same(sc["traj"], want, f"{case.name} B={nb} scored traj")
    same(sc["final"], want[:, -1], "scored final")
    check_metrics(sc["metrics"], want)


# --------------------------------------------------------------- PureGNN backward
def pure_backward(m, nf_np, ei, gup, nf_grad=True):
    m.zero_grad()
    nf = torch.from_numpy(nf_np).to(DEV).requires_grad_(nf_grad)
    d = m(nf, ei)
    (d * torch.from_numpy(gup).to(DEV)).sum().backward()
    g = {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    if nf_grad:
        g["node_features"] = nf.grad.detach().cpu().numpy().copy()
    return d, g


@by_kind("pure_bwd")
def test_pure_backward_bitwise(hf, case):
    """PureGNN.forward under autograd and backward() with an integer upstream
    gradient: delta, every parameter gradient and the feature gradient equal the
    float64 autograd through sat (tanh' exactly 1 at z == 0, 0 elsewhere); with
    requires_grad=False on the features the parameter gradients are the same."""
    b = C.find_case(case)
    m = load(hf, b)
    for what, ei in edge_indices(hf, b):
        d, g = pure_backward(m, b.nf, ei, b.gup)
        same(d, b.out, f"{case.name} {what} delta")
        assert set(g) == set(b.grads)
        for k in g:
            same(g[k], b.grads[k], f"{case.name} {what} d {k}")
        d0, g0 = pure_backward(m, b.nf, ei, b.gup, nf_grad=False)
        same(d0, b.out, f"{case.name} {what} delta, features without grad")
        assert set(g0) == set(b.sd)
        for k in g0:
            same(g0[k], b.grads[k], f"{case.name} {what} d {k}, features without grad")


# ------------------------------------------------------------------ PINN backward
@by_kind("pinn_bwd")
def test_pinn_backward_bitwise(hf, case):
    """training.pinn_forward and backward() with an integer upstream gradient:
    the prediction, every parameter gradient and the state gradient."""
    from hybridflux import training
    b = C.find_case(case)
    m = load(hf, b)
    s = torch.from_numpy(b.state0).to(DEV).requires_grad_(True)
    pred = training.pinn_forward(m, s)
    same(pred, b.out, f"{case.name} prediction")
    (pred * torch.from_numpy(b.gup).to(DEV)).sum().backward()
    same(s.grad, b.grads["state"], f"{case.name} d state")
    for k, p in m.named_parameters():
        same(p.grad, b.grads[k], f"{case.name} d {k}")
