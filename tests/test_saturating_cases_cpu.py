"""The saturating-input cases (tests/saturating_cases.py) on the CPU: every case
that tests/test_gpu_saturating_structure.py runs on the PureGNN and PINN
kernels is shown here to be

  * valid (every tanh input is 0 or at least S in size; every GEMM of the
    forward and the backward sums exactly in float32 in any order) and
    non-vacuous (every tanh layer takes -1, 0 and +1 in every IC, every
    parameter tensor has a nonzero gradient in at least 2 % of its entries, a
    rollout's state moves at every step in every IC);
  * tied to the pinned oracles: oracle.pure_gnn_forward, pure_gnn_rollout and
    pinn_forward in torch float32, and float32 autograd of them, give the
    float64 references' values exactly;
  * what tanh_fast computes: the references with the numpy restatement of
    tanh_fast (tests/test_tanh_fast_cpu.py) in place of sign(z), exp and rcp
    off by -1, 0 and +1 ulp, give the same values;
  * sharp: six CPU mutants of the references (W_a / W_b swapped between source
    and destination, a wrap-around neighbour from the next chain of a shared
    128-row tile, one neighbour's message doubled and the other dropped, a PINN
    IC reading its neighbour's input, the PINN's last layer summing half of K
    on rows >= 128, a backward mask of z >= 0) each change at least one output
    of every case they apply to.  No wrong kernel is ever built.

Comparison is by value (-0.0 == +0.0), with no tolerance.
"""
import types

import numpy as np
import pytest
import torch

import saturating_cases as C
from oracle import hybrid_oracle as O
from test_tanh_fast_cpu import _tanh_fast

ALL = pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
GRADS = pytest.mark.parametrize("case", [c for c in C.CASES if c.grads], ids=lambda c: c.name)


def same(got, want, what=""):
    msg = C.mismatch(got, want)
    assert msg is None, f"{what}: {msg}"


def edge_index(b):
    c = b.case
    return torch.from_numpy(b.ei) if b.ei is not None else O.chain_edges(c.nx, c.B)


@ALL
def test_case_is_valid_and_sharp(case):
    b = C.find_case(case)      # raises when no seed of exact_cases.SEEDS qualifies
    assert b.rec.sat_ok and b.rec.max_bound() < 2.0 ** 24, (b.rec.sat_ok, b.rec.max_bound())
    tanh_layers = (case.L + 2) if case.pure else (case.L - 1)
    assert len(b.rec.counts) == tanh_layers and set(b.rec.counts) == set(b.rec.min_ic_share)
    assert all(v > 0 for v in b.rec.min_ic_share.values()), b.rec.min_ic_share
    if case.grads:
        assert b.grec.sat_ok and b.grec.max_bound() < 2.0 ** 24, b.grec.max_bound()
        assert set(b.grec.grad_share) == set(b.sd) | {"node_features" if case.pure else "state"}
        assert all(v >= C.MIN_GRAD_SHARE for v in b.grec.grad_share.values()), b.grec.grad_share
    if case.rollout:
        assert np.any(b.out[:, 1:] != b.out[:, :-1], axis=(2, 3)).all()
    assert C.accept(b) == []


@ALL
def test_oracle_f32_equals_reference64(case):
    b = C.find_case(case)
    p = O.params_from(b.sd)
    n = C.sub_batch(case)
    if case.kind == "pure_roll":
        grid = types.SimpleNamespace(nx=case.nx, x=b.x.astype(np.float64))
        for ic in range(n):
            traj = O.pure_gnn_rollout(p, grid, b.state0[ic], C.T_STEPS)
            assert traj.dtype == np.float32
            same(traj, b.out[ic], f"IC {ic}")
    elif not case.pure:
        s = torch.from_numpy(b.state0[:n])
        with torch.no_grad():
            for t in range(C.T_STEPS if case.rollout else 1):
                s = O.pinn_forward(p, s)
                assert s.dtype == torch.float32
                same(s.numpy(), b.out[:n, t + 1] if case.rollout else b.out[:n], f"step {t + 1}")
    else:
        with torch.no_grad():
            d = O.pure_gnn_forward(p, torch.from_numpy(b.nf), edge_index(b))
        assert d.dtype == torch.float32
        same(d.numpy(), b.out)


@GRADS
def test_autograd_f32_equals_grads64(case):
    b = C.find_case(case)
    p = {k: v.clone().requires_grad_(True) for k, v in O.params_from(b.sd).items()}
    if case.pure:
        x = torch.from_numpy(b.nf).clone().requires_grad_(True)
        out = O.pure_gnn_forward(p, x, edge_index(b))
    else:
        x = torch.from_numpy(b.state0).clone().requires_grad_(True)
        out = O.pinn_forward(p, x)
    (out * torch.from_numpy(b.gup)).sum().backward()
    same(out.detach().numpy(), b.out, "forward")
    same(x.grad.numpy(), b.grads["node_features" if case.pure else "state"], "input gradient")
    for k, v in p.items():
        assert v.grad.dtype == torch.float32
        same(v.grad.numpy(), b.grads[k], k)


@ALL
def test_restated_tanh_fast_equals_sat(case):
    """tanh_fast as the header writes it, with exp and rcp each off by -1, 0 and
    +1 ulp, in place of sign(z), on the first ICs."""
    b = C.find_case(case)
    n = min(C.sub_batch(case), 4)
    want = C.forward(b, ics=n)
    same(want, b.out if case.graph else b.out[:want.shape[0]], "sub-batch")
    for eu in (-1, 0, 1):
        for ru in (-1, 0, 1):
            got = C.forward(b, ics=n, act=lambda z: _tanh_fast(z.astype(np.float32), eu, ru)[0].astype(np.float64))
            same(got, want, f"exp {eu:+d} ulp, rcp {ru:+d} ulp")


@ALL
def test_forward_mutants_are_detected(case):
    b = C.find_case(case)
    n = C.sub_batch(case)
    base = C.forward(b, ics=n)
    for m in case.mutants():
        assert not np.array_equal(C.forward(b, ics=n, mutant=m), base), f"{m} not detected"
    known = C.PURE_MUTANTS if case.pure else C.PINN_MUTANTS
    assert set(case.mutants()) <= set(known)
    if case.pure and case.L >= 1 and not case.graph and case.nx >= 3:
        assert "swap_ab" in case.mutants() and "double_left" in case.mutants()
        assert ("next_chain_wrap" in case.mutants()) == (case.B >= 2 and case.nx < 128 and 128 % case.nx == 0)
    if not case.pure and case.B >= 2:
        assert "next_ic_input" in case.mutants() and (("half_k_tail" in case.mutants()) == (case.D > 128))


@GRADS
def test_backward_mask_mutant_is_detected(case):
    """tanh' taken as (z >= 0) instead of (z == 0): some gradient moves, the forward does not."""
    b = C.find_case(case)
    if case.pure:
        out, grads, _ = C.pure_grads64(b.sd, b.nf, b.gup, case.B, case.nx, edge_index=b.ei, mask_ge=True)
    else:
        out, grads, _ = C.pinn_grads64(b.sd, b.state0, b.gup, mask_ge=True)
    assert np.array_equal(out, b.out)
    assert any(not np.array_equal(grads[k], b.grads[k]) for k in grads)


def test_table_covers_every_dispatch_path():
    """The shapes of the table against the kernels' own dispatch rules
    (csrc/baselines.hip pure_chain_ok, pure_fused_ok, pinn_fused_ok)."""
    chain_ok = lambda c: c.graph is None and 128 % c.nx == 0 and c.H % 64 == 0    # noqa: E731
    fused = lambda c: c.H in (64, 128) and c.nx in (16, 32, 48, 64)               # noqa: E731
    for kind in ("pure_fwd", "pure_bwd"):
        cs = C.cases(kind)
        assert any(chain_ok(c) for c in cs) and any(not chain_ok(c) and not c.graph for c in cs)
        assert any(c.graph for c in cs) and any(c.in_dim == 3 for c in cs)
    assert max(c.L for c in C.cases("pure_bwd")) == 2
    roll = C.cases("pure_roll")
    assert {(c.H, c.nx) for c in roll if fused(c) and c.L == 4} == {(H, nx) for H in (64, 128) for nx in (16, 32, 48, 64)}
    assert {c.L for c in roll if fused(c)} == {0, 1, 4, 8, 10} and any(not fused(c) for c in roll)
    assert {c.B for c in roll if fused(c)} == {5, C.BIG_B}
    pinn = C.cases("pinn_roll")
    assert {c.L for c in pinn if (c.D, c.H) == (192, 256)} == {2, 3, 4, 8} and any(c.D != 192 for c in pinn)
    assert all(c.B == 33 for c in pinn if c.D == 192)


def test_pinn_backward_at_8_layers_is_forbidden_by_the_record():
    """Why PINN_BWD stops at L = 4 on (192, 256): at L = 8 the forward is valid
    but the backward's absolute sums leave float32's 24 bits (first seeds)."""
    case = C.Case("pinn_bwd", 256, 8, 32, D=192)
    for seed in range(3):
        b = C.build(case, seed)
        assert b.rec.valid() and b.grec.sat_ok and b.grec.max_bound() >= 2.0 ** 24 and C.accept(b) != []


def test_record_predicates():
    """The record's own predicates on known values."""
    assert C.pow2_unit([48.0, -16.0, 0.0]) == 16 and C.pow2_unit([3.0, 16.0]) == 1 and C.pow2_unit([0.0]) == 1
    a, w = np.array([[16.0, 0.0], [-32.0, 16.0]]), np.array([[2.0, 6.0]])
    assert C.gemm_bound([a], [w], np.array([64.0])) == (32 * 2 + 16 * 6 + 64) / 32
    rec = C.SatRecord()
    assert rec.note_tanh("l", np.array([[0.0, 16.0, -32.0]]), 1) and rec.valid()
    assert rec.shares()["l"] == (1 / 3, 1 / 3, 1 / 3) and rec.min_ic_share["l"] == 1 / 3
    assert not rec.note_tanh("l", np.array([[0.0, 8.0, -32.0]]), 1) and not rec.valid()   # 0 < 8 < S
    rec = C.SatRecord()
    rec.note_tanh("l", np.array([[0.0, 16.0, -16.0], [16.0, 16.0, 0.0]]), 2)              # IC 1 never takes -1
    assert rec.min_ic_share["l"] == 0
    rec.note_bound("g", 2.0 ** 24)
    assert not rec.valid()
    sd = C.make_pure_sd(4, 64, 1, 0)
    nf = C.ternary((32, 4), 0)
    nf[0, 0] = 0.5                                                                         # not an integer input
    with pytest.raises(AssertionError):
        C.pure_forward64(sd, nf, 2, 16)
