"""Saturating-input cases of the PureGNN and PINN kernels (a plain helper module).

PureGNN and PINN are tanh MLPs, and tanh blocks the small-integer trick of
tests/exact_cases.py unless it saturates.  Here every layer that feeds a tanh
has weights and a bias in S * {small integers} (S = 16) and integer inputs, so
every pre-activation is 0 or has |z| >= S:

  * tanh(0) = 0 exactly, and both device tanhs return exactly +-1 from far
    below S on: tanh_fast (csrc/hf_device.h) once 2 rcp(1 + e) < 2^-25, that is
    from |x| = 9.02 (its numpy restatement, with exp and rcp each one ulp off in
    the worst direction: from 9.015); the device libm tanhf at +-16, +-32, ...
    is the premise test of tests/test_gpu_saturating_structure.py, which passed
    at S = 16 (no doubling was needed);
  * activations are therefore in {-1, 0, 1}, PureGNN's residual h stays a small
    integer (|h| <= 1 + 2L on a chain), the last linear layer (no tanh behind
    it) has plain integer weights, rollout states stay small integers, and
    every float32 partial sum is exact in any order;
  * backward: 1 - y*y is exactly 1 where z == 0 and exactly 0 elsewhere, so
    with an integer upstream gradient every gradient is an integer.  They grow
    by S per tanh layer; PureGNN's residual path mixes the scales, which limits
    its backward cases to L <= 2 (the ratio largest / smallest nonzero addend
    must stay below 2^24), PINN's layers each share one power-of-16 unit.

The references are a plain float64 forward with sat(z) = sign(z), which asserts
z == 0 or |z| >= S at every tanh, and float64 autograd through a function with
forward sign(z) and backward g * (z == 0).  Each fills a record: (a) the
saturation of every tanh input, (b) per GEMM of the forward and the backward
sum |a||b| + |bias| in units of the largest power of two that divides every
addend (below 2^24: exact in float32 in any order), (c) per tanh layer the
shares of -1, 0, +1, (d) per parameter tensor the share of nonzero gradient
entries.  A case is valid when (a) and (b) hold, and non-vacuous when every
tanh layer takes all three values in every IC, every parameter tensor has a
nonzero gradient in at least 2 % of its entries and a rollout's state changes
at every step in every IC.  find_case takes the first such seed on the CPU
only; CASES is the one table tests/test_saturating_cases_cpu.py and
tests/test_gpu_saturating_structure.py both run.
"""
import numpy as np
import torch

import exact_cases as X
from exact_cases import F32_EXACT, Record, _sparse_rows, chain_edges, mismatch  # noqa: F401 (mismatch: for the tests)

S = 16.0            # the scale of every layer that feeds a tanh
MIN_GRAD_SHARE = 0.02
PM1 = (-1.0, 1.0)


# ------------------------------------------------------------------------- inputs
def _ints(g, lo, hi, shape):
    return g.integers(lo, hi + 1, shape).astype(np.float64)


def make_pure_sd(in_dim, H, L, seed):
    """PureGNN(in_dim, H, L) state dict (reference keys): every tanh layer's
    rows hold 2 nonzeros of +-S and its bias is S * {-1, 0, 1}; output_mlp.2
    (no tanh behind it) has 4 nonzeros of +-1 per row and a bias in {-1, 0, 1}."""
    g = np.random.default_rng([seed, in_dim, H, L, 1])
    sd = {"input_mlp.0.weight": S * _sparse_rows(g, H, in_dim, 2, PM1), "input_mlp.0.bias": S * _ints(g, -1, 1, H)}
    for l in range(L):
        sd[f"update_mlps.{l}.0.weight"] = S * _sparse_rows(g, H, 2 * H, 2, PM1)
        sd[f"update_mlps.{l}.0.bias"] = S * _ints(g, -1, 1, H)
    sd["output_mlp.0.weight"] = S * _sparse_rows(g, H, H, 2, PM1)
    sd["output_mlp.0.bias"] = S * _ints(g, -1, 1, H)
    sd["output_mlp.2.weight"] = _sparse_rows(g, 3, H, 4, PM1)
    sd["output_mlp.2.bias"] = _ints(g, -1, 1, 3)
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


def make_pinn_sd(D, H, L, seed):
    """PINN(D, H, L) state dict (reference keys net.0, net.2, ...): the L - 1
    tanh layers as in make_pure_sd, the last layer 3 nonzeros of +-1 per row."""
    g = np.random.default_rng([seed, D, H, L, 2])
    dims = [D] + [H] * (L - 1) + [D]
    sd = {}
    for j in range(L):
        last = j == L - 1
        W = _sparse_rows(g, dims[j + 1], dims[j], 3 if last else 2, PM1)
        b = _ints(g, -1, 1, dims[j + 1])
        sd[f"net.{2 * j}.weight"] = W if last else S * W
        sd[f"net.{2 * j}.bias"] = b if last else S * b
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


def ternary(shape, seed, tag=0):
    """Integer features / states / x column in {-1, 0, 1}, i.i.d. (not smooth)."""
    g = np.random.default_rng([seed, tag, 55] + [int(s) for s in shape])
    return g.integers(-1, 2, shape).astype(np.float32)


def upstream(shape, seed):
    """Integer upstream gradient in {-2..2}."""
    return X.upstream(int(np.prod(shape)), seed).reshape(shape)


def random_graph():
    """(N, edge_index [2, 128]): 64 nodes, the last 8 isolated, 116 random edges
    among the others, 4 self-loops and 8 duplicates of earlier edges."""
    g = np.random.default_rng(7)
    e = g.integers(0, 56, (2, 116))
    loops = np.array([[3, 10, 10, 41], [3, 10, 10, 41]])
    ei = np.concatenate([e, loops, e[:, :8]], axis=1)
    return 64, np.ascontiguousarray(ei[:, g.permutation(ei.shape[1])]).astype(np.int64)


def pure_layers(sd):
    return sum(1 for k in sd if k.startswith("update_mlps.") and k.endswith(".0.weight"))


def pinn_layers(sd):
    return sum(1 for k in sd if k.endswith(".weight"))


# ------------------------------------------------------------------------- record
def pow2_unit(*arrays):
    """The largest power of two that divides every nonzero entry (integers)."""
    bits = 0
    for a in arrays:
        a = np.abs(np.asarray(a, np.float64)).reshape(-1)
        if a.size:
            assert a.max() < 2.0 ** 62, "too large for an int64"
            i = a.astype(np.int64)
            assert np.array_equal(i, a), "not an integer tensor"
            bits |= int(np.bitwise_or.reduce(i))      # zeros add no bit
    return float(bits & -bits) if bits else 1.0


def gemm_bound(xs, Ws, b=None):
    """max over outputs of sum |a||w| + |bias| (bounded from above through the
    column maxima of |a|), in units of the largest power of two that divides
    every addend (bounded from below by unit(a) * unit(w) and unit(bias))."""
    tot = sum(np.abs(a).max(0) @ np.abs(w).T for a, w in zip(xs, Ws) if a.size)
    units = [pow2_unit(a) * pow2_unit(w) for a, w in zip(xs, Ws)]
    unit = min(units + ([pow2_unit(b)] if b is not None and np.any(b) else []))
    if b is not None:
        tot = tot + np.abs(b)
    return float(np.max(tot)) / unit if np.size(tot) else 0.0


class SatRecord(Record):
    """exact_cases.Record plus (a) sat_ok, (c) shares / min_ic_share per tanh
    layer, (d) grad_share per parameter tensor; bound holds (b), in units."""

    def __init__(self):
        super().__init__()
        self.sat_ok = True
        self.counts = {}         # per tanh layer: counts of -1, 0, +1
        self.min_ic_share = {}   # per tanh layer: the smallest share of a value within one IC
        self.grad_share = {}

    def shares(self):
        return {k: tuple(float(c) / max(v.sum(), 1) for c in v) for k, v in self.counts.items()}

    def note_bound(self, name, value):
        self.bound[name] = max(self.bound.get(name, 0.0), float(value))

    def note_tanh(self, name, z, ics):
        ok = bool(np.all((z == 0) | (np.abs(z) >= S)))
        self.sat_ok &= ok
        z = z.reshape(ics, -1)
        neg, zero = (z < 0).sum(1), (z == 0).sum(1)
        per_ic = np.stack([neg, zero, z.shape[1] - neg - zero]).astype(float)      # counts of -1, 0, +1 per IC
        self.counts[name] = self.counts.get(name, np.zeros(3)) + per_ic.sum(1)
        self.min_ic_share[name] = min(self.min_ic_share.get(name, 1.0), float(per_ic.min()) / max(z.shape[1], 1))
        return ok

    def valid(self, precision="f32"):
        return bool(self.sat_ok and self.max_bound() < F32_EXACT)


# ---------------------------------------------------------------------- references
def _act(rec, name, z, ics, act):
    """sat(z) = sign(z) with the saturation asserted; act (tests only): another
    tanh, float64 -> float64, in its place (the restated tanh_fast)."""
    if rec is not None:
        rec.note_tanh(name, z, ics)
    assert np.all((z == 0) | (np.abs(z) >= S)), f"{name}: a tanh input with 0 < |z| < {S}"
    return np.sign(z) if act is None else act(z)


def _linear(rec, name, xs, Ws, b):
    if rec is not None:
        rec.note_bound(name, gemm_bound(xs, Ws, b))
    return sum(a @ w.T for a, w in zip(xs, Ws)) + b


PURE_MUTANTS = ("swap_ab", "next_chain_wrap", "double_left")
PINN_MUTANTS = ("next_ic_input", "half_k_tail")


def pure_forward64(sd, nf, B=1, nx=None, edge_index=None, rec=None, mutant=None, act=None):
    """Plain numpy float64 PureGNN forward (scripts/training/train_pure_gnn.py:57-76)
    on B periodic chains of nx cells, or on the graph edge_index [2, E] (one IC):
    h = sat(W_in x + b); per layer the messages sat([W_a | W_b] [h_src ; h_dst] + b)
    summed at dst and added to h; delta = W_o2 sat(W_o1 h + b_o1) + b_o2 [N, 3].

    CPU mutants (tests only): "swap_ab": W_a is applied to the destination and
    W_b to the source.  "next_chain_wrap": the message a chain's last cell gets
    over the wrap-around edge comes from the first cell of the NEXT chain, where
    the two lie in one 128-row tile.  "double_left": every cell's message from
    its left neighbour counts twice and the one from its right neighbour is
    dropped."""
    W = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    L = pure_layers(sd)
    x = np.asarray(nf, np.float64).reshape(-1, W["input_mlp.0.weight"].shape[1])
    N = x.shape[0]
    chain = edge_index is None
    ei = chain_edges(nx, B) if chain else np.asarray(edge_index)
    src, dst = ei[0].copy(), ei[1]
    ics = B if chain else 1
    if chain:
        cell = np.arange(nx)
        assert np.array_equal(dst.reshape(B, 2 * nx) - (np.arange(B) * nx)[:, None],
                              np.broadcast_to(np.concatenate([(cell + 1) % nx, cell]), (B, 2 * nx)))
    if mutant == "next_chain_wrap":
        assert chain
        for b in range(B - 1):
            nxt = (b + 1) * nx
            if nxt // 128 == (nxt - 1) // 128:
                e = b * 2 * nx + 2 * nx - 1          # the edge cell 0 -> cell nx-1 of chain b
                assert src[e] == b * nx and dst[e] == nxt - 1
                src[e] = nxt
    h = _act(rec, "input", _linear(rec, "input", [x], [W["input_mlp.0.weight"]], W["input_mlp.0.bias"]), ics, act)
    H = h.shape[1]
    for l in range(L):
        Wl = W[f"update_mlps.{l}.0.weight"]
        # [W_a | W_b] [h_src ; h_dst] = (W_a h)[src] + (W_b h)[dst]: one product per node, gathered per edge
        if rec is not None:
            rec.note_bound(f"layer{l}", gemm_bound([h, h], [Wl[:, :H], Wl[:, H:]], W[f"update_mlps.{l}.0.bias"]))
        P, Q = h @ Wl[:, :H].T, h @ Wl[:, H:].T
        z = (P[dst] + Q[src] if mutant == "swap_ab" else P[src] + Q[dst]) + W[f"update_mlps.{l}.0.bias"]
        upd = _act(rec, f"layer{l}", z, ics, act)
        if mutant == "double_left":
            assert chain
            upd = upd.reshape(B, 2 * nx, H).copy()
            upd[:, :nx] *= 2
            upd[:, nx:] = 0
            upd = upd.reshape(-1, H)
        if chain:    # dst is cell i+1 for the first nx edges of an IC and cell i for the others
            u3 = upd.reshape(B, 2 * nx, H)
            agg = (np.roll(u3[:, :nx], 1, axis=1) + u3[:, nx:]).reshape(N, H)
        else:
            agg = np.zeros_like(h)
            np.add.at(agg, dst, upd)
        h = h + agg
        if rec is not None:
            rec.max_act = max(rec.max_act, float(np.abs(h).max()))
    o = _act(rec, "out0", _linear(rec, "out0", [h], [W["output_mlp.0.weight"]], W["output_mlp.0.bias"]), ics, act)
    delta = _linear(rec, "out2", [o], [W["output_mlp.2.weight"]], W["output_mlp.2.bias"])
    assert delta.shape == (N, 3)
    return delta


def pure_rollout64(sd, state0, x, T, rec=None, mutant=None, act=None):
    """evaluate_multi_ic.py:53-64 for B ICs: state [B,3,nx] -> traj [B,T+1,3,nx]
    with node features [n, u, E, x] and state += delta."""
    s = np.asarray(state0, np.float64)
    B, _, nx = s.shape
    xc = np.broadcast_to(np.asarray(x, np.float64)[None, :, None], (B, nx, 1))
    out = [s]
    for _ in range(T):
        nf = np.concatenate([s.transpose(0, 2, 1), xc], axis=2).reshape(B * nx, 4)
        d = pure_forward64(sd, nf, B, nx, rec=rec, mutant=mutant, act=act)
        s = s + d.reshape(B, nx, 3).transpose(0, 2, 1)
        out.append(s)
    return np.stack(out, axis=1)


def pinn_forward64(sd, state, rec=None, mutant=None, act=None):
    """train_pinn.py:48-61: state [B,3,nx] -> state + net(flat state), float64.

    CPU mutants (tests only): "next_ic_input": IC b reads the layer-0 input of
    IC b+1 where both lie in one group of 16.  "half_k_tail": the last layer's
    output rows at or above 128 sum only the first half of K."""
    W = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    L = pinn_layers(sd)
    s = np.asarray(state, np.float64)
    B = s.shape[0]
    z = s.reshape(B, -1)
    if mutant == "next_ic_input":
        b = np.arange(B)
        z = z[np.where(((b + 1) % 16 != 0) & (b + 1 < B), b + 1, b)]
    for j in range(L - 1):
        z = _act(rec, f"net{2 * j}", _linear(rec, f"net{2 * j}", [z], [W[f"net.{2 * j}.weight"]], W[f"net.{2 * j}.bias"]),
                 B, act)
    Wl, bl = W[f"net.{2 * (L - 1)}.weight"], W[f"net.{2 * (L - 1)}.bias"]
    d = _linear(rec, f"net{2 * (L - 1)}", [z], [Wl], bl)
    if mutant == "half_k_tail":
        K = Wl.shape[1] // 2
        d[:, 128:] = z[:, :K] @ Wl[128:, :K].T + bl[128:]
    return s + d.reshape(s.shape)


def pinn_rollout64(sd, state0, T, rec=None, mutant=None, act=None):
    """evaluate_multi_ic.py:75-81: traj [B,T+1,3,nx]."""
    out = [np.asarray(state0, np.float64)]
    for _ in range(T):
        out.append(pinn_forward64(sd, out[-1], rec=rec, mutant=mutant, act=act))
    return np.stack(out, axis=1)


class _Sat(torch.autograd.Function):
    """forward sign(z), backward g * (z == 0): tanh on saturating inputs, where
    1 - y*y is exactly 1 at z == 0 and exactly 0 elsewhere.  mask_ge (CPU
    mutant): the mask is z >= 0."""

    @staticmethod
    def forward(ctx, z, mask_ge):
        assert bool(((z == 0) | (z.abs() >= S)).all()), "a tanh input with 0 < |z| < S"
        ctx.save_for_backward(z)
        ctx.mask_ge = mask_ge
        return torch.sign(z)

    @staticmethod
    def backward(ctx, g):
        (z,) = ctx.saved_tensors
        return g * ((z >= 0) if ctx.mask_ge else (z == 0)).to(g.dtype), None


def _backward_record(rec, maps, extra, grads):
    """(b) of the backward: per linear map |dy|^T |a| (weight gradient), sum |dy|
    (bias gradient) and |dy| |W| (data gradient), and every elementwise sum of
    gradients (extra: tensors whose .grad adds several terms), in units; (d)."""
    for name, a, Wm, y in maps:
        dy, a, Wm = y.grad.numpy(), a.detach().numpy(), Wm.detach().numpy()
        if not dy.size or not np.any(dy):
            continue
        u = pow2_unit(dy)
        rec.note_bound(name + ".dW", float((np.abs(dy).T @ np.abs(a)).max()) / (u * pow2_unit(a)))
        rec.note_bound(name + ".db", float(np.abs(dy).sum(0).max()) / u)
        rec.note_bound(name + ".dx", float((np.abs(dy) @ np.abs(Wm)).max()) / (u * pow2_unit(Wm)))
    for name, t in extra:
        g = t.grad.numpy()
        if np.any(g):   # a sum of terms that are each a multiple of its unit or of a larger power of two
            rec.note_bound(name + ".sum", float(np.abs(g).max()) / pow2_unit(g))
    for k, g in grads.items():
        assert np.array_equal(np.rint(g), g), f"gradient of {k} is not an integer tensor"
        rec.grad_share[k] = float(np.mean(g != 0))


def pure_grads64(sd, nf, gup, B=1, nx=None, edge_index=None, mask_ge=False):
    """float64 torch autograd of the PureGNN forward through _Sat with upstream
    gradient gup [N, 3].  Returns (delta [N,3], grads: every parameter's and
    "node_features"' gradient as float64 numpy, SatRecord of the backward)."""
    f64 = torch.float64
    p = {k: torch.tensor(np.asarray(v, np.float64), dtype=f64, requires_grad=True) for k, v in sd.items()}
    L = pure_layers(sd)
    x = torch.tensor(np.asarray(nf, np.float64), dtype=f64, requires_grad=True)
    ei = torch.from_numpy(chain_edges(nx, B) if edge_index is None else np.asarray(edge_index, np.int64))
    src, dst = ei[0], ei[1]
    maps, extra = [], []

    def layer(name, a, Wk, bk, sat=True):
        y = a @ p[Wk].T + p[bk]
        y.retain_grad()
        maps.append((name, a, p[Wk], y))
        return _Sat.apply(y, mask_ge) if sat else y

    h = layer("input", x, "input_mlp.0.weight", "input_mlp.0.bias")
    for l in range(L):
        h.retain_grad()
        extra.append((f"h{l}", h))
        upd = layer(f"layer{l}", torch.cat([h[src], h[dst]], -1), f"update_mlps.{l}.0.weight", f"update_mlps.{l}.0.bias")
        h = h + torch.zeros_like(h).index_add_(0, dst, upd)
    o = layer("out0", h, "output_mlp.0.weight", "output_mlp.0.bias")
    delta = layer("out2", o, "output_mlp.2.weight", "output_mlp.2.bias", sat=False)
    (delta * torch.tensor(np.asarray(gup, np.float64))).sum().backward()
    grads = {k: v.grad.numpy().copy() for k, v in p.items()}
    grads["node_features"] = x.grad.numpy().copy()
    rec = SatRecord()
    _backward_record(rec, maps, extra, grads)
    return delta.detach().numpy().copy(), grads, rec


def pinn_grads64(sd, state, gup, mask_ge=False):
    """float64 torch autograd of state + net(state) through _Sat with upstream
    gradient gup [B,3,nx].  Returns (out, grads: every parameter's and "state"'s
    gradient, SatRecord of the backward)."""
    f64 = torch.float64
    p = {k: torch.tensor(np.asarray(v, np.float64), dtype=f64, requires_grad=True) for k, v in sd.items()}
    L = pinn_layers(sd)
    s = torch.tensor(np.asarray(state, np.float64), dtype=f64, requires_grad=True)
    z = s.reshape(s.shape[0], -1)
    maps = []
    for j in range(L):
        y = z @ p[f"net.{2 * j}.weight"].T + p[f"net.{2 * j}.bias"]
        y.retain_grad()
        maps.append((f"net{2 * j}", z, p[f"net.{2 * j}.weight"], y))
        z = _Sat.apply(y, mask_ge) if j < L - 1 else y
    out = s + z.reshape(s.shape)
    (out * torch.tensor(np.asarray(gup, np.float64))).sum().backward()
    grads = {k: v.grad.numpy().copy() for k, v in p.items()}
    grads["state"] = s.grad.numpy().copy()
    rec = SatRecord()
    _backward_record(rec, maps, [("state", s)], grads)
    return out.detach().numpy().copy(), grads, rec


# --------------------------------------------------------------------- case table
T_STEPS = 6


class Case:
    """One row of the table.  kind: "pure_fwd" (PureGNN.forward), "pure_roll"
    (PureGNN.rollout), "pure_bwd" (PureGNN under autograd), "pinn_roll"
    (PINN.rollout and forward), "pinn_bwd" (training.pinn_forward).  PureGNN:
    H, nx, B, L, in_dim, graph ("random" or None: B chains of nx cells); PINN:
    D, H, L, B.  The GPU tests also run the first ICs of a case as sub-batches."""

    def __init__(self, kind, H, L, B, nx=None, D=None, in_dim=4, graph=None):
        self.kind, self.H, self.L, self.B, self.nx, self.D, self.in_dim, self.graph = kind, H, L, B, nx, D, in_dim, graph
        self.pure = kind.startswith("pure")
        self.seed0 = 0
        if self.pure:
            shape = "graph" if graph else f"nx{nx}_B{B}"
            self.name = f"sat_{kind}_H{H}_{shape}_L{L}" + (f"_F{in_dim}" if in_dim != 4 else "")
        else:
            self.name = f"sat_{kind}_D{D}_H{H}_L{L}_B{B}"
            self.nx = D // 3

    def __repr__(self):
        return self.name

    @property
    def grads(self):
        return self.kind.endswith("bwd")

    @property
    def rollout(self):
        return self.kind.endswith("roll")

    def edge_index(self):
        return random_graph()[1] if self.graph else None

    def nodes(self):
        return random_graph()[0] if self.graph else self.B * self.nx

    def ics(self):
        return 1 if self.graph else self.B

    def mutants(self):
        """The forward mutants that can change this case's outputs."""
        if not self.pure:
            return [m for m, ok in zip(PINN_MUTANTS, (self.B >= 2, self.D > 128)) if ok]
        if self.L == 0:
            return []
        if self.graph:
            return ["swap_ab"]
        nx = self.nx   # nx = 1: source = destination; nx <= 2: both messages of a cell are the same one
        return [m for m, ok in zip(PURE_MUTANTS, (nx >= 2, self.B >= 2 and nx < 128 and 128 % nx == 0, nx >= 3)) if ok]


class Built:
    """A case with its seed chosen: inputs, float64 references and records."""


def forward(b, mutant=None, act=None, rec=None, ics=None):
    """The case's float64 reference output (of its first `ics` ICs): delta
    [N,3] (pure_fwd, pure_bwd), traj [B,T+1,3,nx] (rollouts), out [B,3,nx]
    (pinn_bwd)."""
    c = b.case
    n = c.B if ics is None else ics
    if c.kind == "pure_roll":
        return pure_rollout64(b.sd, b.state0[:n], b.x, T_STEPS, rec=rec, mutant=mutant, act=act)
    if c.kind == "pinn_roll":
        return pinn_rollout64(b.sd, b.state0[:n], T_STEPS, rec=rec, mutant=mutant, act=act)
    if c.kind == "pinn_bwd":
        return pinn_forward64(b.sd, b.state0[:n], rec=rec, mutant=mutant, act=act)
    if c.graph:
        return pure_forward64(b.sd, b.nf, edge_index=b.ei, rec=rec, mutant=mutant, act=act)
    return pure_forward64(b.sd, b.nf[:n * c.nx], n, c.nx, rec=rec, mutant=mutant, act=act)


def sub_batch(case):
    """ICs the CPU mutants and oracle comparisons run on (the first ones: ICs
    are independent in the reference).  Two chains past the first 128-row tile
    at least, and past the first group of 16 ICs of the PINN."""
    if case.graph:
        return 1
    return min(case.B, 20 if not case.pure else max(4, 256 // case.nx + 2))


def build(case, seed):
    """Inputs, references and records of `case` at `seed` (no acceptance test)."""
    b = Built()
    b.case, b.seed = case, seed
    b.ei = case.edge_index()
    b.rec = SatRecord()
    b.gup = b.grads = b.grec = None
    if case.pure:
        b.sd = make_pure_sd(case.in_dim, case.H, case.L, seed)
        if case.rollout:
            b.state0, b.x = ternary((case.B, 3, case.nx), seed, 1), ternary((case.nx,), seed, 2)
        else:
            b.nf = ternary((case.nodes(), case.in_dim), seed, 3)
    else:
        b.sd = make_pinn_sd(case.D, case.H, case.L, seed)
        b.state0 = ternary((case.B, 3, case.nx), seed, 4)
    b.out = forward(b, rec=b.rec)
    if case.grads:
        b.gup = upstream(b.out.shape, seed)
        if case.pure:
            out, b.grads, b.grec = pure_grads64(b.sd, b.nf, b.gup, case.B, case.nx, edge_index=b.ei)
        else:
            out, b.grads, b.grec = pinn_grads64(b.sd, b.state0, b.gup)
        assert np.array_equal(out, b.out), "the autograd forward and the numpy forward disagree"
        b.rec.grad_share = b.grec.grad_share
    return b


def nonvacuous(b):
    """The conditions of a sharp case (conditions, not measurements): returns
    the list of those that fail."""
    bad = [f"tanh layer {k} misses a value of (-1, 0, 1) in some IC" for k, v in b.rec.min_ic_share.items() if v <= 0]
    if b.case.grads:
        bad += [f"gradient of {k}: nonzero share {v:.4f} < {MIN_GRAD_SHARE}" for k, v in b.grec.grad_share.items()
                if v < MIN_GRAD_SHARE]
    if b.case.rollout:
        moved = np.any(b.out[:, 1:] != b.out[:, :-1], axis=(2, 3))
        if not moved.all():
            bad.append(f"the state stands still at {int((~moved).sum())} (IC, step) pairs")
    return bad


def accept(b):
    """Why this seed is not taken ([] = taken): validity (a), (b) of the
    forward and of the backward, then non-vacuity."""
    bad = []
    for name, rec in (("forward", b.rec), ("backward", b.grec)):
        if rec is not None and not rec.valid():
            bad.append(f"{name}: saturated {rec.sat_ok}, bound {rec.max_bound():.3g} of 2^24 = {F32_EXACT:.3g}")
    return bad or nonvacuous(b)


def find_case(case):
    """The case at the first valid, non-vacuous seed (exact_cases' search and
    cache with this module's build and accept).  CPU only."""
    return X.find_case(case, build, accept)


# PureGNN.forward: tagged chains on the chain GEMMs (nx | 128 and H % 64 == 0) ...
PURE_FWD_CHAIN = [(64, 16, 9, 3), (128, 64, 3, 4), (64, 128, 2, 2), (192, 32, 5, 1), (64, 1, 3, 1), (64, 2, 4, 1)]
PURE_FWD_GENERIC = [(64, 48, 3, 3), (128, 100, 2, 2), (32, 16, 3, 2)]     # ... and on the generic path (H, nx, B, L)
# PureGNN under autograd: CHAIN_CASES of test_gpu_pure_gnn_training.py, L capped at 2 (H, nx, L, B, in_dim)
PURE_BWD = [(64, 16, 2, 9, 4), (128, 64, 2, 3, 4), (64, 128, 2, 2, 4), (64, 64, 2, 9, 4), (192, 32, 1, 5, 4),
            (64, 48, 2, 3, 4), (128, 100, 2, 2, 4), (32, 16, 2, 3, 4), (64, 32, 0, 2, 4), (64, 1, 1, 3, 4),
            (64, 2, 1, 4, 4), (64, 16, 2, 3, 3)]
# PINN backward (D, H, L, B).  (192, 256, 8, 32) is not here: the record forbids it at every seed (the backward's
# absolute sums reach 2^31 units of the smallest addend, float32 holds 2^24)
PINN_BWD = [(192, 256, 4, 32), (192, 256, 2, 5), (96, 64, 3, 130), (144, 96, 3, 7)]
BIG_B = 600   # more one-IC workgroups than are resident at once


def _table():
    T = []
    for H, nx, B, L in PURE_FWD_CHAIN + PURE_FWD_GENERIC:
        T.append(Case("pure_fwd", H, L, B, nx=nx))
    T.append(Case("pure_fwd", 64, 2, 3, nx=16, in_dim=3))
    T.append(Case("pure_fwd", 64, 3, 1, graph="random"))
    # the one-launch rollout: the full cross at L = 4, the other depths at two corners (L = 10: nn.Linear rows);
    # B = 600 at the two corners, 5 elsewhere; the GPU tests also run the first 1 and 5 ICs alone
    for H in (64, 128):
        for nx in (16, 32, 48, 64):
            T.append(Case("pure_roll", H, 4, BIG_B if (H, nx) in ((64, 16), (128, 64)) else 5, nx=nx))
    for H, nx in ((64, 32), (128, 64)):
        for L in (0, 1, 8, 10):
            T.append(Case("pure_roll", H, L, 5, nx=nx))
    for H, nx in ((64, 100), (32, 16)):     # the per-step kernels
        T.append(Case("pure_roll", H, 2, 3, nx=nx))
    for H, nx, L, B, F in PURE_BWD:
        T.append(Case("pure_bwd", H, L, B, nx=nx, in_dim=F))
    T.append(Case("pure_bwd", 64, 2, 1, graph="random"))
    # PINN: the one-launch kernel at every depth (the GPU tests run B = 1, 15, 16, 17, 33 of these 33 ICs)
    for L in (2, 3, 4, 8):
        T.append(Case("pinn_roll", 256, L, 33, D=192))
    for D, H, L, B in ((96, 64, 3, 7), (63, 40, 3, 5)):
        T.append(Case("pinn_roll", H, L, B, D=D))
    for D, H, L, B in PINN_BWD:
        T.append(Case("pinn_bwd", H, L, B, D=D))
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases(kind):
    return [c for c in CASES if c.kind == kind]
