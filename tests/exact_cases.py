"""Exact-input cases of the FluxGNN kernels (a plain helper module).

FluxGNN is ReLU plus linear maps.  With small-integer features and sparse
small-integer weights every value of the forward (and of the backward with an
integer upstream gradient) is a dyadic rational of bounded size, so

  * every GEMM input is exactly representable in float32, bf16 and the fp16
    hi+lo split, and
  * every float32 partial sum is exact whatever the summation order,

and every kernel family, in every precision, must reproduce a plain float64
forward BIT FOR BIT: accumulation order, split-K, the P/Q split of the readout
and the mean written as a division or as a reciprocal cannot matter.  The
features are i.i.d. per cell (deliberately rough), so a wrong neighbour, a
stale seam slot or an index off by one moves the flux by O(1).

`forward64` / `grads64` are the references and also return the RECORD that
decides whether a case is valid for a precision; `find_case` searches seeds on
the CPU only (nothing from the GPU enters the choice of inputs).  CASES is the
one table tests/test_exact_cases_cpu.py (validity, agreement with the pinned
oracle, non-vacuity, mutants) and tests/test_gpu_exact_structure.py (the
kernels) both run.
"""
import numpy as np
import torch

F32_EXACT = float(2 ** 24)   # integers below it, and their sums, are exact in float32
SEEDS = 32                   # find_case tries seeds 0 .. SEEDS-1

# super-window geometry of the bf16 flux kernel (csrc/chain_bf16.hip chain_flux_sw_kernel)
SW_WAVES, SW_STRIDE = 8, 63


def sw_segment(nx, layers):
    """Cells of one IC's padded segment in the super-window stream."""
    return nx + 2 * layers + 1


def sw_faces(layers):
    """Exact faces of one 8-wave super-window."""
    return SW_STRIDE * SW_WAVES - 2 * layers


def sw_count(layers, B, nx):
    faces = sw_faces(layers)
    return (B * sw_segment(nx, layers) + faces - 1) // faces


def win_faces(layers):
    """Exact faces of one 64-cell window of the f32 / f16x3 windowed kernels
    (csrc/hf_internal.h win_faces_of, chain_common.h launch_flux_windowed)."""
    return 64 - 2 * layers - 1


# ------------------------------------------------------------------ number formats
def bf16_round(a):
    """float64 -> nearest bfloat16 (ties to even), as float64."""
    a32 = np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))
    u = a32.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_exact(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(bf16_round(a), a))


def f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def f16x3_exact(a):
    """v == f16(v) + f16(v - f16(v)) and |v| < 65504: the fp16 hi+lo split holds v."""
    a = np.asarray(a, np.float64)
    if a.size and np.abs(a).max() >= 65504:
        return False
    hi = f16(a)
    return bool(np.array_equal(hi + f16(a - hi), a))


def f16_exact(a):
    """fp16-exact with a zero low part (the f16x3 kernels drop the lo*lo product)."""
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(f16(a), a))


def dyadic_bits(*arrays):
    """Smallest m such that every value of every array is a multiple of 2^-m."""
    m = 0
    for a in arrays:
        a = np.asarray(a, np.float64)
        while m < 40:
            s = a if m == 0 else a * 2.0 ** m
            if np.array_equal(np.rint(s), s):
                break
            m += 1
    return m


# ------------------------------------------------------------------------- inputs
def n_layers(sd):
    return sum(1 for k in sd if k.startswith("update_mlps.") and k.endswith(".0.weight"))


def _sparse_rows(g, rows, cols, k, values):
    W = np.zeros((rows, cols))
    k = min(k, cols)
    for r in range(rows):
        c = g.choice(cols, size=k, replace=False)
        W[r, c] = g.choice(values, size=k)
    return W


def make_sd(layers, seed, hidden=128, in_dim=4, ka=None, kb=1, zero_x=False, kin=2, ke=2):
    """Sparse small-integer FluxGNN(in_dim, hidden, layers) state dict (reference
    keys): input weights kin nonzeros +-1 per row, W_a ka nonzeros +-1 (default 2,
    1 from 8 layers on), W_b kb nonzeros +-2 (W_b/2 = +-1: the mean aggregation
    stays on multiples of 1/2), edge weights ke + ke nonzeros +-1, small integer
    biases, edge_mlp.2.weight in {-2..2}, edge_mlp.2.bias 1.  zero_x: column 3
    of the input weights is zero (the rollouts' x is not an integer)."""
    g = np.random.default_rng([seed, layers, hidden])
    if ka is None:
        ka = 1 if layers >= 8 else 2
    H = hidden
    sd = {"input_mlp.0.weight": _sparse_rows(g, H, in_dim - 1 if zero_x else in_dim, kin, (-1.0, 1.0)),
          "input_mlp.0.bias": g.integers(-1, 2, H).astype(np.float64)}
    if zero_x:
        sd["input_mlp.0.weight"] = np.concatenate([sd["input_mlp.0.weight"], np.zeros((H, 1))], axis=1)
    for l in range(layers):
        sd[f"update_mlps.{l}.0.weight"] = np.concatenate(
            [_sparse_rows(g, H, H, ka, (-1.0, 1.0)), _sparse_rows(g, H, H, kb, (-2.0, 2.0))], axis=1)
        sd[f"update_mlps.{l}.0.bias"] = g.integers(-2, 2, H).astype(np.float64)
    sd["edge_mlp.0.weight"] = np.concatenate(
        [_sparse_rows(g, H, H, ke, (-1.0, 1.0)), _sparse_rows(g, H, H, ke, (-1.0, 1.0))], axis=1)
    sd["edge_mlp.0.bias"] = g.integers(-1, 2, H).astype(np.float64)
    sd["edge_mlp.2.weight"] = g.integers(-2, 3, (1, H)).astype(np.float64)
    sd["edge_mlp.2.bias"] = np.ones(1)
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


def features(B, nx, seed, hi=4, in_dim=4):
    """[B*nx, in_dim] float32: i.i.d. integers in [0, hi) per cell and feature (not smooth)."""
    g = np.random.default_rng([seed, B, nx, 77])
    return g.integers(0, hi, (B * nx, in_dim)).astype(np.float32)


def upstream(E, seed, quarter=False):
    """Integer upstream gradient [E] in {-2..2} (quarter: nonzero on a quarter of the edges)."""
    g = np.random.default_rng([seed, E, 99])
    gup = g.integers(-2, 3, E).astype(np.float32)
    if quarter:
        gup = gup * (g.integers(0, 4, E) == 0)
    return gup.astype(np.float32)


def chain_edges(nx, B=1):
    """[2, B*2nx] int64 numpy: per IC the edges i -> i+1, then i+1 -> i (reference order)."""
    src = np.arange(nx)
    dst = (src + 1) % nx
    off = (np.arange(B) * nx)[:, None]
    row, col = np.concatenate([src, dst]), np.concatenate([dst, src])
    return np.stack([(row + off).reshape(-1), (col + off).reshape(-1)]).astype(np.int64)


def circulant4_edges(N):
    """Degree-4 circulant graph: i -> i+-1, i+-2 (mod N)."""
    i = np.arange(N)
    row = np.concatenate([i, i, i, i])
    col = np.concatenate([(i + 1) % N, (i - 1) % N, (i + 2) % N, (i - 2) % N])
    return np.stack([row, col]).astype(np.int64)


def mixed_edges():
    """(N, edge_index) of a graph whose out-degrees (what the mean divides by)
    are only 0, 1, 2 and 4: a ring of 9 (degree 2), a pair (degree 1), four
    isolated nodes, a node with four out-edges into nodes that have none, a
    degree-1 tail, and a circulant of 11 (degree 4)."""
    e = []
    for i in range(9):
        e += [(i, (i + 1) % 9), ((i + 1) % 9, i)]
    e += [(9, 10), (10, 9)]
    # 11..14 isolated
    e += [(15, 16), (15, 17), (15, 18), (15, 19)]        # 16..19: out-degree 0, read by 15
    e += [(20, 21), (21, 22)]                            # a tail: 20 and 21 degree 1, 22 degree 0
    for i in range(11):
        e += [(23 + i, 23 + (i + d) % 11) for d in (1, -1, 2, -2)]
    ei = np.array(e, np.int64).T
    order = np.random.default_rng(5).permutation(ei.shape[1])  # edges in no particular order
    return 34, np.ascontiguousarray(ei[:, order])


# ---------------------------------------------------------------------- references
class Record:
    """What forward64 / grads64 saw: representability per precision, the
    absolute-sum bound of every linear map, the dyadic depth m."""

    def __init__(self):
        self.repr_ok = {"f32": True, "bf16": True, "f16x3": True}
        self.bound = {}
        self.m = 0
        self.zero_frac = {}   # per ReLU layer: fraction of pre-activations exactly 0
        self.max_act = 0.0

    def max_bound(self):
        return max(self.bound.values()) if self.bound else 0.0

    def valid(self, precision):
        return bool(self.repr_ok[precision] and self.max_bound() * 2.0 ** self.m < F32_EXACT)


def _check_repr(rec, a, weight=False, bf16=True):
    """Records whether the GEMM input `a` is exact in bf16 and in the fp16 hi+lo
    split (a weight: in fp16 itself), and its dyadic depth.  Values that are
    multiples of 2^-m with |v| 2^m <= 256 have at most 8 significant bits and
    are exact in both; anything else is tested value by value."""
    a = np.asarray(a, np.float64)
    m = dyadic_bits(a)
    rec.m = max(rec.m, m)
    if weight:
        rec.repr_ok["bf16"] &= bf16_exact(a)
        rec.repr_ok["f16x3"] &= f16_exact(a)
    elif a.size and np.abs(a).max() * 2.0 ** m > 256:
        if bf16:
            rec.repr_ok["bf16"] &= bf16_exact(a)
        rec.repr_ok["f16x3"] &= f16x3_exact(a)
    return m


def forward64(sd, nf, B, nx, edge_index=None, record=True, seam_mutant=False):
    """Plain numpy float64 FluxGNN forward (src/flux_gnn.py:40-67) on B periodic
    chains of nx cells (or, with edge_index [2,E], on that graph: B, nx ignored).
    Input layer, L layers of h = ReLU(W_a h + W_b mean_nb(h) + b), the edge MLP
    on [h_row ; h_col], edges i -> i+1 first and i+1 -> i second.  Returns
    (flux [B, 2nx] (graph: [E]), Record or None).

    seam_mutant (CPU mutant, tests only): from the second update layer on, the
    left neighbour of every cell whose super-window stream index is a multiple
    of 63 is the cell itself (a stale seam slot of the bf16 kernel)."""
    f64 = np.float64
    W = {k: np.asarray(v, f64) for k, v in sd.items()}
    L = n_layers(sd)
    rec = Record() if record else None
    x = np.asarray(nf, f64).reshape(-1, W["input_mlp.0.weight"].shape[1])
    chain = edge_index is None
    if not chain:
        row, col = np.asarray(edge_index[0]), np.asarray(edge_index[1])
        deg = np.maximum(np.bincount(row, minlength=x.shape[0]), 1).astype(f64)[:, None]
    stale = None
    if seam_mutant:
        P = sw_segment(nx, L)
        s = (np.arange(B)[:, None] * P + L + np.arange(nx)[None, :])
        stale = (s % SW_STRIDE == 0)[:, :, None]

    def mean_nb(h, l):
        if chain:
            h3 = h.reshape(B, nx, -1)
            left = np.roll(h3, 1, axis=1)
            if stale is not None and l >= 1:
                left = np.where(stale, h3, left)
            return ((left + np.roll(h3, -1, axis=1)) / 2).reshape(h.shape)
        agg = np.zeros_like(h)
        np.add.at(agg, row, h[col])
        return agg / deg

    def linear(name, xs, Ws, b, relu_layer=True):
        y = sum(a @ w.T for a, w in zip(xs, Ws)) + b
        if rec is not None:
            # max over rows of |x| @ |W|^T + |b|, bounded from above by the column maxima of |x|
            rec.bound[name] = float((sum(np.abs(a).max(0) @ np.abs(w).T for a, w in zip(xs, Ws)) + np.abs(b)).max())
            if relu_layer:
                rec.zero_frac[name] = float(np.mean(y == 0))
        return y

    if rec is not None:
        live = np.abs(W["input_mlp.0.weight"]).sum(0) > 0    # columns with a zero weight never reach a GEMM
        _check_repr(rec, x[:, live])
        for k, v in W.items():
            if k.endswith("weight"):
                _check_repr(rec, v, weight=True)
        wm = dyadic_bits(*W.values())
        assert wm == 0, "integer weights and biases: a map's output is as dyadic as its input"
    h = np.maximum(linear("input", [x], [W["input_mlp.0.weight"]], W["input_mlp.0.bias"]), 0)
    H = h.shape[1]
    for l in range(L):
        Wl = W[f"update_mlps.{l}.0.weight"]
        agg = mean_nb(h, l)
        if rec is not None:
            _check_repr(rec, h)
            _check_repr(rec, h @ Wl[:, H:].T, bf16=False)   # the linearity form's per-cell W_b h (f16x3)
            rec.bound[f"layer{l}.Wb_h"] = float((h.max(0) @ np.abs(Wl[:, H:]).T).max())
            rec.m = max(rec.m, dyadic_bits(agg))
            rec.max_act = max(rec.max_act, float(h.max()))
        h = np.maximum(linear(f"layer{l}", [h, agg], [Wl[:, :H], Wl[:, H:]], W[f"update_mlps.{l}.0.bias"]), 0)
    if rec is not None:
        _check_repr(rec, h)
        rec.max_act = max(rec.max_act, float(h.max()))
    We, be = W["edge_mlp.0.weight"], W["edge_mlp.0.bias"]
    w2, b2 = W["edge_mlp.2.weight"], W["edge_mlp.2.bias"]
    if chain:
        h3 = h.reshape(B, nx, H)
        hr = np.concatenate([h3, np.roll(h3, -1, axis=1)], axis=1).reshape(-1, H)   # row: i, then i+1
        hc = np.concatenate([np.roll(h3, -1, axis=1), h3], axis=1).reshape(-1, H)   # col: i+1, then i
    else:
        hr, hc = h[row], h[col]
    z = np.maximum(linear("edge0", [hr, hc], [We[:, :H], We[:, H:]], be), 0)
    flux = linear("edge2", [z], [w2], b2, relu_layer=False)[:, 0]
    return (flux.reshape(B, 2 * nx) if chain else flux), rec


def forward64_faces(sd, state, nx):
    """The rollout cases' reference: face flux F[i] = 0.5 (fe[i] + fe[nx+i])
    (src/hybrid_solver.py:47-49) of the forward on node features (n, u, E, x)
    with zero_x weights: x enters with weight 0, so it is taken as 0 here.
    Returns (F [B, nx], flux [B, 2nx], Record)."""
    state = np.asarray(state, np.float64)
    B = state.shape[0]
    nf = np.concatenate([state.transpose(0, 2, 1), np.zeros((B, nx, 1))], axis=2).reshape(B * nx, 4)
    assert not np.any(np.asarray(sd["input_mlp.0.weight"])[:, 3]), "rollout cases need zero_x weights"
    fe, rec = forward64(sd, nf, B, nx)
    F = 0.5 * (fe[:, :nx] + fe[:, nx:])
    rec.m = max(rec.m, dyadic_bits(F))
    return F, fe, rec


def halo_mutant_forward64(sd, nf, B, nx):
    """CPU mutant: the bf16 kernel's padded segments (segment cell p of IC b is
    IC cell (p - L) mod nx, P = nx + 2L + 1 cells) with the halo cells (p < L
    and p >= L + nx) read from IC b+1: a `locate` off by one at IC boundaries."""
    L = n_layers(sd)
    P = sw_segment(nx, L)
    x = np.asarray(nf, np.float64).reshape(B, nx, -1)
    p = np.arange(P)
    cell = (p - L) % nx
    seg = x[:, cell]
    halo = (p < L) | (p >= L + nx)
    seg[:, halo] = np.roll(x, -1, axis=0)[:, cell[halo]]
    fe, _ = forward64(sd, seg.reshape(B * P, -1), B, P, record=False)
    return np.concatenate([fe[:, L:L + nx], fe[:, P + L:P + L + nx]], axis=1)


def swap_k_mutant(sd):
    """CPU mutant: two adjacent k-columns of the last update layer's W_b swapped:
    a packing-order fault.  Of the adjacent pairs that differ, the one with the
    most nonzero weights (a pair of empty columns is no fault at all)."""
    L = n_layers(sd)
    key = f"update_mlps.{L - 1}.0.weight"
    W = np.array(sd[key])
    H = W.shape[0]
    nz = (W[:, H:] != 0).sum(0)
    pairs = [(int(nz[k] + nz[k + 1]), -k) for k in range(H - 1) if not np.array_equal(W[:, H + k], W[:, H + k + 1])]
    k = H - max(pairs)[1]
    W[:, [k, k + 1]] = W[:, [k + 1, k]]
    return {**sd, key: W}


def grads64(sd, nf, B, nx, gup, edge_index=None, mask_ge=False):
    """float64 torch autograd of the same forward (written on the edge list, as
    the reference is) with upstream gradient gup [E].  Returns (flux [E], grads:
    every parameter's and "node_features"' gradient as float64 numpy, Record).
    The record adds the backward's absolute-sum bounds per linear map
    (|dy|^T @ |x| and sum |dy| for the weight and bias gradients, |dy| @ |W| for
    the data gradient) and the dyadic depth of every gradient; valid("f32")
    then covers the backward too.  mask_ge (CPU mutant): ReLU' = (z >= 0)."""
    f64 = torch.float64
    p = {k: torch.tensor(np.asarray(v, np.float64), dtype=f64, requires_grad=True) for k, v in sd.items()}
    L = n_layers(sd)
    x = torch.tensor(np.asarray(nf, np.float64), dtype=f64, requires_grad=True)
    ei = torch.from_numpy(chain_edges(nx, B) if edge_index is None else np.asarray(edge_index, np.int64))
    row, col = ei[0], ei[1]
    deg = torch.bincount(row, minlength=x.shape[0]).clamp_min(1).to(f64).unsqueeze(-1)
    maps = []

    def relu(z):
        return torch.where((z >= 0) if mask_ge else (z > 0), z, torch.zeros_like(z))

    def linear(name, a, Wk, bk):
        y = a @ p[Wk].T + p[bk]
        y.retain_grad()
        maps.append((name, a, p[Wk], p[bk], y))
        return y

    h = relu(linear("input", x, "input_mlp.0.weight", "input_mlp.0.bias"))
    for l in range(L):
        agg = torch.zeros_like(h).index_add_(0, row, h[col]) / deg
        h = relu(linear(f"layer{l}", torch.cat([h, agg], -1), f"update_mlps.{l}.0.weight", f"update_mlps.{l}.0.bias"))
    z = relu(linear("edge0", torch.cat([h[row], h[col]], -1), "edge_mlp.0.weight", "edge_mlp.0.bias"))
    flux = linear("edge2", z, "edge_mlp.2.weight", "edge_mlp.2.bias").squeeze(-1)
    (flux * torch.tensor(np.asarray(gup, np.float64))).sum().backward()
    rec = Record()
    grads = {k: v.grad.numpy().copy() for k, v in p.items()}
    grads["node_features"] = x.grad.numpy().copy()
    with torch.no_grad():
        for name, a, Wm, bm, y in maps:
            dy = y.grad.abs()
            rec.bound[name] = float((a.abs() @ Wm.abs().T + bm.abs()).max())
            rec.bound[name + ".dW"] = float((dy.T @ a.abs()).max()) if a.numel() else 0.0
            rec.bound[name + ".db"] = float(dy.sum(0).max())
            rec.bound[name + ".dx"] = float((dy @ Wm.abs()).max())
    rec.m = dyadic_bits(*grads.values(), flux.detach().numpy(), *(a.detach().numpy() for _, a, _, _, _ in maps))
    return flux.detach().numpy().copy(), grads, rec


# --------------------------------------------------------------------- case table
PRECS = ("f32", "f16x3", "bf16")


class Case:
    """One row of the table.  kind: "flux" (chain_flux / FluxGNN.forward),
    "graph" (generic path), "rollout" (engine.run / engine.step face flux),
    "train" (autograd path: flux and gradients)."""

    def __init__(self, name, kind, nx, B, layers, precisions=PRECS, hidden=128, hi=4, dense=False, graph=None,
                 quarter=False, grads=False, seed0=0):
        self.name, self.kind, self.nx, self.B, self.layers = name, kind, nx, B, layers
        self.precisions, self.hidden, self.hi, self.dense = tuple(precisions), hidden, hi, dense
        self.graph, self.quarter = graph, quarter
        self.grads = grads or kind == "train"
        self.zero_x = kind == "rollout"
        self.seed0 = seed0   # where the seed search starts (itself a result of that search, to keep it short)

    def __repr__(self):
        return self.name

    # inputs of one seed ------------------------------------------------------
    def edge_index(self):
        if self.graph == "circ4":
            return circulant4_edges(self.B * self.nx)
        if self.graph == "mixed":
            return mixed_edges()[1]
        return None

    def nodes(self):
        return mixed_edges()[0] if self.graph == "mixed" else self.B * self.nx

    def inputs(self, seed):
        kw = dict(ka=8, kb=8, kin=4, ke=8) if self.dense else {}
        sd = make_sd(self.layers, seed, hidden=self.hidden, zero_x=self.zero_x, **kw)
        nf = features(1, self.nodes(), seed, self.hi) if self.graph == "mixed" else \
            features(self.B, self.nx, seed, self.hi)
        if self.zero_x:
            nf[:, 3] = 0
        return sd, nf

    def state0(self, nf):
        """The rollout cases' integer state [B,3,nx] (the node features' n, u, E)."""
        return np.ascontiguousarray(nf.reshape(self.B, self.nx, 4)[:, :, :3].transpose(0, 2, 1))


class Built:
    """A case with its seed chosen: inputs and float64 references."""


def sub_batch(case):
    """ICs the CPU mutants run on (the first ones: ICs are independent in the
    reference, so a mutant that shows on them shows on the case)."""
    return case.B if case.graph is not None else min(case.B, max(8, 4096 // case.nx))


def sensitivity(case, sd, nf, flux):
    """Faces of IC 0 whose flux (either direction) changes when every feature of
    its middle cell changes, and the size of that cell's receptive field."""
    nx, L = case.nx, case.layers
    c = nx // 2
    x = np.array(nf[:nx])
    x[c] = (x[c] + 1) % max(case.hi, 2)
    if case.zero_x:
        x[c, 3] = 0
    f2, _ = forward64(sd, x, 1, nx, record=False)
    diff = (f2[0, :nx] != flux[0, :nx]) | (f2[0, nx:] != flux[0, nx:])
    return int(diff.sum()), min(nx, 2 * L + 2)


def nonvacuous(case, sd, nf, flux, rec):
    """The conditions of a sharp case (conditions, not measurements): returns
    the list of those that fail."""
    bad = []
    if np.mean(flux != 0) < 0.99:
        bad.append(f"nonzero fluxes {np.mean(flux != 0):.3f} < 0.99")
    want = min(2 * case.nx, 50) if case.graph is None else min(flux.size // 2, 50)
    if len(np.unique(flux)) < want:
        bad.append(f"distinct fluxes {len(np.unique(flux))} < {want}")
    low = {k: v for k, v in rec.zero_frac.items() if v < 0.005}
    if low:
        bad.append(f"pre-activations exactly 0: {low} < 0.5 %")
    if case.layers >= 1:   # a packing-order fault (swap_k_mutant) must show in a flux of the first ICs
        nb = sub_batch(case)
        ei = case.edge_index()
        n = case.nodes() if ei is not None else nb * case.nx
        swapped, _ = forward64(swap_k_mutant(sd), nf[:n], nb, case.nx, edge_index=ei, record=False)
        if np.array_equal(swapped.reshape(-1), flux.reshape(-1)[:swapped.size]):
            bad.append("two swapped k-columns of W_b change no flux")
    if case.graph is None:
        changed, field = sensitivity(case, sd, nf, flux)
        if changed < field - case.layers // 2:
            bad.append(f"one cell changes {changed} of {field} faces")
    return bad


def build(case, seed):
    """Inputs, references and records of `case` at `seed` (no acceptance test)."""
    b = Built()
    b.case, b.seed = case, seed
    b.sd, b.nf = case.inputs(seed)
    b.ei = case.edge_index()
    if case.kind == "rollout":
        b.faces, b.flux, b.rec = forward64_faces(b.sd, case.state0(b.nf), case.nx)
    else:
        b.flux, b.rec = forward64(b.sd, b.nf, case.B, case.nx, edge_index=b.ei)
    b.gup = b.grads = b.grec = None
    if case.grads:
        b.gup = upstream(b.flux.size, seed, case.quarter)
        gflux, b.grads, b.grec = grads64(b.sd, b.nf, case.B, case.nx, b.gup, edge_index=b.ei)
        assert np.array_equal(gflux, b.flux.reshape(-1)), "grads64 and forward64 disagree"
    return b


def accept(b):
    """Why this seed is not taken ([] = taken): validity for every precision the
    case runs in (the backward too for gradient cases), then non-vacuity."""
    bad = [f"not valid for {p}" for p in b.case.precisions if not b.rec.valid(p)]
    if b.grec is not None and not b.grec.valid("f32"):
        bad.append(f"backward bound {b.grec.max_bound():.3g} * 2^{b.grec.m} >= 2^24")
    return bad or nonvacuous(b.case, b.sd, b.nf, b.flux, b.rec)


_BUILT = {}


def find_case(case, build=build, accept=accept):
    """The case at the first seed (of SEEDS) that is valid for all its
    precisions and non-vacuous; cached per case.  CPU only.  build / accept:
    another case family's own (tests/saturating_cases.py; its names are its own)."""
    if case.name not in _BUILT:
        why = []
        for seed in range(case.seed0, SEEDS):
            b = build(case, seed)
            bad = accept(b)
            if not bad:
                _BUILT[case.name] = b
                break
            why.append((seed, bad[0]))
        else:
            raise RuntimeError(f"no valid seed for {case.name}: {why[:4]} ...")
    return _BUILT[case.name]


def _table():
    T = []
    # fused kernels: nx = 16 MT.  B = 5 reaches the cell-split kernels, 2048 the IC-per-wave ones
    for nx in (16, 32, 48, 64):
        for B in (5, 2048):
            for L in (0, 1, 4) + ((8,) if nx >= 48 else ()):
                # 8 layers over 2048 ICs: features in {0, 1} keep every activation a bf16 value
                big8 = L == 8 and B == 2048
                T.append(Case(f"fused_nx{nx}_B{B}_L{L}", "flux", nx, B, L, hi=2 if big8 else 4, seed0=2 if big8 else 0))
    # every other nx: the bf16 super-window kernel, the f32 / f16x3 64-cell windows
    for nx in (1, 2, 3, 7, 15, 17):
        T.append(Case(f"tiny_nx{nx}_B300_L4", "flux", nx, 300, 4))
    for nx in (53, 54, 55):              # bf16 segment P = nx + 2L + 1 = 62, 63, 64 (the wave stride is 63)
        T.append(Case(f"seg_nx{nx}_B7_L4", "flux", nx, 7, 4))
    for nx in (56, 110, 111):            # f32 / f16x3: one window holds win_faces(4) = 55 faces; 2 -> 3 windows at 110 -> 111
        T.append(Case(f"win_nx{nx}_B7_L4", "flux", nx, 7, 4))
    for nx in (486, 487, 488):           # P = sw_faces(4) - 1, sw_faces(4), sw_faces(4) + 1
        T.append(Case(f"swface_nx{nx}_B7_L4", "flux", nx, 7, 4))
    for L in (0, 1, 2, 3, 4, 8):
        T.append(Case(f"win_nx100_B6_L{L}", "flux", 100, 6, L))
    for nx in (1000, 1024):
        T.append(Case(f"long_nx{nx}_B3_L4", "flux", nx, 3, 4))
    T.append(Case("persist_nx100_B1500_L4", "flux", 100, 1500, 4))   # 330 super-windows: a second persistent round
    # dense recipe (8 nonzeros per row), f32 and f16x3
    for nx, B in ((64, 5), (64, 2048), (100, 6)):
        T.append(Case(f"dense_nx{nx}_B{B}_L2", "flux", nx, B, 2, precisions=("f32", "f16x3"), hi=2, dense=True))
    # generic path, f32: untagged chains use win_nx100_B6_L4; graphs at every width
    for H in (32, 64, 128, 256):
        T.append(Case(f"graph_circ4_H{H}", "graph", 37, 1, 2, precisions=("f32",), hidden=H, graph="circ4",
                      grads=H == 128))
        T.append(Case(f"graph_mixed_H{H}", "graph", 34, 1, 2, precisions=("f32",), hidden=H, graph="mixed"))
    # rollout cores (zero_x weights, integer state)
    for L in (1, 4):
        for nx in (16, 32, 48, 64):
            for B in (5, 2048):
                T.append(Case(f"rollout_nx{nx}_B{B}_L{L}", "rollout", nx, B, L))
        for nx in (100, 1024):
            T.append(Case(f"rollout_nx{nx}_B3_L{L}", "rollout", nx, 3, L))
    # chain training path, f32 (shapes of test_chain_training_path_vs_oracle)
    for nx, B, L, H in ((64, 5, 4, 128), (64, 300, 4, 128), (64, 301, 4, 128), (32, 11, 3, 128), (48, 7, 8, 128),
                        (16, 5, 2, 128), (100, 3, 3, 128), (1, 3, 2, 128), (2, 4, 1, 64), (7, 6, 0, 32),
                        (64, 3, 2, 256), (64, 4, 3, 16)):
        big = B >= 300
        T.append(Case(f"train_nx{nx}_B{B}_L{L}_H{H}", "train", nx, B, L, precisions=("f32",), hidden=H,
                      hi=2 if big else 4, quarter=big))
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases(kind):
    return [c for c in CASES if c.kind == kind]


# ------------------------------------------------------------------ mismatch report
def mismatch(got, want, nx=None):
    """None when got == want bitwise as values (float64 compare), else a message
    with the first mismatching (IC, edge), the count and edge mod 63."""
    got = np.asarray(got).astype(np.float64).reshape(np.shape(want))
    want = np.asarray(want, np.float64)
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    first = tuple(int(v) for v in bad[0])
    msg = f"{len(bad)} of {want.size} differ; first at {first}: got {got[first]!r}, want {want[first]!r}"
    if want.ndim == 2 and nx:
        e = bad[:, 1] % nx
        msg += f"; (IC, edge) = {first}; face mod 63 of the first 8: {[int(v) % 63 for v in e[:8]]}"
        msg += f"; ICs hit: {len(np.unique(bad[:, 0]))}; faces hit (first 8): {[int(v) for v in e[:8]]}"
    return msg
