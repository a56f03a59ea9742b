"""The row counts at which the PureGNN, PINN and generic-graph training kernels
change regime, and the cases that put a test on each side of every boundary.
A shared table, not a test: test_row_regimes_cpu.py ties the constants to
csrc/ and checks that the cases reach what their `why` says,
test_gpu_row_regimes.py runs them.  When a threshold moves in the sources,
move it here and add the sizes next to its new place.

The rows are what the training GEMMs reduce over (weight gradients) or tile
(forward, data gradients): N = B nx for PureGNN, B for PINN, N and E for the
generic path.  The regimes, from csrc/:
  tg_block (tgemm.h) ..... output tiles of a launch with T workgroups are paired per
      XCD for the linear index below T - T % REMAP_GROUP; the tail keeps its order
  split-K ................ pure_wg_splits / pinn_wg_splits request a split count,
      tgemm_splits rounds the rows per split up to the stage depth; a split runs
      its stages in pairs plus an odd last one; rows past the split's end are zeroed
  EX kernels ............. whole tiles and whole stages only (ex_ok)
  graph.hip .............. split_rows keeps GENERIC_MIN_ROWS per split up to
      GENERIC_MIN_ROWS * GENERIC_MAX_SPLITS rows, then grows the splits; scan_kernel
      carries across SCAN_CHUNK-node chunks
"""
import math

import numpy as np
import torch

TILE_M = 128               # kBM (tgemm.h)
TILE_N = 128               # kBN
STAGE = 32                 # kKC, in tgemm.h and in graph.hip
PURE_SPLIT_ROWS = 256      # pure_wg_splits: N / 256
PURE_SPLIT_CAP = 64
PINN_SPLIT_ROWS = 128      # pinn_wg_splits: ceil(B / 128)
PINN_SPLIT_CAP = 64
GENERIC_MIN_ROWS = 256     # split_rows
GENERIC_MAX_SPLITS = 128   # kMaxSplits
SCAN_CHUNK = 1024          # scan_kernel
REMAP_GROUP = 16           # tg_block

REL = 2e-5                 # the gradient gate: |got - ref| <= REL max|ref| + 1e-9 per tensor


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------- restatements of csrc/
def tgemm_splits(R, splits):
    """(rows per split, number of splits) tgemm / tgemm_batch make of R rows."""
    rsplit = cdiv(cdiv(R, splits), STAGE) * STAGE
    return rsplit, (cdiv(R, rsplit) if R > 0 else 1)


def pure_wg_splits(N):
    return min(PURE_SPLIT_CAP, max(1, N // PURE_SPLIT_ROWS))


def pinn_wg_splits(B):
    return min(PINN_SPLIT_CAP, max(1, cdiv(B, PINN_SPLIT_ROWS)))


def split_rows(M):
    """graph.hip: rows per split of gemm_wgrad; the split count is ceil(M / rows)."""
    R = max(cdiv(M, GENERIC_MAX_SPLITS), GENERIC_MIN_ROWS)
    return cdiv(R, STAGE) * STAGE


def split_lengths(R, rsplit):
    return [min(rsplit, R - z * rsplit) for z in range(cdiv(R, rsplit))]


def stage_counts(R, rsplit):
    return [cdiv(n, STAGE) for n in split_lengths(R, rsplit)]


def last_stage_rows(R, rsplit):
    """Rows of the last stage of the last split."""
    n = split_lengths(R, rsplit)[-1]
    return n - (cdiv(n, STAGE) - 1) * STAGE


def tg_decode(L, T):
    """tg_block's map of a linear workgroup index."""
    if L < T - T % REMAP_GROUP:
        L = 2 * (8 * (L >> 4) + (L & 7)) + ((L >> 3) & 1)
    return L


def tg_block(bx, by, bz, grid):
    """(bx, by, bz) of the tile a workgroup computes."""
    gx, gy, gz = grid
    L = tg_decode(bx + gx * (by + gy * bz), gx * gy * gz)
    return L % gx, (L // gx) % gy, L // (gx * gy)


def ex_ok(I, J, R):
    """tgemm<..., EXOK> and tgemm_batch take the exact kernel (unsplit views within R)."""
    return R > 0 and I % TILE_M == 0 and J % TILE_N == 0 and R % STAGE == 0


def pure_chain_path(H, nx, N):
    """pure_train_chain: tagged chains on the tgemm GEMMs."""
    return nx > 0 and 128 % nx == 0 and H % 64 == 0 and H <= 1024 and (N + 1) * 2 * H < 2 ** 31


def pinn_gemm_path(D, H, B):
    return D % 32 == 0 and H % 32 == 0 and (B + 1) * max(D, H) < 2 ** 31


def _launch(name, I, J, R, splits=1, batch=1):
    rsplit, S = tgemm_splits(R, splits)
    return dict(name=name, I=I, J=J, R=R, rsplit=rsplit, S=S, batch=batch,
                grid=(cdiv(I, TILE_M), cdiv(J, TILE_N), S * batch))


def pure_forward_launches(H, nx, L, B):
    """The tgemm launches of launch_pure_forward_train on the chain path."""
    N = B * nx
    return [_launch(f"msg{l}", N, 2 * H, H) for l in range(L)] + [_launch("out0", N, H, H)]


def pure_backward_launches(H, nx, L, B):
    """The tgemm / tgemm_batch launches of launch_pure_backward on the chain path;
    `wgrad` marks the split-K ones (their EX form is ex_ok(I, J, R))."""
    N = B * nx
    sp = pure_wg_splits(N)
    out = [dict(_launch("head_wgrad", H, H, N, splits=sp), wgrad=True), _launch("head_dgrad", N, H, H)]
    out += [_launch(f"dgrad{l}", N, H, 2 * H) for l in reversed(range(L))]
    if L > 0:
        out.append(dict(_launch("layers_wgrad", 2 * H, H, N, splits=sp, batch=L), wgrad=True))
    return out


def pinn_forward_launches(D, H, L, B):
    return [_launch(f"fwd{l}", B, H, D if l == 0 else H) for l in range(L - 1)] + [_launch(f"fwd{L - 1}", B, D, H)]


def pinn_backward_launches(D, H, L, B):
    sp = pinn_wg_splits(B)
    out = [_launch(f"dgrad{l}", B, H, D if l == L - 1 else H) for l in range(L - 1, 0, -1)]
    out.append(_launch("dstate", B, D, H))
    out.append(dict(_launch(f"wgrad{L - 1}", D, H, B, splits=sp), wgrad=True))
    out.append(dict(_launch("wgrad0", H, D, B, splits=sp), wgrad=True))
    if L > 2:
        out.append(dict(_launch("hidden_wgrad", H, H, B, splits=sp, batch=L - 2), wgrad=True))
    return out


# ------------------------------------------------------------------------ the cases
# PureGNN chain path: (H, nx, L, B, why)
PURE_CHAIN_WHY = [
    (64, 64, 2, 257, "N = 16448: splits capped at 64, S = 58 below the request, a 32-row last split (stage "
                     "counts 9 and 1); forward grid 129 with a remap tail of 1 and a half-empty last row tile; "
                     "batched weight-gradient grid 116, tail 4"),
    (128, 64, 2, 256, "N = 16384: EX kernels, exactly 64 splits of 256 rows, 8 stages each; grids of 256, 64, 256"),
    (128, 16, 1, 1023, "N = 16368: N / 256 = 63 just under the cap, S = 57; N % 32 = 16, a ragged last stage "
                       "inside a 240-row last split; N % 128 = 112"),
    (64, 64, 1, 30, "forward grid 15: below the first remap group"),
    (64, 64, 1, 32, "forward grid 16: exactly one remap group"),
    (64, 64, 1, 34, "forward grid 17: one remap group and a tail of 1"),
    (128, 64, 1, 34, "forward grid 17 x 2 = 34: gridDim.x odd with two column tiles, tail 2; EX weight gradients"),
    (64, 64, 2, 7, "N = 448: one split"),
    (64, 64, 2, 8, "N = 512: two splits"),
]
PURE_CHAIN = [c[:4] for c in PURE_CHAIN_WHY]
PURE_IN_DIM = 4

# PINN GEMM path: (D, H, L, B, why)
PINN_GEMM_WHY = [
    (192, 256, 4, 2000, "the bench shape: 16 splits of 128 rows, an 80-row last split with a ragged 16-row stage, "
                        "clamped kernels; 32-block forward grids, a 128-block batched weight gradient"),
    (192, 256, 4, 2048, "the same with B % 32 = 0: EX on the hidden layers"),
    (192, 256, 3, 8192, "64 splits, exactly at the cap"),
    (192, 256, 3, 8193, "capped: rsplit 160, S = 52, a 33-row last split whose last stage holds one row"),
]
PINN_GEMM = [c[:4] for c in PINN_GEMM_WHY]

# the generic path (graph.hip): PureGNN on chains whose nx does not divide 128, PINN with D % 32 != 0
PURE_GENERIC_WHY = [
    (64, 48, 2, 682, "N = 32736: 128 splits of 256 rows, the last size before split_rows grows them"),
    (64, 48, 2, 700, "N = 33600: capped at 128 splits, R = 288, S = 117"),
]
PURE_GENERIC = [c[:4] for c in PURE_GENERIC_WHY]
PINN_GENERIC_WHY = [(15, 16, 2, 40000, "B = 40000: capped, R = 320, S = 125")]
PINN_GENERIC = [c[:4] for c in PINN_GENERIC_WHY]
# FluxGNN(in, H, L) on a general graph: nodes, isolated from, edges
FLUX_GRAPH = dict(dims=(4, 32, 2), N=2500, first_isolated=2400, E=40000,
                  why="three scan chunks; the edge-row weight gradients capped (R = 320, S = 125); duplicate "
                      "edges, self-loops, isolated nodes")

# the sliding-block cases of test_gpu_row_regimes.py (c)
PURE_SLIDE = [(64, 64, 2, 257), (128, 64, 2, 256), (128, 16, 1, 1023)]
PINN_SLIDE = [(192, 256, 4, 2000), (192, 256, 3, 8193)]
# two backward passes, bit for bit
PURE_TWICE = (64, 64, 2, 257)
PINN_TWICE = (192, 256, 3, 8193)
# the cases that also run an untagged clone (the generic kernels on CSR buckets) in (a)
PURE_UNTAGGED = [(64, 64, 2, 257), (128, 16, 1, 1023), (64, 64, 2, 8)] + PURE_GENERIC


# ----------------------------------------------------------------------- the inputs
def _linear(g, out, inp, scale=1.0):
    a = scale / math.sqrt(inp)
    return g.uniform(-a, a, (out, inp)).astype(np.float32), g.uniform(-a, a, out).astype(np.float32)


def pure_sd(H, L, seed, in_dim=PURE_IN_DIM):
    """A PureGNN(in_dim, H, L) state dict, nn.Linear's uniform init from a numpy seed."""
    g = np.random.default_rng(seed)
    sd = {}
    sd["input_mlp.0.weight"], sd["input_mlp.0.bias"] = _linear(g, H, in_dim)
    for l in range(L):
        sd[f"update_mlps.{l}.0.weight"], sd[f"update_mlps.{l}.0.bias"] = _linear(g, H, 2 * H)
    sd["output_mlp.0.weight"], sd["output_mlp.0.bias"] = _linear(g, H, H)
    sd["output_mlp.2.weight"], sd["output_mlp.2.bias"] = _linear(g, 3, H)
    return sd


def pinn_sd(D, H, L, seed):
    """A PINN(D, H, L) state dict (net.0, net.2, ...), nn.Linear's uniform init."""
    g = np.random.default_rng(seed)
    sd = {}
    for l in range(L):
        sd[f"net.{2 * l}.weight"], sd[f"net.{2 * l}.bias"] = _linear(g, D if l == L - 1 else H, D if l == 0 else H)
    return sd


def pure_seed(H, nx, L, B):
    return 100000 * L + 1000 * H + 10 * nx + B


def pure_inputs(H, nx, L, B):
    """(sd, nf [N, 4] float32, up [N, 3] float32) of a PureGNN case."""
    g = np.random.default_rng(pure_seed(H, nx, L, B) + 1)
    N = B * nx
    return (pure_sd(H, L, pure_seed(H, nx, L, B)), g.normal(0, 1, (N, PURE_IN_DIM)).astype(np.float32),
            g.normal(0, 1, (N, 3)).astype(np.float32))


def pinn_seed(D, H, L, B):
    return 100000 * L + 1000 * H + 10 * D + B


def pinn_inputs(D, H, L, B):
    """(sd, state [B, 3, nx] float32, up [B, 3, nx] float32) of a PINN case."""
    g = np.random.default_rng(pinn_seed(D, H, L, B) + 1)
    nx = D // 3
    st = np.stack([1 + 0.1 * g.normal(0, 1, (B, nx)), 0.1 * g.normal(0, 1, (B, nx)), 0.1 * g.normal(0, 1, (B, nx))], 1)
    return pinn_sd(D, H, L, pinn_seed(D, H, L, B)), st.astype(np.float32), g.normal(0, 1, (B, 3, nx)).astype(np.float32)


def flux_graph_inputs():
    """(sd, nf [N, 4], edge_index [2, E] int64, up [E]) of the FluxGNN general-graph case.
    Every edge joins two of the first `first_isolated` nodes; the last 2000 edges repeat
    the first 2000, and 500 more are self-loops.  The weights are the kink-free recipe
    of test_chain_training_path_vs_oracle (biases of 4 against products below 3): at
    E H = 1.28 M pre-activations random weights put a few ReLUs within rounding of 0."""
    c = FLUX_GRAPH
    F, H, L = c["dims"]
    g = np.random.default_rng(c["N"] + c["E"])
    u = lambda a, shape: g.uniform(-a, a, shape)  # noqa: E731
    sd = {"input_mlp.0.weight": u(0.1, (H, F)), "input_mlp.0.bias": np.full(H, 4.0)}
    for l in range(L):
        sd[f"update_mlps.{l}.0.weight"] = u(0.002, (H, 2 * H))
        sd[f"update_mlps.{l}.0.bias"] = np.full(H, 4.0)
    sd["edge_mlp.0.weight"] = u(0.002, (H, 2 * H))
    sd["edge_mlp.0.bias"] = np.full(H, 4.0)
    sd["edge_mlp.2.weight"] = g.normal(0, 1 / np.sqrt(H), (1, H))
    sd["edge_mlp.2.bias"] = g.normal(0, 0.1, 1)
    sd = {k: np.asarray(v, np.float32) for k, v in sd.items()}
    nf = g.normal(0, 1, (c["N"], F)).astype(np.float32)
    ei = g.integers(0, c["first_isolated"], (2, c["E"]))
    ei[:, -2000:] = ei[:, :2000]
    ei[1, 3000:3500] = ei[0, 3000:3500]
    return sd, nf, ei.astype(np.int64), g.normal(0, 1, c["E"]).astype(np.float32)


def periodic(base, rows):
    """`base` repeated along axis 0 and cut to `rows` rows."""
    return np.concatenate([base] * cdiv(rows, len(base)))[:rows]


# -------------------------------------------------- float64 references with operands
def _p64(sd):
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float64).requires_grad_(True) for k, v in sd.items()}


def pure_chain_operands64(sd, nf, up, nx):
    """PureGNN on B chains of nx cells in float64, written per cell as EpiMsgTape
    forms it (P of the two neighbours, Q of the cell), with the operands of every
    weight-gradient GEMM kept: returns (delta, {param: grad}, nf grad, ops) where
    ops[param] = (A [N, I], X [N, J]) with grad(param) = A^T X (for a message layer
    A = [gP | gQ] and the gradient is [gP^T h | gQ^T h]) and the bias gradient the
    column sums of A (of its gQ half)."""
    p = _p64(sd)
    x = torch.as_tensor(nf, dtype=torch.float64).requires_grad_(True)
    N, H = x.shape[0], p["input_mlp.0.bias"].shape[0]
    B = N // nx
    keep = {}

    def pre(name, v):
        v.retain_grad()
        keep[name] = v
        return v

    h = torch.tanh(pre("in", x @ p["input_mlp.0.weight"].T + p["input_mlp.0.bias"]))
    hs = [h]
    l = 0
    while f"update_mlps.{l}.0.weight" in p:
        W, b = p[f"update_mlps.{l}.0.weight"], p[f"update_mlps.{l}.0.bias"]
        P, Q = pre(f"P{l}", h @ W[:, :H].T), pre(f"Q{l}", h @ W[:, H:].T)
        Pc = P.reshape(B, nx, H)
        prev, nxt = torch.roll(Pc, 1, 1).reshape(N, H), torch.roll(Pc, -1, 1).reshape(N, H)
        h = h + torch.tanh(prev + Q + b) + torch.tanh(nxt + Q + b)
        hs.append(h)
        l += 1
    z = torch.tanh(pre("o0", h @ p["output_mlp.0.weight"].T + p["output_mlp.0.bias"]))
    d = pre("o2", z @ p["output_mlp.2.weight"].T + p["output_mlp.2.bias"])
    (d * torch.as_tensor(up, dtype=torch.float64)).sum().backward()
    ops = {"output_mlp.0.weight": (keep["o0"].grad.numpy(), hs[-1].detach().numpy())}
    for k in range(l):
        ops[f"update_mlps.{k}.0.weight"] = (np.concatenate([keep[f"P{k}"].grad.numpy(), keep[f"Q{k}"].grad.numpy()], 1),
                                            hs[k].detach().numpy())
    return d.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()}, x.grad.numpy(), ops


def pinn_operands64(sd, st, up):
    """PINN in float64 with the operands (G_l, X_l) of every layer's weight gradient."""
    p = _p64(sd)
    s = torch.as_tensor(st, dtype=torch.float64).requires_grad_(True)
    L = len(sd) // 2
    z = s.reshape(s.shape[0], -1)
    xs, pres = [], []
    for l in range(L):
        xs.append(z)
        z = z @ p[f"net.{2 * l}.weight"].T + p[f"net.{2 * l}.bias"]
        z.retain_grad()
        pres.append(z)
        if l < L - 1:
            z = torch.tanh(z)
    out = s + z.reshape(s.shape)
    (out * torch.as_tensor(up, dtype=torch.float64)).sum().backward()
    ops = {f"net.{2 * l}.weight": (pres[l].grad.numpy(), xs[l].detach().numpy()) for l in range(L)}
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()}, s.grad.numpy(), ops


def oracle_run(forward, sd, x, up, dtype, *extra):
    """Autograd of an oracle forward(params, x, *extra) in `dtype` on the CPU:
    (out, {param: grad}, x grad) as float64 numpy arrays."""
    p = {k: torch.as_tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for k, v in sd.items()}
    xx = torch.as_tensor(x, dtype=dtype).requires_grad_(True)
    out = forward(p, xx, *extra)
    (out * torch.as_tensor(up, dtype=dtype)).sum().backward()
    f = lambda t: t.detach().double().numpy()  # noqa: E731
    return f(out), {k: f(v.grad) for k, v in p.items()}, f(xx.grad)


# --------------------------------------- the split-K weight gradient and its mutants
def splitk(A, X, rsplit, mutant=None):
    """gW = A^T X over the rows as tgemm reduces them, in float64: rows cut into splits
    of rsplit and stages of STAGE, each split's stages added in order, the partials
    added in split order.  Mutants, the faults the GPU gates must catch:
      "split" ..... the partial of the last split (the shortest) left out
      "ragged" .... the rows of the last stage past its last whole STAGE left out
                    (None when R % STAGE == 0: there are none)
      "tile" ...... the rows of the second 128-row tile read in place of the first's
      "out" ....... the last 128 x 128 tile of the output left unwritten (zero)"""
    R = A.shape[0]
    if mutant == "ragged":
        if R % STAGE == 0:
            return None
        A = A.copy()
        A[R - R % STAGE:] = 0.0
    if mutant == "tile":
        A, X = A.copy(), X.copy()
        A[:TILE_M], X[:TILE_M] = A[TILE_M:2 * TILE_M], X[TILE_M:2 * TILE_M]
    S = cdiv(R, rsplit)
    out = np.zeros((A.shape[1], X.shape[1]))
    for z in range(S - 1 if mutant == "split" else S):
        part = np.zeros_like(out)
        for r0 in range(z * rsplit, min(R, (z + 1) * rsplit), STAGE):
            r1 = min(r0 + STAGE, R, (z + 1) * rsplit)
            part += A[r0:r1].T @ X[r0:r1]
        out += part
    if mutant == "out":
        out[(out.shape[0] - 1) // TILE_M * TILE_M:, (out.shape[1] - 1) // TILE_N * TILE_N:] = 0.0
    return out


MUTANTS = ("split", "ragged", "tile", "out")


def from_pq(gw, H):
    """[gP | gQ]^T h, [2H][H], as nn.Linear's [H][2H] weight gradient (pure_part_reduce_kernel, split = 1)."""
    return np.concatenate([gw[:H], gw[H:]], 1)


# ----------------------------------------------------------- sliding-block positions
def slide_blocks(R, rsplit, unit, wgrad_grids):
    """[(start, rows, why)] for test (c): blocks of whole units (a chain's nx rows; 1 for
    PINN), at most 256 rows, starting at a multiple of STAGE and inside one split.
    Where whole units cannot cover the named stage of the named split (a chain that
    straddles two splits), the next split where they can is taken."""
    S = cdiv(R, rsplit)
    step = unit * STAGE // math.gcd(unit, STAGE)

    def span(z):
        return z * rsplit, min(R, (z + 1) * rsplit)

    def first(z):
        for k in range(z, S):
            lo, hi = span(k)
            n = cdiv(STAGE, unit) * unit
            if lo % step == 0 and lo + n <= hi:
                return lo, n, k
        return None

    def last(z):
        for k in range(z, S):
            lo, hi = span(k)
            ls = lo + (cdiv(hi - lo, STAGE) - 1) * STAGE  # the last stage's first row
            start = ls // step * step
            if start >= lo and (hi % unit == 0) and hi - start <= 256:
                return start, hi - start, k
        return None

    out = []
    for tag, hit in (("first stage of split", first(0)), ("last stage of split", last(0)),
                     ("first stage of split", first(1)), ("last stage of split", last(1))):
        if hit:
            out.append((hit[0], hit[1], f"{tag} {hit[2]}"))
    for g in wgrad_grids:  # the first split whose workgroups lie past the remap's last full group
        gx, gy, gz = g["grid"]
        T = gx * gy * gz
        if T % REMAP_GROUP:
            z = ((T - T % REMAP_GROUP) // (gx * gy)) % g["S"]
            hit = first(z + (1 if (T - T % REMAP_GROUP) % (gx * gy) else 0))
            if hit:
                out.append((hit[0], hit[1], f"{g['name']}: split {hit[2]}, past the last full remap group"))
    lo, hi = span(S - 1)
    if hi - lo <= 256 and lo % step == 0 and (hi - lo) % unit == 0:
        out.append((lo, hi - lo, f"the whole last split ({hi - lo} rows, a last stage of {last_stage_rows(R, rsplit)})"))
    else:
        hit = last(S - 1)
        if hit:
            out.append((hit[0], hit[1], f"last stage of the last split ({hi - lo} rows)"))
    seen, uniq = set(), []
    for b in out:
        if b[:2] not in seen:
            seen.add(b[:2])
            uniq.append(b)
    return uniq


def pure_slide_blocks(H, nx, L, B):
    la = [g for g in pure_backward_launches(H, nx, L, B) if g.get("wgrad")]
    return slide_blocks(B * nx, la[0]["rsplit"], nx, la)


def pinn_slide_blocks(D, H, L, B):
    la = [g for g in pinn_backward_launches(D, H, L, B) if g.get("wgrad")]
    return slide_blocks(B, la[0]["rsplit"], 1, la)
