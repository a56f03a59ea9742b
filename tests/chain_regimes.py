"""The batch and row counts at which the FluxGNN chain training path
(csrc/train_chain.hip, chain_train_fwd_kernel / chain_train_bwd_kernel) changes
regime, and the cases that reach each regime.  A shared table, not a test:
test_chain_regimes_cpu.py ties the constants to csrc/, checks that every case
reaches what its `why` says and that the gates reject the mutants below;
test_gpu_chain_regimes.py runs the cases.  When a threshold moves in the
sources, move it here and move the sizes next to its new place.

B chains of nx cells, N = B nx rows.  The regimes, from csrc/:
  fused passes ........... FluxGNN(4, 128, L <= 8) on nx in {16, 32, 48, 64}: one chain per
      wave, NW per workgroup, min(ceil(B / NW), CUs * WG_PER_CU) persistent workgroups;
      a workgroup takes group grp + gridDim.x next (feature prefetch, tape rows and ReLU'
      mask words addressed by chain); the last group may be ragged
  edge readout backward .. EDGE_BLOCKS x 4 persistent waves; a wave unit is EB_CELLS
      cells of one chain at H = 128 (periodic by one wrap, or modulo for nx < EB_CELLS)
      and one cell otherwise; dw2 / db2 accumulate per wave over its trips
  stencil weight grads ... wgs (fused, L >= 1, nx % 32 == 0): WGS_SPLITS splits of whole
      WS_KC-cell stages, double-buffered in pairs plus an odd last stage, halo rows
      wrapped inside the chain; else tgemm_batch over the stencil view (BATCH_SPLITS)
  GEMM path .............. any other nx or width: tgemm row tiles (tg_block's remap from
      REMAP_GROUP tiles on), split-K over WGRAD_SPLITS
  input layer ............ INPUT_SPLITS blocks of ceil(N / INPUT_SPLITS) rows
  reductions ............. PR_SLICES slices cut S splits at S q / PR_SLICES (empty for S < slices)

The cases were sized for CUS = 256 compute units; fewer only add passes.
"""
import numpy as np

import exact_cases as X
from row_regimes import REL, REMAP_GROUP, STAGE, TILE_M, cdiv, split_lengths, stage_counts, tgemm_splits  # noqa: F401

NW = 4                 # kNW (CoreF32: kWaves), chains per workgroup
WG_PER_CU = 1          # kWGPerCU (CoreF32)
EDGE_BLOCKS = 1024     # kEdgeBlocks
EDGE_WAVES = 4         # 256 threads per edge block
EB_CELLS = 8           # kEbCells
WGS_SPLITS = 128       # kWgsSplits
WS_KC = 32             # kWsKC
WGRAD_SPLITS = 256     # kWgradSplits
BATCH_SPLITS = 64      # kWgradBatchSplits
INPUT_SPLITS = 512     # kInputSplits
PR_SLICES = 16         # kPrSlices
FUSED_NX = (16, 32, 48, 64)
FUSED_IN, FUSED_H, MAX_LAYERS = 4, 128, 8   # kIn, kH, kMaxChainLayers
CUS = 256              # the compute units the cases were sized for (MI355X)


# ----------------------------------------------------------- restatements of csrc/
def chain_train_ok(H, in_dim, nx, N):
    return (nx > 0 and STAGE <= H <= 256 and H & (H - 1) == 0 and 1 <= in_dim <= 8 and N > 0
            and N * 2 * H + 2 * H < 2 ** 31)


def fused_chain(in_dim, H, L, nx):
    """chain_train_fused_ok (N = B nx is a whole number of chains by construction)."""
    return in_dim == FUSED_IN and H == FUSED_H and 0 <= L <= MAX_LAYERS and nx in FUSED_NX


def wgs(in_dim, H, L, nx, N):
    """launch_chain_backward's `wgs`: the layers' weight gradients on wgrad_stencil_kernel."""
    return fused_chain(in_dim, H, L, nx) and L >= 1 and nx % WS_KC == 0 and N % WS_KC == 0 and N * FUSED_H < 2 ** 31


def train_blocks(B, cus=CUS):
    return min(cdiv(B, NW), cus * WG_PER_CU)


def fused_passes(B, cus=CUS):
    """Groups the busiest workgroup of the fused kernels takes."""
    return cdiv(cdiv(B, NW), train_blocks(B, cus))


def last_pass_chains(B, cus=CUS):
    """First chain of the last fused pass (the groups a workgroup takes last)."""
    return (fused_passes(B, cus) - 1) * train_blocks(B, cus) * NW


def edge_trips(H, nx, B):
    """Units the busiest wave of the edge backward kernel takes."""
    units = B * cdiv(nx, EB_CELLS) if H == 128 else B * nx
    return cdiv(units, EDGE_BLOCKS * EDGE_WAVES)


def wgs_rsplit(N):
    return cdiv(cdiv(N, WGS_SPLITS), WS_KC) * WS_KC


def wgs_splits(N):
    return cdiv(N, wgs_rsplit(N))


def input_rows(N):
    """(rows per block, blocks) of the input layer's weight gradient."""
    rows = cdiv(N, INPUT_SPLITS)
    return rows, cdiv(N, rows)


def slice_cuts(S):
    """[s0, s1) of every slice of part_reduce4 / final_reduce."""
    return [(S * q // PR_SLICES, S * (q + 1) // PR_SLICES) for q in range(PR_SLICES)]


def layer_splits(in_dim, H, L, nx, N):
    """(kernel, rows per split, splits) of the update layers' weight gradients."""
    if L < 1:
        return None
    if wgs(in_dim, H, L, nx, N):
        return ("stencil", wgs_rsplit(N), wgs_splits(N))
    if fused_chain(in_dim, H, L, nx):
        return ("batch",) + tgemm_splits(N, BATCH_SPLITS)
    return ("gemm",) + tgemm_splits(N, WGRAD_SPLITS)


def regime(nx, B, L, H, in_dim=4, cus=CUS):
    """Everything the tests assert about a case, from the restatements."""
    N = B * nx
    fused = fused_chain(in_dim, H, L, nx)
    r = dict(N=N, ok=chain_train_ok(H, in_dim, nx, N), fused=fused, layers=layer_splits(in_dim, H, L, nx, N),
             edge=tgemm_splits(N, WGRAD_SPLITS), edge_kernel="h128" if H == 128 else "any",
             edge_trips=edge_trips(H, nx, B), input=input_rows(N), row_tiles=cdiv(N, TILE_M))
    if fused:
        r.update(passes=fused_passes(B, cus), last_group=B - NW * (cdiv(B, NW) - 1),
                 last_pass_from=last_pass_chains(B, cus))
    return r


# ------------------------------------------------------------------------ the cases
# (nx, B, L, H, why)
CASES_WHY = [
    (64, 1027, 2, 128, "257 groups: a second fused pass whose only group holds 3 chains; edge h128 3 trips; "
                       "stencil: 121 splits of 17 stages, a 14-stage last split"),
    (64, 1027, 0, 128, "the same passes without the batched weight gradients: separate reductions and "
                       "input_wgrad_h128f4_kernel"),
    (32, 2051, 2, 128, "3 fused passes, ragged group of 3 in the third; both halo rows wrap in every stage; "
                       "121 splits of 17 stages, an 11-stage last split"),
    (32, 131, 2, 128, "N = 4192: just past one stage per split: 66 splits of 2 stages, a 1-stage last split"),
    (32, 12, 1, 128, "N = 384: 12 one-stage splits, fewer than the 16 slices of the reductions: empty slices"),
    (16, 4100, 1, 128, "tgemm_batch: 63 splits of 33 stages (a 4-stage last one); 5 fused passes; edge h128 3 trips"),
    (48, 1030, 2, 128, "tgemm_batch: 62 splits of 25 stages whose 32-row stages cut the 48-cell chains; a second "
                       "fused pass with a ragged group of 2"),
    (100, 700, 2, 128, "GEMM path at width 128: 547 row tiles (remapped), N = 70000 > 8192: 244 splits of 9 stages, "
                       "a ragged last stage of 16 rows; edge h128 with a 4-cell last segment, 3 trips"),
    (7, 9000, 1, 128, "nx < kEbCells: the modulo wrap of the edge h128 kernel over 3 trips"),
    (64, 1100, 2, 64, "edge_backward_kernel 18 trips; the GEMM path at width 64"),
    (64, 1100, 1, 32, "edge_backward_kernel 18 trips; the GEMM path at width 32"),
    (64, 600, 2, 256, "edge_backward_kernel 10 trips, two channel rounds per lane; the GEMM path at width 256"),
    (64, 2000, 4, 128, "the training benchmark's batch: 2 fused passes, 125 splits of 32 stages"),
]
SHAPES = [c[:4] for c in CASES_WHY]
# GEMM-path cases with in_dim != 4 (HF_INPUT_DISPATCH): (nx, B, L, H, in_dim, why)
IN_DIM_WHY = [
    (64, 9, 1, 128, 3, "in_dim 3: input_forward_kernel<3>, input_wgrad_kernel<3>, the scalar part_reduce_kernel"),
    (64, 9, 1, 128, 8, "in_dim 8: the widest instantiation, float4 reductions"),
]
# two backward passes, bit for bit
TWICE = [(64, 1027, 2, 128), (48, 1030, 2, 128)]
# chain invariance with the golden weights (FluxGNN(4, 128, 4)): (nx, B)
INVARIANCE = [(nx, B) for nx in (16, 32, 48, 64) for B in (1027, 2051)] + [(100, 700)]
INVARIANCE_BASE = 8

# seed0 per case: the first seed of exact_cases.find_case that also meets extra_conditions (CPU search)
SEED0 = {"regime_nx64_B1027_L2_H128": 1, "regime_nx64_B1027_L0_H128": 4, "regime_nx32_B2051_L2_H128": 1,
         "regime_nx32_B131_L2_H128": 1, "regime_nx48_B1030_L2_H128": 1, "regime_nx100_B700_L2_H128": 1,
         "regime_nx64_B1100_L2_H64": 1, "regime_nx64_B1100_L1_H32": 2, "regime_nx64_B600_L2_H256": 4,
         "regime_nx64_B2000_L4_H128": 2, "regime_nx64_B9_L1_H128_F3": 3}   # every other case: seed 0


class RegimeCase(X.Case):
    """exact_cases.Case (kind "train") with the input width as a parameter."""

    def __init__(self, nx, B, L, H, in_dim=4):
        name = f"regime_nx{nx}_B{B}_L{L}_H{H}" + (f"_F{in_dim}" if in_dim != 4 else "")
        super().__init__(name, "train", nx, B, L, precisions=("f32",), hidden=H, hi=2, quarter=True,
                         seed0=SEED0.get(name, 0))
        self.in_dim = in_dim

    def inputs(self, seed):
        sd = X.make_sd(self.layers, seed, hidden=self.hidden, in_dim=self.in_dim, kin=min(2, self.in_dim))
        return sd, X.features(self.B, self.nx, seed, self.hi, in_dim=self.in_dim)


CASES = [RegimeCase(*s) for s in SHAPES] + [RegimeCase(*c[:5]) for c in IN_DIM_WHY]
BY_SHAPE = {(c.nx, c.B, c.layers, c.hidden, c.in_dim): c for c in CASES}
assert len(BY_SHAPE) == len(CASES)


def case_of(nx, B, L, H, in_dim=4):
    return BY_SHAPE[(nx, B, L, H, in_dim)]


# ------------------------------------------------- the float64 reference, layer by layer
def _roll(a, B, nx, k):
    return np.roll(a.reshape(B, nx, -1), k, axis=1).reshape(a.shape)


def agg(a, B, nx):
    """The chain's mean aggregation (a[i-1] + a[i+1]) / 2; self-adjoint."""
    return (_roll(a, B, nx, 1) + _roll(a, B, nx, -1)) / 2


def tape64(sd, nf, B, nx):
    """exact_cases.forward64 on chains with what the backward needs kept: x, hs[0..L]
    (the ReLU' mask of layer l is hs[l] > 0), the readout's pre-activations zf (edge
    i -> i+1) and zb (i+1 -> i), flux [B, 2nx]."""
    W = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    L = X.n_layers(sd)
    x = np.asarray(nf, np.float64)
    hs = [np.maximum(x @ W["input_mlp.0.weight"].T + W["input_mlp.0.bias"], 0)]
    H = hs[0].shape[1]
    for l in range(L):
        Wl = W[f"update_mlps.{l}.0.weight"]
        hs.append(np.maximum(hs[l] @ Wl[:, :H].T + agg(hs[l], B, nx) @ Wl[:, H:].T + W[f"update_mlps.{l}.0.bias"], 0))
    We, be = W["edge_mlp.0.weight"], W["edge_mlp.0.bias"]
    P, Q = hs[L] @ We[:, :H].T + be, hs[L] @ We[:, H:].T
    zf, zb = P + _roll(Q, B, nx, -1), _roll(P, B, nx, -1) + Q
    w2, b2 = W["edge_mlp.2.weight"][0], W["edge_mlp.2.bias"][0]
    flux = np.concatenate([(np.maximum(zf, 0) @ w2 + b2).reshape(B, nx), (np.maximum(zb, 0) @ w2 + b2).reshape(B, nx)], 1)
    return dict(x=x, hs=hs, zf=zf, zb=zb, flux=flux, B=B, nx=nx)


def backward64(sd, T, gup, masks=None, keep_pre=False):
    """The backward as launch_chain_backward orders it, in float64: dPQ from the flux
    gradient, g[L] = mask[L] * [W_a ; W_b]^T dPQ, g[l] = mask[l] * (W_a^T g[l+1] + W_b^T
    agg g[l+1]).  masks: the ReLU' masks [L + 1] of [N, H] bool (default: T's own).
    Returns (grads as exact_cases.grads64 names them, G = [g[0..L]], dPQ, pre) with pre
    the unmasked dh[0..L] when keep_pre."""
    W = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    B, nx, hs, x = T["B"], T["nx"], T["hs"], T["x"]
    L, H = len(hs) - 1, hs[0].shape[1]
    masks = [h > 0 for h in hs] if masks is None else masks
    g2 = np.asarray(gup, np.float64).reshape(B, 2 * nx)
    gf, gb = g2[:, :nx].reshape(-1, 1), g2[:, nx:].reshape(-1, 1)
    w2 = W["edge_mlp.2.weight"][0]
    grads = {"edge_mlp.2.weight": (gf * np.maximum(T["zf"], 0) + gb * np.maximum(T["zb"], 0)).sum(0)[None],
             "edge_mlp.2.bias": np.array([g2.sum()])}
    dzf, dzb = gf * w2 * (T["zf"] > 0), gb * w2 * (T["zb"] > 0)
    dP, dQ = dzf + _roll(dzb, B, nx, 1), dzb + _roll(dzf, B, nx, 1)
    del dzf, dzb
    We = W["edge_mlp.0.weight"]
    grads["edge_mlp.0.weight"] = np.concatenate([dP.T @ hs[L], dQ.T @ hs[L]], 1)
    grads["edge_mlp.0.bias"] = dP.sum(0)
    dh = dP @ We[:, :H] + dQ @ We[:, H:]
    G, pre = [None] * (L + 1), [None] * (L + 1)
    for l in range(L, -1, -1):
        if l < L:
            Wl = W[f"update_mlps.{l}.0.weight"]
            grads[f"update_mlps.{l}.0.weight"] = np.concatenate([G[l + 1].T @ hs[l], G[l + 1].T @ agg(hs[l], B, nx)], 1)
            grads[f"update_mlps.{l}.0.bias"] = G[l + 1].sum(0)
            dh = G[l + 1] @ Wl[:, :H] + agg(G[l + 1], B, nx) @ Wl[:, H:]
        if keep_pre:
            pre[l] = dh
        G[l] = np.where(masks[l], dh, 0.0)
    grads["input_mlp.0.weight"] = G[0].T @ x
    grads["input_mlp.0.bias"] = G[0].sum(0)
    grads["node_features"] = G[0] @ W["input_mlp.0.weight"]
    return grads, G, np.concatenate([dP, dQ], 1), pre


def chains(T, gup, lo, hi):
    """The tape and upstream gradient of chains [lo, hi) as their own batch."""
    nx = T["nx"]
    r = slice(lo * nx, hi * nx)
    sub = dict(x=T["x"][r], hs=[h[r] for h in T["hs"]], zf=T["zf"][r], zb=T["zb"][r], flux=T["flux"][lo:hi],
               B=hi - lo, nx=nx)
    return sub, np.asarray(gup).reshape(T["B"], 2 * nx)[lo:hi].reshape(-1)


# ------------------------------------------------------------- conditions on a case
MASK_FRAC = 0.05    # every layer's ReLU' mask holds both values on at least this fraction
GRAD_FRAC = 0.25    # every gradient tensor is non-zero on at least this fraction


def extra_conditions(case, b, T=None, cus=CUS):
    """Beyond exact_cases.accept, from the reference alone: the list of conditions that fail."""
    T = tape64(b.sd, b.nf, case.B, case.nx) if T is None else T
    bad = []
    fused = fused_chain(case.in_dim, case.hidden, case.layers, case.nx)
    lo = last_pass_chains(case.B, cus) * case.nx if fused else 0
    named = [(f"h{l}", h > 0) for l, h in enumerate(T["hs"])] + [("zf", T["zf"] > 0), ("zb", T["zb"] > 0)]
    for name, m in named:
        for where, part in (("", m), (" (last fused pass)", m[lo:])):
            f = float(part.mean())
            if min(f, 1 - f) < MASK_FRAC:
                bad.append(f"mask {name}{where}: {f:.3f} set")
    for k, g in b.grads.items():
        f = float(np.mean(g != 0))
        if f < GRAD_FRAC:
            bad.append(f"gradient {k}: {f:.3f} non-zero")
    return bad


def accept(b):
    """exact_cases.accept, then extra_conditions: the seed search of this table."""
    return X.accept(b) or extra_conditions(b.case, b)


# ------------------------------------------------------------------------ the mutants
def stencil_rows(h, B, nx, rows, halo_prev_chain=False):
    """[h ; agg h] of the given rows.  halo_prev_chain (mutant): the row before a chain's
    first cell is row r - 1 of the batch (the chain before), not the chain's own last."""
    N = B * nx
    i = rows % nx
    prev = np.where(i == 0, rows + nx - 1, rows - 1)
    if halo_prev_chain:
        prev = (rows - 1) % N
    nxt = np.where(i == nx - 1, rows - (nx - 1), rows + 1)
    return np.concatenate([h[rows], (h[prev] + h[nxt]) / 2], 1)


def last_stage_rows(N, rsplit, z):
    """The rows of the last stage of split z."""
    lo, hi = z * rsplit, min(N, (z + 1) * rsplit)
    return np.arange(lo + (cdiv(hi - lo, STAGE) - 1) * STAGE, hi)


def mask_word(nx, cell, g):
    """(row within the chain, channels) of one ReLU' mask word of the fused kernels:
    lane group g holds channels 4 g + 16 nt + r of its cell, bit 4 nt + r."""
    return cell, np.array([4 * g + 16 * nt + r for nt in range(8) for r in range(4)])


def mutants(case, b, T, G, dPQ, cus=CUS):
    """{mutant: {tensor: mutated - reference}} on the inputs of case b, in the float64
    reference.  A mutant that does not apply to the case's regime is absent.
      pass2 ..... the chains of every fused pass after the first contribute no g[l] rows
                  to the weight and bias gradients below the readout
      ragged .... the same for the chains of the ragged last group
      halo ...... the stencil's row before a chain's first cell read from the chain before
      stage ..... the last stage of the first and of the last split dropped, per weight GEMM
                  with its own split geometry (reported per split: stage0, stageZ)
      maskword .. one ReLU' mask word of layer 0 of a chain of a later pass read from the
                  chain 4 CUs before it (the first such word that masks a live gradient)"""
    nx, B, L, H = case.nx, case.B, case.layers, case.hidden
    N = B * nx
    hs, x = T["hs"], T["x"]
    fused = fused_chain(case.in_dim, H, L, nx)
    out = {}

    def dropped(rows):
        d = {"input_mlp.0.weight": -G[0][rows].T @ x[rows], "input_mlp.0.bias": -G[0][rows].sum(0)}
        for l in range(L):
            d[f"update_mlps.{l}.0.weight"] = -G[l + 1][rows].T @ stencil_rows(hs[l], B, nx, rows)
            d[f"update_mlps.{l}.0.bias"] = -G[l + 1][rows].sum(0)
        return d

    if fused and fused_passes(B, cus) > 1:
        out["pass2"] = dropped(np.arange(train_blocks(B, cus) * NW * nx, N))
    if fused and B % NW:
        out["ragged"] = dropped(np.arange((B - B % NW) * nx, N))
    if L >= 1 and nx > 1 and B > 1:
        r0 = np.arange(B) * nx
        out["halo"] = {f"update_mlps.{l}.0.weight":
                       G[l + 1][r0].T @ (stencil_rows(hs[l], B, nx, r0, True) - stencil_rows(hs[l], B, nx, r0))
                       for l in range(L)}
    geo = {"edge_mlp.0.weight": tgemm_splits(N, WGRAD_SPLITS)}
    lay = layer_splits(case.in_dim, H, L, nx, N)
    for l in range(L):
        geo[f"update_mlps.{l}.0.weight"] = lay[1:]
    for tag, pick in (("stage0", lambda S: 0), ("stageZ", lambda S: S - 1)):
        d = {}
        for k, (rsplit, S) in geo.items():
            rows = last_stage_rows(N, rsplit, pick(S))
            if k.startswith("edge"):
                gw = -dPQ[rows].T @ hs[L][rows]
                d[k] = np.concatenate([gw[:H], gw[H:]], 1)
            else:
                l = int(k.split(".")[1])
                d[k] = -G[l + 1][rows].T @ stencil_rows(hs[l], B, nx, rows)
        out[tag] = d
    if fused and fused_passes(B, cus) > 1:
        out["maskword"] = _maskword(case, b, T, cus)
    return out


def _maskword(case, b, T, cus):
    nx, B = case.nx, case.B
    back = train_blocks(B, cus) * NW
    for c in range(back, B):
        sub, gup = chains(T, b.gup, c, c + 1)
        ref, _, _, pre = backward64(b.sd, sub, gup, keep_pre=True)
        own, other = sub["hs"][0] > 0, chains(T, b.gup, c - back, c - back + 1)[0]["hs"][0] > 0
        for cell in range(nx):
            for g in range(4):
                row, ch = mask_word(nx, cell, g)
                if np.any((own[row, ch] != other[row, ch]) & (pre[0][row, ch] != 0)):
                    masks = [h > 0 for h in sub["hs"]]
                    masks[0] = masks[0].copy()
                    masks[0][row, ch] = other[row, ch]
                    got = backward64(b.sd, sub, gup, masks=masks)[0]
                    d = {k: got[k] - ref[k] for k in ref if k != "node_features"}
                    d["node_features"] = np.zeros_like(b.grads["node_features"])
                    d["node_features"][c * nx:(c + 1) * nx] = got["node_features"] - ref["node_features"]
                    return d
    return {}
