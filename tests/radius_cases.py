"""Exact-input cases of FluxGNN on the radius-R chain graph (a plain helper
module, built on tests/exact_cases.py).

The radius-R chain graph of nx cells (1 <= R <= 3, nx >= 2R + 1) is, per IC, a
block of 2*R*nx edges: for r = 1..R in order the nx edges i -> (i+r) mod nx,
then the nx edges (i+r) mod nx -> i.  FluxGNN.forward on it is the reference's
forward unchanged (mean over the 2R neighbours, readout on every edge); the
solver reads only the first 2nx fluxes of a block.  The neighbour sum is formed
in the order ((((h[i+1] + h[i-1]) + h[i+2]) + h[i-2]) + h[i+3]) + h[i-3] and the
1/deg is folded into W_b as w / (2R).

The exact recipe: exact_cases.make_sd with the W_b half multiplied by R, so its
entries are +-2R and W_b / (2R) = +-1.  `forward64_radius` multiplies INTEGER
neighbour sums by that exact +-1: every value of the forward is an integer in
float64 for R = 3 too, where a mean s / 6 is not a binary fraction.  The fused
radius kernels (weights packed as w / (2R), sums of integers) must reproduce it
bit for bit.

CASES is the one table tests/test_radius_cases_cpu.py (validity, agreement with
the pinned references, sharpness under four mutants, every figure of a row's
`why` recomputed from csrc/) and tests/test_gpu_radius.py /
tests/test_gpu_radius_regimes.py (the kernels) both run.  Seeds are searched on
the CPU only, as exact_cases.find_case does.

The regime of a row (`regime`): a fused row (nx = 16 MT) is B items, one IC per
wave; any other nx runs 64-cell windows of F = 63 - 2 L R exact faces, nwin =
ceil(nx / F) windows per IC (the last keeps nx - (nwin - 1) F faces), B * nwin
items.  NW = 4 items make a group, one workgroup per CU takes groups blockIdx.x,
blockIdx.x + gridDim.x, ...: `passes` of the persistent loop, counted on 256 CUs.

The order recipe (`order_sd`, `forward32_order`): float32 inputs on which the
ORDER of the neighbour sum shows in the bits, and nothing else does.
"""
import numpy as np

import exact_cases as X

MAX_RADIUS = 3

# csrc/ constants the table's figures rest on (tests/test_radius_cases_cpu.py reads them out of the sources)
WIN_CELLS = 64           # hf_internal.h kWinCells = 16 * CoreF32T::kWinMT
WIN_MT = 4               # CoreF32T::kWinMT
MAX_LAYERS = 8           # hf_internal.h kMaxChainLayers
NW = 4                   # CoreF32T::kNW = chain_common.h kWaves: items per group
WG_PER_CU = 1            # CoreF32T::kWGPerCU
CUS = 256                # the CU count the `why` figures are written for
LANE_MIN_CELLS = 1 << 20  # capi.cpp kLaneMinCells
DEFAULT_LANES = 3        # capi.cpp kDefaultLanes
FUSED_NX = (16, 32, 48, 64)


def cdiv(a, b):
    return -(-a // b)


def win_faces(halo):
    """hf_internal.h win_faces_of: exact faces of a 64-cell window of that halo."""
    return WIN_CELLS - 2 * halo - 1


def regime(nx, B, L, R, cus=CUS):
    """The figures of chain_common.h's flux_launch / launch_flux_windowed for
    hf_chain_flux on B chains of nx cells, L layers, radius R, on `cus` CUs."""
    fused = nx in FUSED_NX
    r = {"fused": fused, "halo": L * R}
    if fused:
        r.update(F=None, nwin=1, keeps=nx)
    else:
        F = win_faces(L * R)
        assert F >= 1
        nwin = cdiv(nx, F)
        r.update(F=F, nwin=nwin, keeps=nx - (nwin - 1) * F)
    items = B * r["nwin"]
    groups, res = cdiv(items, NW), cus * WG_PER_CU
    passes = cdiv(groups, res)
    r.update(items=items, groups=groups, passes=passes, pass2=groups - res if passes > 1 else 0,
             live=items - (groups - 1) * NW, first_later_item=res * NW)
    return r


def lanes(nx, B):
    """capi.cpp run_lanes: lane streams of an hf_run of B x nx cells, and the even split's cuts."""
    n = DEFAULT_LANES
    while n > 1 and B * nx < n * LANE_MIN_CELLS:
        n -= 1
    return n, [B * k // n for k in range(n + 1)]


def radius_edges(nx, B=1, R=1):
    """[2, B*2*R*nx] int64 numpy: the definition above (R = 1: exact_cases.chain_edges)."""
    assert 1 <= R <= MAX_RADIUS and (R == 1 or nx >= 2 * R + 1)
    src = np.arange(nx)
    rows, cols = [], []
    for r in range(1, R + 1):
        dst = (src + r) % nx
        rows += [src, dst]
        cols += [dst, src]
    row, col = np.concatenate(rows), np.concatenate(cols)
    off = (np.arange(B) * nx)[:, None]
    return np.stack([(row + off).reshape(-1), (col + off).reshape(-1)]).astype(np.int64)


def make_sd_radius(layers, seed, R, zero_x=False):
    """exact_cases.make_sd with the W_b half of every update layer multiplied by
    R: entries +-2R, so W_b / (2R) = +-1 exactly."""
    sd = X.make_sd(layers, seed, zero_x=zero_x)
    H = sd["input_mlp.0.weight"].shape[0]
    for l in range(layers):
        W = np.array(sd[f"update_mlps.{l}.0.weight"])
        W[:, H:] *= R
        sd[f"update_mlps.{l}.0.weight"] = W
    return sd


def nb_sum(h3, R, mutant=None):
    """Integer neighbour sum of h3 [B, nx, H] in the fixed order.  mutant:
    "drop" leaves the +-R neighbours out, "twice" takes i+R in place of i-R."""
    s = None
    for r in range(1, R + 1):
        plus, minus = np.roll(h3, -r, axis=1), np.roll(h3, r, axis=1)
        if r == R and R > 1 and mutant == "drop":
            continue
        if r == R and mutant == "twice":
            minus = plus
        s = plus + minus if s is None else (s + plus) + minus
    return s


def forward64_radius(sd, nf, B, nx, R, all_edges=False, record=True, mutant=None):
    """float64 forward on B radius-R chains: input layer, L layers of h = ReLU(W_a h
    + (W_b / (2R)) nbsum(h) + b) with INTEGER neighbour sums, the edge MLP on
    [h_row ; h_col].  Returns (flux, Record or None): flux [B, 2nx], the first
    2nx edges of every IC (what the solver and the fused kernels use), or with
    all_edges [B, 2*R*nx].  The Record is exact_cases': representability, the
    absolute-sum bound of every linear map, the dyadic depth."""
    f64 = np.float64
    W = {k: np.asarray(v, f64) for k, v in sd.items()}
    L = X.n_layers(sd)
    rec = X.Record() if record else None
    x = np.asarray(nf, f64).reshape(B * nx, -1)

    def linear(name, xs, Ws, b, relu_layer=True):
        y = sum(a @ w.T for a, w in zip(xs, Ws)) + b
        if rec is not None:
            rec.bound[name] = float((sum(np.abs(a).max(0) @ np.abs(w).T for a, w in zip(xs, Ws)) + np.abs(b)).max())
            if relu_layer:
                rec.zero_frac[name] = float(np.mean(y == 0))
        return y

    h = np.maximum(linear("input", [x], [W["input_mlp.0.weight"]], W["input_mlp.0.bias"]), 0)
    H = h.shape[1]
    for l in range(L):
        Wl = W[f"update_mlps.{l}.0.weight"]
        Wb = Wl[:, H:] / (2 * R)
        assert np.array_equal(Wb, np.rint(Wb)), "W_b / (2R) must be an integer matrix (make_sd_radius)"
        s = nb_sum(h.reshape(B, nx, H), R, mutant).reshape(h.shape)
        if rec is not None:
            rec.max_act = max(rec.max_act, float(h.max()))
        h = np.maximum(linear(f"layer{l}", [h, s], [Wl[:, :H], Wb], W[f"update_mlps.{l}.0.bias"]), 0)
    if rec is not None:
        rec.max_act = max(rec.max_act, float(h.max()))
    We, be = W["edge_mlp.0.weight"], W["edge_mlp.0.bias"]
    w2, b2 = W["edge_mlp.2.weight"], W["edge_mlp.2.bias"]
    h3 = h.reshape(B, nx, H)
    blocks_r, blocks_c = [], []
    for r in range(1, (R if all_edges else 1) + 1):
        far = np.roll(h3, -r, axis=1)
        blocks_r += [h3, far]
        blocks_c += [far, h3]
    hr = np.concatenate(blocks_r, axis=1).reshape(-1, H)
    hc = np.concatenate(blocks_c, axis=1).reshape(-1, H)
    z = np.maximum(linear("edge0", [hr, hc], [We[:, :H], We[:, H:]], be), 0)
    flux = linear("edge2", [z], [w2], b2, relu_layer=False)[:, 0].reshape(B, -1)
    if rec is not None:
        rec.m = X.dyadic_bits(flux, h)
    return flux, rec


def faces_of(flux, nx):
    """F[i] = 0.5 (fe[i] + fe[nx + i]) of the first 2nx edges [B, >= 2nx]."""
    return 0.5 * (flux[:, :nx] + flux[:, nx:2 * nx])


def windowed64(sd, nf, B, nx, R, halo, drop_last=False):
    """The windowed flux kernel restated: 64-cell windows starting at cell
    w * faces - halo (mod nx), each a periodic 64-chain of its own (the wrap is
    artificial), faces [halo, halo + faces) of a window kept, faces = 64 - 2 halo
    - 1.  With halo = L * R every kept face is exact, for R = 2 as for R = 3 and
    for a chain shorter than the window; a smaller halo keeps faces the wrap has
    reached.  drop_last: the last window's faces stay zero (nwin one short).
    Returns flux [B, 2nx]."""
    faces = win_faces(halo)
    assert faces >= 1
    x = np.asarray(nf, np.float64).reshape(B, nx, -1)
    out = np.zeros((B, 2 * nx))
    nwin = cdiv(nx, faces)
    for w in range(nwin - 1 if drop_last else nwin):
        cells = (w * faces - halo + np.arange(WIN_CELLS)) % nx
        fe, _ = forward64_radius(sd, x[:, cells].reshape(B * WIN_CELLS, -1), B, WIN_CELLS, R, record=False)
        for k in range(halo, halo + faces):
            f = w * faces + (k - halo)
            if f < nx:
                out[:, f], out[:, nx + f] = fe[:, k], fe[:, WIN_CELLS + k]
    return out


# --------------------------------------------------------------------- case table
class RCase:
    """kind "flux": hf_chain_flux / FluxGNN.forward; "rollout": zero_x weights and
    an integer state (the rollout kernels).  fused: nx = 16 MT."""

    def __init__(self, name, kind, nx, B, layers, R, hi=4, why=None):
        self.name, self.kind, self.nx, self.B, self.layers, self.R = name, kind, nx, B, layers, R
        self.zero_x = kind == "rollout"
        self.fused = nx in FUSED_NX
        self.seed0, self.hi = 0, hi
        self.why = why            # the regime a row reaches, with its figures (None: the first table's rows)

    def regime(self, cus=CUS):
        return regime(self.nx, self.B, self.layers, self.R, cus)

    def __repr__(self):
        return self.name

    def inputs(self, seed):
        sd = make_sd_radius(self.layers, seed, self.R, zero_x=self.zero_x)
        nf = X.features(self.B, self.nx, seed, self.hi)
        if self.zero_x:
            nf[:, 3] = 0
        return sd, nf

    def state0(self, nf):
        return np.ascontiguousarray(nf.reshape(self.B, self.nx, 4)[:, :, :3].transpose(0, 2, 1))


def changed_faces(a, b, nx):
    """Fraction of (IC, face) pairs whose flux, either direction, differs."""
    return float(np.mean((a[:, :nx] != b[:, :nx]) | (a[:, nx:2 * nx] != b[:, nx:2 * nx])))


def halo_zone(case):
    """Faces a window of halo L (instead of L * R) keeps although the wrap has
    reached them: window positions [L, L*R) and (62 - L*R, 62 - L] of each of the
    mutant's windows.  Boolean [nx]."""
    L, R, nx = case.layers, case.R, case.nx
    faces = win_faces(L)
    zone = np.zeros(nx, bool)
    for w in range(cdiv(nx, faces)):
        for k in range(L, L + faces):
            f = w * faces + (k - L)
            if f < nx and (k < L * R or k > WIN_CELLS - 2 - L * R):
                zone[f] = True
    return zone


def last_window(case):
    """Faces the last window of a windowed case keeps (regime()'s `keeps`).  Boolean [nx]."""
    r = case.regime()
    zone = np.zeros(case.nx, bool)
    zone[(r["nwin"] - 1) * r["F"]:] = True
    assert int(zone.sum()) == r["keeps"]
    return zone


def later_pass_faces(case, cus=CUS):
    """(IC, face) pairs the later passes of the persistent loop write (items from
    4 * cus on: whole ICs of a fused case, windows of a windowed one).  Boolean [B, nx]."""
    r = case.regime(cus)
    mask = np.zeros((case.B, case.nx), bool)
    for item in range(r["first_later_item"], r["items"]):
        b, w = divmod(item, r["nwin"])
        if case.fused:
            mask[b] = True
        else:
            mask[b, w * r["F"]:min((w + 1) * r["F"], case.nx)] = True
    return mask


def applicable(case):
    """The mutants that can change a case: "drop" and "twice" need a layer (at
    L = 0 no neighbour sum is formed), "halo" a windowed case whose halo L * R
    exceeds L, "last" a windowed case."""
    want = {"drop", "twice"} if case.layers >= 1 else set()
    if not case.fused:
        want.add("last")
        if case.layers >= 1:
            want.add("halo")
    return want


def mutants(case, sd, nf, flux):
    """Fractions of faces the four mutants change, of the faces each can reach:
    "drop" and "twice" of all faces; "halo" (windows of halo L) of halo_zone;
    "last" (the last window's faces left at zero) of last_window.  Only those of
    applicable(case)."""
    a = (case.B, case.nx, case.R)
    nx, want, out = case.nx, applicable(case), {}
    for k in ("drop", "twice"):
        if k in want:
            out[k] = changed_faces(forward64_radius(sd, nf, *a, record=False, mutant=k)[0], flux, nx)
    for k, zone, kw in (("halo", halo_zone, dict(halo=case.layers)),
                        ("last", last_window, dict(halo=case.layers * case.R, drop_last=True))):
        if k in want:
            wm = windowed64(sd, nf, *a, **kw)
            diff = (wm[:, :nx] != flux[:, :nx]) | (wm[:, nx:] != flux[:, nx:2 * nx])
            out[k] = float(diff[:, zone(case)].mean())
    return out


def build(case, seed):
    b = X.Built()
    b.case, b.seed = case, seed
    b.sd, b.nf = case.inputs(seed)
    b.flux_all, b.rec = forward64_radius(b.sd, b.nf, case.B, case.nx, case.R, all_edges=True)
    b.flux = np.ascontiguousarray(b.flux_all[:, :2 * case.nx])
    b.faces = faces_of(b.flux, case.nx)
    b.rec.m = max(b.rec.m, X.dyadic_bits(b.faces))
    b.ei = radius_edges(case.nx, case.B, case.R)
    return b


def accept(b):
    """Why this seed is not taken ([] = taken): valid for f32, nearly every flux
    nonzero, and each applicable mutant changes more than half of the faces it
    can reach.  At L = 0 no neighbour sum exists for "drop" and "twice" to
    change; in their place the flux must be the radius-1 forward of the same
    state dict (exact_cases.forward64): the radius cannot enter."""
    if not b.rec.valid("f32"):
        return [f"not valid for f32: bound {b.rec.max_bound():.3g} * 2^{b.rec.m}"]
    bad = []
    if np.mean(b.flux != 0) < 0.9:
        bad.append(f"nonzero fluxes {np.mean(b.flux != 0):.3f} < 0.9")
    if b.case.layers == 0 and not np.array_equal(X.forward64(b.sd, b.nf, b.case.B, b.case.nx, record=False)[0], b.flux):
        bad.append("L = 0: the flux is not the radius-1 forward")
    for k, v in mutants(b.case, b.sd, b.nf, b.flux_all).items():
        if v <= 0.5:
            bad.append(f"mutant {k} changes {v:.3f} of the faces it can reach")
    return bad


def find_case(case):
    return X.find_case(case, build=build, accept=accept)


def _table():
    T = []
    # fused kernels, nx = 16 MT: MT = 1..4 differ in which neighbours cross the
    # tile seam; B = 5 leaves a ragged last workgroup of 4 waves
    for kind in ("flux", "rollout"):
        for nx in (16, 32, 48, 64):
            for R in (2, 3):
                for L in (1, 4):
                    T.append(RCase(f"r{kind}_nx{nx}_R{R}_L{L}", kind, nx, 5, L, R))
    # windowed kernel: the smallest legal chain at R = 3, wrapped many times
    # inside a window; 100 and 128 cells at L = 4, R = 3 (39 faces per window:
    # three and four windows, a seam mid-chain)
    T.append(RCase("rwin_nx7_R3_L4", "flux", 7, 3, 4, 3))
    T.append(RCase("rwin_nx100_R3_L4", "flux", 100, 3, 4, 3))
    T.append(RCase("rwin_nx128_R3_L4", "flux", 128, 3, 4, 3))
    return T + _regimes()


def _regimes():
    """The regime rows.  Every `why` names the regime and its figures (F faces per
    window, nwin windows per IC of which the last keeps `keeps` faces, items,
    groups of 4, passes of the persistent loop on 256 CUs, pass2 groups in the
    second pass, live waves of the last group); tests/test_radius_cases_cpu.py
    recomputes each from csrc/."""
    T = []

    def row(name, kind, nx, B, L, R, why, hi=4):
        T.append(RCase(name, kind, nx, B, L, R, hi=hi, why=why))

    # ---- fused flux, the remaining depths (B = 5: items = 5, groups = 2, passes = 1, live = 1)
    b5 = "items = 5, groups = 2, passes = 1, live = 1"
    for nx in (48, 64):
        for R in (2, 3):
            row(f"rflux_nx{nx}_R{R}_L8", "flux", nx, 5, 8, R,
                f"fused, the deepest model (kMaxChainLayers = 8 layers of the radius core's operand pipeline); {b5}")
    for R in (2, 3):
        row(f"rflux_nx32_R{R}_L2", "flux", 32, 5, 2, R, f"fused, two layers: one hand-over between layer steps; {b5}")
    row("rflux_nx64_R3_L0", "flux", 64, 5, 0, 3,
        f"fused, no layer: the radius core with no neighbour sum at all, equal to the radius-1 forward; {b5}")
    # ---- fused flux, a later pass of the persistent loop
    p2 = "items = 1029, groups = 258, passes = 2, pass2 = 2, live = 1"
    row("rpersist_nx64_B1029_R2_L4", "flux", 64, 1029, 4, 2, hi=2,
        why=f"fused, MT = 4, second pass of chain_flux_kernel's loop on the prefetched features, its last group one "
            f"live wave; features in {{0, 1}} (hi = 2); {p2}")
    row("rpersist_nx16_B1029_R3_L1", "flux", 16, 1029, 1, 3,
        f"fused, MT = 1, second pass of the persistent loop, its last group one live wave; {p2}")
    # ---- windowed flux, the window-count boundaries (B = 3)
    for nx, fig in ((39, "nwin = 1, keeps = 39, items = 3, groups = 1, passes = 1, live = 3"),
                    (40, "nwin = 2, keeps = 1, items = 6, groups = 2, passes = 1, live = 2"),
                    (79, "nwin = 3, keeps = 1, items = 9, groups = 3, passes = 1, live = 1")):
        row(f"rwin_nx{nx}_R3_L4", "flux", nx, 3, 4, 3, f"window-count boundary of halo = 12, F = 39; {fig}")
    for nx, fig in ((47, "nwin = 1, keeps = 47, items = 3, groups = 1, passes = 1, live = 3"),
                    (94, "nwin = 2, keeps = 47, items = 6, groups = 2, passes = 1, live = 2"),
                    (95, "nwin = 3, keeps = 1, items = 9, groups = 3, passes = 1, live = 1")):
        row(f"rwin_nx{nx}_R2_L4", "flux", nx, 3, 4, 2,
            f"the R = 2 windowed kernel, window-count boundary of halo = 8, F = 47; {fig}")
    for nx, fig in ((15, "nwin = 1, keeps = 15, items = 3, groups = 1, passes = 1, live = 3"),
                    (31, "nwin = 3, keeps = 1, items = 9, groups = 3, passes = 1, live = 1"),
                    (100, "nwin = 7, keeps = 10, items = 21, groups = 6, passes = 1, live = 1")):
        row(f"rwin_nx{nx}_R3_L8", "flux", nx, 3, 8, 3,
            f"the tightest window (L = 8, R = 3), halo = 24, F = 15; {fig}")
    for nx, fig in ((63, "nwin = 3, keeps = 1"), (65, "nwin = 3, keeps = 3")):
        row(f"rwin_nx{nx}_R2_L8", "flux", nx, 3, 8, 2,
            f"R = 2 at eight layers, halo = 16, F = 31; {fig}, items = 9, groups = 3, passes = 1, live = 1")
    row("rwin_nx100_R3_L0", "flux", 100, 3, 0, 3,
        "windowed, no layer: halo = 0, F = 63; nwin = 2, keeps = 37, items = 6, groups = 2, passes = 1, live = 2")
    for L, fig in ((1, "halo = 2, F = 59; nwin = 2, keeps = 41"), (2, "halo = 4, F = 55; nwin = 2, keeps = 45"),
                   (3, "halo = 6, F = 51; nwin = 2, keeps = 49")):
        row(f"rwin_nx100_R2_L{L}", "flux", 100, 3, L, 2,
            f"the R = 2 windowed kernel at the remaining depths, {fig}, items = 6, groups = 2, passes = 1, live = 2")
    # ---- windowed flux, chains shorter than a window (the chain wraps inside it)
    row("rwin_nx5_R2_L4", "flux", 5, 3, 4, 2,
        "the smallest legal chain at R = 2, wrapped 12 times in a window: halo = 8, F = 47; nwin = 1, keeps = 5, "
        "items = 3, groups = 1, passes = 1, live = 3")
    row("rwin_nx17_R3_L4", "flux", 17, 3, 4, 3,
        "a chain of 17 wrapped inside its window: halo = 12, F = 39; nwin = 1, keeps = 17, items = 3, groups = 1, "
        "passes = 1, live = 3")
    row("rwin_nx63_R3_L1", "flux", 63, 3, 1, 3,
        "one cell short of the window, yet two windows of faces: halo = 3, F = 57; nwin = 2, keeps = 6, items = 6, "
        "groups = 2, passes = 1, live = 2")
    # ---- windowed flux, long chains
    row("rwin_nx1024_R3_L4", "flux", 1024, 3, 4, 3,
        "long chain: halo = 12, F = 39; nwin = 27, keeps = 10, items = 81, groups = 21, passes = 1, live = 1")
    row("rwin_nx1024_R2_L1", "flux", 1024, 3, 1, 2,
        "long chain: halo = 2, F = 59; nwin = 18, keeps = 21, items = 54, groups = 14, passes = 1, live = 2")
    # ---- windowed flux, a later pass of the persistent loop
    row("rpersistwin_nx100_B150_R3_L8", "flux", 100, 150, 8, 3, hi=2,
        why="windowed, second pass of the persistent loop at the tightest window, its last group two live waves; "
            "features in {0, 1} (hi = 2); halo = 24, F = 15; nwin = 7, keeps = 10, items = 1050, groups = 263, "
            "passes = 2, pass2 = 7, live = 2")
    # ---- rollouts at unfused nx: the per-step path (launch_chain_flux on the state, then FV)
    for nx, R, L, fig in ((100, 2, 1, "halo = 2, F = 59; nwin = 2, keeps = 41, items = 6, groups = 2, passes = 1, live = 2"),
                          (100, 2, 4, "halo = 8, F = 47; nwin = 3, keeps = 6, items = 9, groups = 3, passes = 1, live = 1"),
                          (100, 3, 4, "halo = 12, F = 39; nwin = 3, keeps = 22, items = 9, groups = 3, passes = 1, live = 1"),
                          (1024, 3, 4, "halo = 12, F = 39; nwin = 27, keeps = 10, items = 81, groups = 21, passes = 1, "
                                       "live = 1")):
        row(f"rrollout_nx{nx}_R{R}_L{L}", "rollout", nx, 3, L, R,
            f"per-step rollout: the windowed kernel reads the state and x and stores the face flux; {fig}")
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and not set(BY_NAME) & set(X.BY_NAME)


def cases(kind, fused=None):
    return [c for c in CASES if c.kind == kind and (fused is None or c.fused == fused)]


# ------------------------------------------------------------------ the order recipe
# Float32 inputs on which the ORDER of the neighbour sum shows and nothing else
# can: every weight matrix has one nonzero per row, so every linear map's output
# is one product by 1, or the sum of exactly two such products (W_a h + (W_b/2R)
# s; the two halves of edge_mlp.0) plus a zero bias.  Whatever the accumulation
# order of a kernel, a float32 sum of two terms and zeros is the one rounding of
# that add.  All values are positive, so ReLU never clips.  The one float32 sum
# of more than two terms left in the forward is the neighbour sum.
ORDERS = ("fixed", "pairwise", "reversed")
ORDER_MIN_CHANGED = 0.05   # each wrong order must change this fraction of a case's observed fluxes


def order_sd(layers, seed, R, k0, hidden=128, in_dim=4):
    """FluxGNN state dict (reference keys, float32) of the order recipe: input rows
    +1 on one of the features; W_a rows +1 at a permutation's column, W_b rows 2R
    at another's (packed as w / (2R) = 1 exactly); the two halves of edge_mlp.0
    +1 at two permutations; every bias 0; edge_mlp.2.weight one-hot at k0."""
    g = np.random.default_rng([seed, layers, R, 4242])
    H = hidden

    def perm(value):
        W = np.zeros((H, H))
        W[np.arange(H), g.permutation(H)] = value
        return W

    Win = np.zeros((H, in_dim))
    Win[np.arange(H), g.integers(0, in_dim, H)] = 1.0
    sd = {"input_mlp.0.weight": Win, "input_mlp.0.bias": np.zeros(H)}
    for l in range(layers):
        sd[f"update_mlps.{l}.0.weight"] = np.concatenate([perm(1.0), perm(2.0 * R)], axis=1)
        sd[f"update_mlps.{l}.0.bias"] = np.zeros(H)
    sd["edge_mlp.0.weight"] = np.concatenate([perm(1.0), perm(1.0)], axis=1)
    sd["edge_mlp.0.bias"] = np.zeros(H)
    w2 = np.zeros((1, H))
    w2[0, k0] = 1.0
    sd["edge_mlp.2.weight"], sd["edge_mlp.2.bias"] = w2, np.zeros(1)
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


def order_features(B, nx, seed, in_dim=4):
    """[B*nx, in_dim] float32 draws from U(0.1, 2): deliberately not dyadic."""
    g = np.random.default_rng([seed, B, nx, 4243])
    return g.uniform(0.1, 2.0, (B * nx, in_dim)).astype(np.float32)


def nb_sum32(h3, R, order):
    """float32 neighbour sum of h3 [B, nx, H], one rounding per add, in `order`:
    "fixed" ((((p1 + m1) + p2) + m2) + p3) + m3 (chain_common.h
    nb_sum_radius, the edge list's own order); "pairwise" ((p1 + m1) + (p2 + m2))
    + (p3 + m3); "reversed" ((((m3 + p3) + m2) + p2) + m1) + p1."""
    assert h3.dtype == np.float32
    p = [np.roll(h3, -r, axis=1) for r in range(1, R + 1)]
    m = [np.roll(h3, r, axis=1) for r in range(1, R + 1)]
    if order == "fixed":
        s = p[0] + m[0]
        for r in range(1, R):
            s = (s + p[r]) + m[r]
    elif order == "pairwise":
        s = p[0] + m[0]
        for r in range(1, R):
            s = s + (p[r] + m[r])
    elif order == "reversed":
        s = m[R - 1] + p[R - 1]
        for r in range(R - 2, -1, -1):
            s = (s + m[r]) + p[r]
    else:
        raise ValueError(order)
    assert s.dtype == np.float32
    return s


def _one_per_row(W):
    """(column, value) of the single nonzero of every row of W."""
    assert np.all((W != 0).sum(1) == 1), "the order recipe: one nonzero per row"
    c = np.argmax(W != 0, axis=1)
    return c, W[np.arange(W.shape[0]), c]


def forward32_order(sd, nf, B, nx, R, order="fixed", all_edges=False):
    """float32 numpy forward of an order_sd model on B radius-R chains, one
    rounding after every add, the neighbour sum in `order`.  Every linear map is
    evaluated as what it is on this recipe: y[:, o] = x[:, c(o)] * w(o) (one exact
    product by 1), the two-input maps as the float32 sum of their two products.
    Returns flux [B, 2nx] float32 (all_edges: [B, 2*R*nx])."""
    f32 = np.float32
    W = {k: np.asarray(v, f32) for k, v in sd.items()}
    L = X.n_layers(sd)
    assert all(not np.any(v) for k, v in W.items() if k.endswith("bias")), "the order recipe: zero biases"
    x = np.asarray(nf, f32).reshape(B * nx, -1)
    c, w = _one_per_row(W["input_mlp.0.weight"])
    h = np.maximum(x[:, c] * w, f32(0))
    H = h.shape[1]
    for l in range(L):
        Wl = W[f"update_mlps.{l}.0.weight"]
        ca, wa = _one_per_row(Wl[:, :H])
        cb, wb = _one_per_row(Wl[:, H:])
        wb = (wb / f32(2 * R)).astype(f32)
        assert np.all(wa == 1) and np.all(wb == 1)
        s = nb_sum32(h.reshape(B, nx, H), R, order).reshape(h.shape)
        h = np.maximum(h[:, ca] * wa + s[:, cb] * wb, f32(0))
    h3 = h.reshape(B, nx, H)
    cr, wr = _one_per_row(W["edge_mlp.0.weight"][:, :H])
    cc, wc = _one_per_row(W["edge_mlp.0.weight"][:, H:])
    k0, w2 = _one_per_row(W["edge_mlp.2.weight"])
    blocks = []
    for r in range(1, (R if all_edges else 1) + 1):
        far = np.roll(h3, -r, axis=1)
        for hr, hc in ((h3, far), (far, h3)):
            z = np.maximum(hr[:, :, cr] * wr + hc[:, :, cc] * wc, f32(0))
            blocks.append(z[:, :, k0[0]] * w2[0])
    flux = np.concatenate(blocks, axis=1)
    assert flux.dtype == f32 and h.min() > 0
    return flux


class OrderCase:
    def __init__(self, nx, R, layers, k0, B=5):
        self.nx, self.R, self.layers, self.k0, self.B = nx, R, layers, k0, B
        self.name = f"order_nx{nx}_R{R}_L{layers}_k{k0}"

    def __repr__(self):
        return self.name


ORDER_K0 = (0, 37, 90, 127)
ORDER_CASES = [OrderCase(nx, R, L, k0) for R in (2, 3) for L in (1, 4) for nx in (16, 64, 100) for k0 in ORDER_K0]
_ORDER_BUILT = {}


def changed_fluxes(a, b):
    return float(np.mean(a != b))


def find_order_case(case):
    """The order case at the first seed (of exact_cases.SEEDS) at which each wrong
    order changes at least ORDER_MIN_CHANGED of the observed fluxes (the first 2nx
    per IC): chosen on the float32 reference alone.  Cached."""
    if case.name not in _ORDER_BUILT:
        for seed in range(X.SEEDS):
            b = X.Built()
            b.case, b.seed = case, seed
            b.sd = order_sd(case.layers, seed, case.R, case.k0)
            b.nf = order_features(case.B, case.nx, seed)
            b.flux = forward32_order(b.sd, b.nf, case.B, case.nx, case.R, "fixed")
            b.changed = {o: changed_fluxes(forward32_order(b.sd, b.nf, case.B, case.nx, case.R, o), b.flux)
                         for o in ORDERS[1:]}
            if min(b.changed.values()) >= ORDER_MIN_CHANGED:
                _ORDER_BUILT[case.name] = b
                break
        else:
            raise RuntimeError(f"no seed for {case.name}")
    return _ORDER_BUILT[case.name]
