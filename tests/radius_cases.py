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
the pinned references, sharpness under three mutants) and
tests/test_gpu_radius.py (the kernels) both run.  Seeds are searched on the CPU
only, as exact_cases.find_case does.
"""
import numpy as np

import exact_cases as X

MAX_RADIUS = 3


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


def windowed64(sd, nf, B, nx, R, halo):
    """The windowed flux kernel restated: 64-cell windows starting at cell
    w * faces - halo (mod nx), each a periodic 64-chain of its own (the wrap is
    artificial), faces [halo, halo + faces) of a window kept, faces = 64 - 2 halo
    - 1.  With halo = L * R every kept face is exact; a smaller halo keeps faces
    the wrap has reached.  Returns flux [B, 2nx]."""
    faces = 64 - 2 * halo - 1
    assert faces >= 1
    x = np.asarray(nf, np.float64).reshape(B, nx, -1)
    out = np.zeros((B, 2 * nx))
    for w in range((nx + faces - 1) // faces):
        cells = (w * faces - halo + np.arange(64)) % nx
        fe, _ = forward64_radius(sd, x[:, cells].reshape(B * 64, -1), B, 64, R, record=False)
        for k in range(halo, halo + faces):
            f = w * faces + (k - halo)
            if f < nx:
                out[:, f], out[:, nx + f] = fe[:, k], fe[:, 64 + k]
    return out


# --------------------------------------------------------------------- case table
class RCase:
    """kind "flux": hf_chain_flux / FluxGNN.forward; "rollout": zero_x weights and
    an integer state (the rollout kernels).  fused: nx = 16 MT."""

    def __init__(self, name, kind, nx, B, layers, R):
        self.name, self.kind, self.nx, self.B, self.layers, self.R = name, kind, nx, B, layers, R
        self.zero_x = kind == "rollout"
        self.fused = nx in (16, 32, 48, 64)
        self.seed0, self.hi = 0, 4

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
    faces = 64 - 2 * L - 1
    zone = np.zeros(nx, bool)
    for w in range((nx + faces - 1) // faces):
        for k in range(L, L + faces):
            f = w * faces + (k - L)
            if f < nx and (k < L * R or k > 62 - L * R):
                zone[f] = True
    return zone


def mutants(case, sd, nf, flux):
    """Fractions of faces the three mutants change (the windowed one: of the
    faces of halo_zone, and only for the windowed cases)."""
    a = (case.B, case.nx, case.R)
    out = {"drop": changed_faces(forward64_radius(sd, nf, *a, record=False, mutant="drop")[0], flux, case.nx),
           "twice": changed_faces(forward64_radius(sd, nf, *a, record=False, mutant="twice")[0], flux, case.nx)}
    if not case.fused:
        wm = windowed64(sd, nf, case.B, case.nx, case.R, case.layers)
        zone = halo_zone(case)
        diff = (wm[:, :case.nx] != flux[:, :case.nx]) | (wm[:, case.nx:] != flux[:, case.nx:2 * case.nx])
        out["halo"] = float(diff[:, zone].mean())
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
    nonzero, and each mutant changes more than half of the faces."""
    if not b.rec.valid("f32"):
        return [f"not valid for f32: bound {b.rec.max_bound():.3g} * 2^{b.rec.m}"]
    bad = []
    if np.mean(b.flux != 0) < 0.9:
        bad.append(f"nonzero fluxes {np.mean(b.flux != 0):.3f} < 0.9")
    for k, v in mutants(b.case, b.sd, b.nf, b.flux_all).items():
        if v <= 0.5:
            bad.append(f"mutant {k} changes {v:.3f} of the faces")
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
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and not set(BY_NAME) & set(X.BY_NAME)


def cases(kind, fused=None):
    return [c for c in CASES if c.kind == kind and (fused is None or c.fused == fused)]
