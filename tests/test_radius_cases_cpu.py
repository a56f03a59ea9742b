"""CPU checks of the radius-graph cases (tests/radius_cases.py) and of the
radius option's host side, without a device:

  edges       radius_edges(., ., 1) is exact_cases.chain_edges; the package's
              chain_edge_index(radius=R) is radius_edges, tagged with its radius
              (chain_tag stays None for it, so every ±1-chain caller passes it on
              to the generic kernels)
  references  forward64_radius (integer neighbour sums times the exact W_b/(2R))
              against exact_cases.forward64 on radius_edges (a float64 mean):
              equal exactly for R <= 2, to 1e-12 relative for R = 3, whose / 6
              is inexact in float64; the pinned oracle's float32 forward on
              those edges equals it exactly for R <= 2
  validity    every case is valid for f32 (exact_cases.Record.valid)
  sharpness   each mutant changes more than half of the faces: a forward that
              drops the ±R neighbours; one that takes i+R twice instead of i-R;
              and, restating the windowed kernel, 64-cell windows with halo L
              instead of L*R.  The last keeps its window's middle exact by
              construction (39 of a mutant window's 55 faces at L = 4, R = 3),
              so its fraction is taken over the faces the wrap has reached
              (radius_cases.halo_zone): all 7 faces at nx = 7, 24 of 100, 40 of
              128.  The same restatement with halo L*R is exact.  A fourth
              mutant leaves the last window out (nwin one short), measured over
              that window's faces.  At L = 0 no neighbour sum exists: those rows
              must equal the radius-1 forward instead.
  regimes     the regime rows (every row with a `why`): the constants and launch
              formulas of the table as csrc/ writes them, so that a moved
              threshold fails here until the table, and the sizes around it, move
              too; every figure of a `why` recomputed; every boundary (nwin
              changing, the second pass, the tightest window) with rows on both
              sides; the faces a later pass of the persistent loop owns nonzero
              in the expectation (its failure mode is "not written"); at R = 3
              the pinned oracle's forward in float64 at the 1e-12 gate
  order       the order recipe (radius_cases.order_sd / forward32_order): the
              recipe is what it says (one nonzero per row, zero biases, positive
              non-dyadic float32 features); a pairwise and a reversed neighbour
              sum each change at least 5 % of every case's fluxes and face
              fluxes; at R = 2 the pinned oracle's float32 forward gives the
              "fixed" order's bits on every edge
  ABI       hf_model_create_ex / hf_model_radius are declared, in the ctypes
              table and exported; radius 0 and 4 are HF_EINVAL, a radius > 1 in
              bf16 / f16x3 or on another width HF_EUNSUPPORTED, all before any
              device call
  Python      HybridSolver(graph_radius=...) validates; an ensemble of mixed
              radii raises the incompatibility error; compare_models groups by
              radius; the unrolled FluxGNN trainers refuse graph_radius > 1
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import exact_cases as X
import radius_cases as RC
from oracle import hybrid_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)


# ----------------------------------------------------------------------- edges
@pytest.mark.parametrize("nx,B", [(1, 1), (2, 3), (7, 2), (64, 5)])
def test_radius_one_is_the_reference_edge_list(nx, B):
    assert np.array_equal(RC.radius_edges(nx, B, 1), X.chain_edges(nx, B))


@pytest.mark.parametrize("nx,B,R", [(5, 1, 2), (7, 3, 3), (16, 5, 2), (64, 2, 3), (100, 3, 3)])
def test_package_edge_index_is_the_definition(nx, B, R):
    from hybridflux.graph_constructor import (build_chain_graph_batch, chain_edge_index, chain_tag, chain_tag_radius,
                                              shared_chain_edge_index)
    want = RC.radius_edges(nx, B, R)
    ei = chain_edge_index(nx, B, radius=R)
    assert ei.dtype == torch.long and np.array_equal(ei.numpy(), want)
    assert np.array_equal(want[:, :2 * nx], X.chain_edges(nx, 1))         # the first 2nx edges are the reference's
    assert len(set(map(tuple, want.T))) == want.shape[1]                  # nx >= 2R + 1: no edge repeats
    assert chain_tag(ei) is None and chain_tag_radius(ei) == (B, nx, R)
    one = chain_edge_index(nx, B)
    assert chain_tag(one) == (B, nx) and chain_tag_radius(one) == (B, nx, 1)
    sh = shared_chain_edge_index(nx, B, None, R)
    assert sh is shared_chain_edge_index(nx, B, None, R) and sh is not shared_chain_edge_index(nx, B)
    assert np.array_equal(sh.numpy(), want)
    _, eb = build_chain_graph_batch(np.zeros((B, 3, nx), np.float32), np.zeros(nx), radius=R)
    assert np.array_equal(eb.numpy(), want)
    ei[0, 0] += 0                                                         # an in-place edit drops the tag
    assert chain_tag_radius(ei) is None


def test_edge_index_refuses_bad_radii():
    from hybridflux.graph_constructor import chain_edge_index
    for nx, R in ((64, 0), (64, 4), (4, 2), (6, 3)):
        with pytest.raises(ValueError):
            chain_edge_index(nx, 1, radius=R)
    assert chain_edge_index(5, 1, radius=2).shape == (2, 20) and chain_edge_index(2, 1).shape == (2, 4)


# ------------------------------------------------------------------ references
@ALL
def test_forward64_radius_is_the_forward_on_the_edge_list(case):
    b = RC.find_case(case)
    # (the rows of a thousand ICs: the first 8, ICs being independent in either forward)
    nb = case.B if case.B * case.nx <= 8192 else 8
    ei = b.ei[:, :nb * 2 * case.R * case.nx]
    assert int(ei.max()) == nb * case.nx - 1
    want, _ = X.forward64(b.sd, b.nf[:nb * case.nx], nb, case.nx, edge_index=ei, record=False)
    want = want.reshape(nb, -1)
    assert b.flux_all.shape == (case.B, 2 * case.R * case.nx) and want.shape == b.flux_all[:nb].shape
    assert np.array_equal(b.flux_all, np.rint(b.flux_all))                # integers, for R = 3 too
    if case.R <= 2:
        assert np.array_equal(b.flux_all[:nb], want)
    else:
        assert np.allclose(b.flux_all[:nb], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", [c for c in RC.CASES if c.R <= 2], ids=lambda c: c.name)
def test_oracle_float32_forward_agrees(case):
    """(R <= 2 only: at R = 3 the oracle's float32 mean s / 6 rounds.)"""
    b = RC.find_case(case)
    with torch.no_grad():
        got = O.flux_gnn_forward(O.params_from(b.sd), torch.from_numpy(b.nf), torch.from_numpy(b.ei)).numpy()
    assert X.mismatch(got.reshape(case.B, -1), b.flux_all) is None


@ALL
def test_case_is_valid_for_f32(case):
    b = RC.find_case(case)
    assert b.rec.valid("f32") and b.rec.m <= 1, (b.rec.max_bound(), b.rec.m)
    assert np.array_equal(b.flux, b.flux_all[:, :2 * case.nx])
    assert np.array_equal(b.faces, 0.5 * (b.flux[:, :case.nx] + b.flux[:, case.nx:]))
    if case.zero_x:
        assert not np.any(b.sd["input_mlp.0.weight"][:, 3]) and not np.any(b.nf[:, 3])
    H = 128
    for l in range(case.layers):
        assert set(np.unique(np.abs(b.sd[f"update_mlps.{l}.0.weight"][:, H:]))) == {0.0, 2.0 * case.R}


# -------------------------------------------------------------------- sharpness
@ALL
def test_case_is_sharp(case):
    b = RC.find_case(case)
    frac = RC.mutants(case, b.sd, b.nf, b.flux_all)
    want = {"drop", "twice"} if case.layers else set()
    if not case.fused:
        want |= {"halo", "last"} if case.layers else {"last"}
    assert set(frac) == want == RC.applicable(case)
    for k, v in frac.items():
        assert v > 0.5, (k, v)
    if case.layers == 0:   # no neighbour sum for a mutant to change: the radius-1 forward, bit for bit
        assert np.array_equal(X.forward64(b.sd, b.nf, case.B, case.nx, record=False)[0], b.flux)
    assert b.seed == 0 and np.mean(b.flux != 0) >= 0.9             # accept()'s other condition; no seed had to move


@pytest.mark.parametrize("case", RC.cases("flux", fused=False), ids=lambda c: c.name)
def test_windowed_restatement(case):
    """Windows with halo L*R reproduce the forward exactly; the faces a halo of L
    would keep wrongly are where the table says; without the last window exactly
    the faces of last_window change, each of them to zero."""
    b = RC.find_case(case)
    halo = case.layers * case.R
    assert np.array_equal(RC.windowed64(b.sd, b.nf, case.B, case.nx, case.R, halo), b.flux)
    zone = RC.halo_zone(case)
    if case.why is None:
        assert int(zone.sum()) == {7: 7, 100: 24, 128: 40}[case.nx]
        assert 64 - 2 * case.layers * case.R - 1 == 39
    # the zone restated: a face is in it when its position in a window of halo L lies within L*R of either end
    Fm = 63 - 2 * case.layers
    pos = case.layers + np.arange(case.nx) % Fm
    assert np.array_equal(zone, (pos < halo) | (pos > 62 - halo))
    assert bool(zone.any()) == (case.layers >= 1)
    short = RC.windowed64(b.sd, b.nf, case.B, case.nx, case.R, halo, drop_last=True)
    last = RC.last_window(case)
    r = case.regime()
    assert int(last.sum()) == r["keeps"] == case.nx - (r["nwin"] - 1) * r["F"] >= 1
    both = np.concatenate([last, last])
    assert not short[:, both].any() and np.array_equal(short[:, ~both], b.flux[:, ~both])


# --------------------------------------------------- the table against the sources
NEW = [c for c in RC.CASES if c.why is not None]
FIGURE = re.compile(r"\b(halo|F|nwin|keeps|items|groups|passes|pass2|live) = (\d+)")


def src(name):
    with open(os.path.join(ROOT, "gnn-plasma-flux_amd", "csrc", name)) as fh:
        return fh.read()


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_constants_match_the_sources():
    """A moved constant or launch formula fails here until the table, and the sizes around it, move too."""
    hi, cc, f32, capi = src("hf_internal.h"), src("chain_common.h"), src("chain_f32.hip"), src("capi.cpp")
    assert int(one(r"constexpr int kWinCells = (\d+);", hi)) == RC.WIN_CELLS
    assert int(one(r"constexpr int kMaxChainLayers = (\d+);", hi)) == RC.MAX_LAYERS
    a, b = one(r"int win_faces_of\(int layers, int cells = kWinCells\) \{ return cells - (\d+) \* layers - (\d+); \}", hi)
    assert (int(a), int(b)) == (2, 1) and RC.win_faces(5) == RC.WIN_CELLS - 2 * 5 - 1 == X.win_faces(5)
    assert int(one(r"constexpr int kWaves = (\d+);", cc)) == RC.NW
    core = f32[f32.index("struct CoreF32T"):f32.index("using CoreF32 =")]
    assert one(r"static constexpr int kNW = (\w+);", core) == "kWaves"
    assert int(one(r"static constexpr int kWGPerCU = (\d+);", core)) == RC.WG_PER_CU
    assert int(one(r"static constexpr int kWinMT = (\d+);", core)) == RC.WIN_MT and 16 * RC.WIN_MT == RC.WIN_CELLS
    assert one(r"static constexpr int kRadius = (\w+);", core) == "RAD"
    assert one(r"static_assert\(RAD >= 1 && RAD <= (\d+),", core) == str(RC.MAX_RADIUS)
    assert int(one(r"constexpr int kDefaultLanes = (\d+);", capi)) == RC.DEFAULT_LANES
    assert one(r"constexpr int64_t kLaneMinCells = ([^;]+);", capi) == "1 << 20" and RC.LANE_MIN_CELLS == 1 << 20
    assert one(r"while \(lanes > 1 && \(int64_t\)B \* nx < lanes \* kLaneMinCells\) --lanes;", capi)
    assert one(r"for \(int i = 0; i <= lanes; \+\+i\) cut\[i\] = \(int64_t\)B \* i / lanes;", capi)
    # the window geometry and the persistent loop of chain_flux_kernel, the launchers' counts
    k = cc[cc.index("void chain_flux_kernel"):cc.index("void chain_train_fwd_kernel")]
    assert one(r"const int halo = W\.layers \* core_radius<Core>::value, win_faces = win_faces_of\(halo, 16 \* MT\);", k)
    assert one(r"const int64_t groups = \(items \+ Core::kNW - 1\) / Core::kNW;", k)
    assert one(r"for \(int64_t grp = blockIdx\.x; grp < groups; grp \+= gridDim\.x\)", k)
    assert one(r"if \(grp \+ gridDim\.x < groups\) load_feat\(grp \+ gridDim\.x, pre\);", k)
    assert one(r"int cidx = \(\(EXACT \? 0 : w \* win_faces - halo\) \+ cell_of<MT>\(mt, j\)\) % nx;", k)
    assert one(r"face = w \* win_faces \+ \(wc - halo\);", k)
    assert one(r"ok = wc >= halo && wc < halo \+ win_faces && face < nx;", k)
    fl = cc[cc.index("hipError_t flux_launch"):cc.index("hipError_t rollout_launch")]
    assert one(r"const int64_t res = \(int64_t\)resident_groups\(\) \* Core::kWGPerCU;", fl)
    assert one(r"const int64_t blocks = groups < res \? groups : res;", fl)
    assert one(r"const int faces = win_faces_of\(w\.layers \* core_radius<Core>::value, 16 \* WMT\);", fl)
    assert one(r"const int nwin = \(nx \+ faces - 1\) / faces;", fl)
    assert one(r"flux_launch<Core, WMT, false>\(w, nf, state, ld_state, x, nx, nwin, \(int64_t\)B \* nwin, fe, ff, s\);", fl)
    assert [int(v) for v in re.findall(r"case (\d+): return flux_launch<Core, \d, true>", fl)] == list(RC.FUSED_NX)
    assert one(r"if \(faces < 1\) return hipErrorInvalidValue;  // \(L <= 8, R <= 3 leave (\d+)\)", fl) == \
        str(RC.win_faces(RC.MAX_LAYERS * RC.MAX_RADIUS)) == "15"


@pytest.mark.parametrize("case", NEW, ids=lambda c: c.name)
def test_the_figures_of_a_row(case):
    """Every figure a `why` states, recomputed; every row states its launch figures."""
    figs = FIGURE.findall(case.why)
    got = {k: int(v) for k, v in figs}
    assert len(got) == len(figs), "a figure stated twice"
    r = case.regime()
    need = {"items", "groups", "passes", "live"} | (set() if case.fused else {"halo", "F", "nwin", "keeps"})
    assert need <= set(got), sorted(need - set(got))
    assert ("pass2" in got) == (r["passes"] > 1)
    for k, v in got.items():
        assert r[k] == v, (k, v, r[k])
    assert case.fused == (case.nx in RC.FUSED_NX) and case.layers <= RC.MAX_LAYERS
    assert ("hi = 2" in case.why) == (case.hi == 2) and case.hi in (2, 4)
    if not case.fused:   # the formulas themselves, written out once more
        assert r["F"] == 63 - 2 * case.layers * case.R and r["nwin"] == -(-case.nx // r["F"])
        assert (r["nwin"] - 1) * r["F"] < case.nx <= r["nwin"] * r["F"]
    assert r["groups"] == -(-r["items"] // 4) and 1 <= r["live"] <= 4


def test_every_regime_is_reached():
    flux = RC.cases("flux")
    regs = {c.name: c.regime() for c in flux}
    # depths: fused L in {0, 1, 2, 4, 8}; windowed 0, 1, 2, 3, 4, 8; the R = 2 windowed kernel has exact cases
    assert {c.layers for c in flux if c.fused} == {0, 1, 2, 4, 8}
    assert {c.layers for c in flux if not c.fused} == {0, 1, 2, 3, 4, 8}
    assert {c.layers for c in flux if not c.fused and c.R == 2} == {1, 2, 3, 4, 8}
    assert {(c.R, c.layers) for c in flux if c.fused and c.layers == 8} == {(2, 8), (3, 8)}
    # a window-count boundary has rows on both sides: nx = k F and nx = k F + 1, for k = 1 and k = 2
    sides = {}
    for c in flux:
        r = regs[c.name]
        if not c.fused and c.nx % r["F"] in (0, 1):
            sides.setdefault((c.R, c.layers), set()).add((c.nx // r["F"], c.nx % r["F"], r["nwin"]))
    assert sides[3, 4] >= {(1, 0, 1), (1, 1, 2), (2, 1, 3)} and sides[2, 4] >= {(1, 0, 1), (2, 0, 2), (2, 1, 3)}
    assert sides[3, 8] >= {(1, 0, 1), (2, 1, 3)} and sides[2, 8] >= {(2, 1, 3)}
    for key in ((3, 4), (2, 4), (3, 8)):
        assert {rem for _, rem, _ in sides[key]} == {0, 1}, key
    assert any(r["keeps"] == 1 for r in regs.values()) and any(r["keeps"] == r["F"] for r in regs.values())
    # the tightest window is reached, and so are wider ones
    tight = RC.win_faces(RC.MAX_LAYERS * RC.MAX_RADIUS)
    Fs = {r["F"] for r in regs.values() if r["F"]}
    assert tight == 15 == min(Fs) and max(Fs) == 63 and len(Fs) >= 8
    # chains shorter than the window, the smallest legal ones, and long ones
    win = [c for c in flux if not c.fused]
    assert {c.nx for c in win if c.nx < RC.WIN_CELLS} >= {5, 7, 15, 17, 31, 39, 40, 47, 63}
    assert any(c.nx == 2 * c.R + 1 for c in win if c.R == 2) and any(c.nx == 2 * c.R + 1 for c in win if c.R == 3)
    assert any(c.nx < RC.WIN_CELLS and regs[c.name]["nwin"] == 2 for c in win)
    assert max(r["nwin"] for r in regs.values()) == 27
    # the persistent loop: one pass and two, in the EXACT form and in the windowed one, MT = 1 and MT = 4
    for fused in (True, False):
        assert {regs[c.name]["passes"] for c in flux if c.fused == fused} == {1, 2}, fused
    two = [c for c in flux if regs[c.name]["passes"] == 2]
    assert {c.nx for c in two} == {16, 64, 100} and {c.R for c in two} == {2, 3}
    assert all(0 < regs[c.name]["pass2"] < RC.CUS and regs[c.name]["live"] < RC.NW for c in two)  # a ragged later pass
    # per-step rollouts at unfused nx
    roll = RC.cases("rollout", fused=False)
    assert {(c.nx, c.R, c.layers) for c in roll} == {(100, 2, 1), (100, 2, 4), (100, 3, 4), (1024, 3, 4)}
    assert all(isinstance(c.why, str) and len(c.why) > 40 for c in NEW) and len(NEW) == 34


def test_fewer_cus_only_add_passes():
    for c in RC.CASES:
        for cus in (64, 128, 192, 240, 256, 304):
            if cus <= RC.CUS:
                assert c.regime(cus)["passes"] >= c.regime()["passes"]
    assert RC.regime(64, 1024, 4, 2)["passes"] == 1 and RC.regime(64, 1025, 4, 2)["passes"] == 2
    assert RC.lanes(1024, 3075) == (3, [0, 1025, 2050, 3075]) and RC.lanes(1024, 3071)[0] == 2


@pytest.mark.parametrize("case", [c for c in NEW if c.regime()["passes"] > 1], ids=lambda c: c.name)
def test_later_pass_is_seen(case):
    """The kernel's failure mode in a later pass is "not written": the faces its
    items own must be nonzero in the expectation, so that a buffer left as it
    was (zeros, or the NaN the GPU test fills in) differs."""
    b = RC.find_case(case)
    r = case.regime()
    mask = RC.later_pass_faces(case)
    n = r["items"] - r["first_later_item"]
    assert r["first_later_item"] == 1024 and n == (r["pass2"] - 1) * 4 + r["live"]
    if case.fused:
        assert int(mask.sum()) == n * case.nx and mask[1024:].all() and not mask[:1024].any()
    else:
        first = divmod(r["first_later_item"], r["nwin"])
        assert not mask[:first[0]].any() and mask[first[0] + 1:].all()
        assert int(mask[first[0]].sum()) == case.nx - first[1] * r["F"]
    nz = (b.flux[:, :case.nx] != 0) | (b.flux[:, case.nx:] != 0)
    assert nz[mask].mean() > 0.9 and np.mean(b.flux != 0) > 0.9
    dropped = b.flux.copy()
    dropped[np.concatenate([mask, mask], axis=1)] = 0
    assert RC.changed_faces(dropped, b.flux, case.nx) == nz[mask].sum() / mask.size > 0


@pytest.mark.parametrize("case", [c for c in NEW if c.R == 3], ids=lambda c: c.name)
def test_oracle_float64_forward_agrees_at_radius_3(case):
    """The pinned oracle's forward on radius_edges with float64 parameters, at
    the gate of test_forward64_radius_is_the_forward_on_the_edge_list (its mean
    s / 6 is inexact in float64 too)."""
    b = RC.find_case(case)
    p = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in b.sd.items()}
    with torch.no_grad():
        got = O.flux_gnn_forward(p, torch.from_numpy(b.nf.astype(np.float64)), torch.from_numpy(b.ei)).numpy()
    assert got.dtype == np.float64 and np.allclose(got.reshape(case.B, -1), b.flux_all, rtol=1e-12, atol=0)


# ------------------------------------------------------------- the order recipe
ORDER = pytest.mark.parametrize("case", RC.ORDER_CASES, ids=lambda c: c.name)


@ORDER
def test_order_recipe_is_what_it_says(case):
    b = RC.find_order_case(case)
    sd, H, R = b.sd, 128, case.R
    assert X.n_layers(sd) == case.layers and b.nf.dtype == np.float32 and b.nf.shape == (case.B * case.nx, 4)
    assert b.nf.min() >= np.float32(0.1) and b.nf.max() <= 2 and X.dyadic_bits(b.nf[:8]) > 12   # not dyadic
    for k, v in sd.items():
        assert v.dtype == np.float32
        if k.endswith("bias"):
            assert not v.any(), k
    halves = [sd["input_mlp.0.weight"], sd["edge_mlp.0.weight"][:, :H], sd["edge_mlp.0.weight"][:, H:],
              sd["edge_mlp.2.weight"]]
    for l in range(case.layers):
        W = sd[f"update_mlps.{l}.0.weight"]
        halves += [W[:, :H], W[:, H:] / np.float32(2 * R)]
        assert set(np.unique(W[:, H:])) == {0.0, 2.0 * R}
    for W in halves:
        assert np.all((W != 0).sum(1) == 1) and set(np.unique(W)) == {0.0, 1.0}
    for W in halves[1:3] + halves[4:]:
        assert np.all((W != 0).sum(0) == 1)                       # a permutation
    assert sd["edge_mlp.2.weight"][0, case.k0] == 1
    assert not np.array_equal(halves[1], halves[2])


@ORDER
def test_order_cases_are_sharp(case):
    """Each wrong order changes at least 5 % of the observed fluxes (the first 2nx
    per IC), and of the face fluxes; the seed is 0, chosen on this reference alone."""
    b = RC.find_order_case(case)
    assert b.seed == 0 and set(b.changed) == {"pairwise", "reversed"}
    a = (b.sd, b.nf, case.B, case.nx, case.R)
    fixed = RC.forward32_order(*a, "fixed")
    assert fixed.dtype == np.float32 and fixed.shape == (case.B, 2 * case.nx) and np.array_equal(fixed, b.flux)
    assert np.array_equal(RC.forward32_order(*a, "fixed", all_edges=True)[:, :2 * case.nx], fixed)
    half = np.float32(0.5)
    for order in ("pairwise", "reversed"):
        other = RC.forward32_order(*a, order)
        assert np.mean(other != fixed) == b.changed[order] >= RC.ORDER_MIN_CHANGED == 0.05, order
        assert np.mean(half * (other[:, :case.nx] + other[:, case.nx:]) !=
                       half * (fixed[:, :case.nx] + fixed[:, case.nx:])) >= RC.ORDER_MIN_CHANGED, order
        # a change of order is a rounding matter: the same forward to float32 accuracy
        assert np.allclose(other, fixed, rtol=1e-5, atol=0)
    assert np.isfinite(fixed).all() and fixed.min() > 0           # ReLU never clips


@pytest.mark.parametrize("case", [c for c in RC.ORDER_CASES if c.R == 2], ids=lambda c: c.name)
def test_order_reference_is_the_oracle_at_radius_2(case):
    """At degree 4 the oracle's float32 mean (a sequential index_add_ over the
    edge list, / 4, times W_b = 4) is the folded form bit for bit: the pinned
    oracle itself gives forward32_order's "fixed" bits on every edge, and not
    those of the other orders."""
    b = RC.find_order_case(case)
    ei = torch.from_numpy(RC.radius_edges(case.nx, case.B, case.R))
    with torch.no_grad():
        got = O.flux_gnn_forward(O.params_from(b.sd), torch.from_numpy(b.nf), ei).numpy().reshape(case.B, -1)
    a = (b.sd, b.nf, case.B, case.nx, case.R)
    assert got.dtype == np.float32 and np.array_equal(got, RC.forward32_order(*a, "fixed", all_edges=True))
    for order in ("pairwise", "reversed"):
        assert np.mean(got != RC.forward32_order(*a, order, all_edges=True)) >= RC.ORDER_MIN_CHANGED


def test_nb_sum32_orders():
    h = np.array([1e8, 1.0, -1e8, 3.0, 0.5, 7.0, 2.0], np.float32).reshape(1, 7, 1)
    p = lambda r: np.roll(h, -r, axis=1)
    m = lambda r: np.roll(h, r, axis=1)
    assert np.array_equal(RC.nb_sum32(h, 2, "fixed"), ((p(1) + m(1)) + p(2)) + m(2))
    assert np.array_equal(RC.nb_sum32(h, 3, "fixed"), ((((p(1) + m(1)) + p(2)) + m(2)) + p(3)) + m(3))
    assert np.array_equal(RC.nb_sum32(h, 3, "pairwise"), ((p(1) + m(1)) + (p(2) + m(2))) + (p(3) + m(3)))
    assert np.array_equal(RC.nb_sum32(h, 3, "reversed"), ((((m(3) + p(3)) + m(2)) + p(2)) + m(1)) + p(1))
    assert not np.array_equal(RC.nb_sum32(h, 3, "fixed"), RC.nb_sum32(h, 3, "pairwise"))
    ints = np.arange(14, dtype=np.float32).reshape(1, 7, 2)
    for R in (2, 3):   # integers: every order the same bits, and the integer reference's
        for order in RC.ORDERS:
            assert np.array_equal(RC.nb_sum32(ints, R, order), RC.nb_sum(ints.astype(np.float64), R))


# -------------------------------------------------------------------------- ABI
def test_symbols_declared_and_exported():
    from hybridflux import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hybridflux.h")).read()
    for n, nargs in (("hf_model_create_ex", 7), ("hf_model_radius", 1), ("hf_graph_flux_radius", 8)):
        assert n in _lib.SIGNATURES and hasattr(L, n), n
        m = re.search(rf"\bint\s+{n}\(([^;]*)\);", header)
        assert m, f"{n} is not declared in include/hybridflux.h"
        res, args = _lib.SIGNATURES[n]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")) == nargs, n
    assert "Replaces: nothing the reference" in header and "src/hybrid_solver.py:32" in header
    mk = open(os.path.join(ROOT, "gnn-plasma-flux_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bchain_f32_radius\.hip\b", mk, re.M)
    assert L.hf_model_radius(None) == 0
    assert L.hf_graph_flux_radius(None, None, 1, 7, None, None, None, None) == _lib.HF_EINVAL


def test_create_ex_validates_before_any_device_call():
    from hybridflux import _lib
    L = _lib.lib()
    n = L.hf_model_param_count(4, 128, 1)
    p = (ctypes.c_float * n)()
    out = ctypes.c_void_p(8)
    for radius in (0, 4, -1, 100):
        assert L.hf_model_create_ex(p, 4, 128, 1, _lib.HF_WDTYPE_F32, radius, out) == _lib.HF_EINVAL, radius
        assert "radius" in L.hf_last_error().decode() and out.value is None
    for wd in (_lib.HF_WDTYPE_BF16, _lib.HF_WDTYPE_F16X3):
        assert L.hf_model_create_ex(p, 4, 128, 1, wd, 2, out) == _lib.HF_EUNSUPPORTED
        assert "float32" in L.hf_last_error().decode()
    small = (ctypes.c_float * L.hf_model_param_count(4, 64, 1))()
    assert L.hf_model_create_ex(small, 4, 64, 1, _lib.HF_WDTYPE_F32, 3, out) == _lib.HF_EUNSUPPORTED
    assert L.hf_model_create_ex(None, 4, 128, 1, _lib.HF_WDTYPE_F32, 2, out) == _lib.HF_EINVAL
    assert L.hf_model_create_ex(p, 4, 128, 1, _lib.HF_WDTYPE_F32, 2, None) == _lib.HF_EINVAL
    assert L.hf_model_create_ex(p, 4, 128, 1, 99, 2, out) == _lib.HF_EINVAL


# ----------------------------------------------------------------------- Python
def _solver(seed, **kw):
    import hybridflux
    sd = X.make_sd(4, seed)
    kw.setdefault("device", "cpu")
    return hybridflux.HybridSolver({k: torch.from_numpy(v) for k, v in sd.items()}, 1, **kw)


def test_solver_option_and_ensembles():
    import hybridflux
    from hybridflux import evaluation
    a = _solver(1)
    assert a.graph_radius == 1 and a.radius == 1
    s = _solver(2, graph_radius=3)
    assert s.graph_radius == 3 and s.radius == 1                          # the label stays a label
    for kw in (dict(graph_radius=0), dict(graph_radius=4), dict(graph_radius=2, precision="bf16"),
               dict(graph_radius=2, precision="f16x3"), dict(graph_radius=3, nx=6)):
        with pytest.raises(ValueError):
            _solver(3, **kw)
    assert "graph_radius" in hybridflux.HybridEnsemble.SIGNATURE
    with pytest.raises(ValueError, match="solver 1 has graph_radius = 2"):
        hybridflux.HybridEnsemble([_solver(1), _solver(2, graph_radius=2)])
    hybridflux.HybridEnsemble([_solver(1, graph_radius=2), _solver(2, graph_radius=2)])
    models = {"r1": _solver(1), "r2a": _solver(2, graph_radius=2), "r2b": _solver(3, graph_radius=2),
              "r3": _solver(4, graph_radius=3)}
    assert evaluation.ensemble_groups(models) == [["r2a", "r2b"]]
    sweep = {f"c{c}_r{r}": _solver(10 * c + r, graph_radius=r) for c in range(4) for r in (1, 2, 3)}
    assert sorted(map(len, evaluation.ensemble_groups(sweep))) == [4, 4, 4]     # 12 models, three launches


def test_unrolled_trainers_refuse_a_radius():
    from hybridflux import training
    for fn, args in ((training.unrolled_loss, (None, None, None, None)),
                     (training.unrolled_step, (None, None, None, None, None)),
                     (training.train_unrolled, (None, None, 5e-3, 0.1, 1e-3))):
        with pytest.raises(ValueError, match="graph_radius"):
            fn(*args, graph_radius=2)
    with pytest.raises(ValueError, match="graph_radius"):
        training.train_model(None, None, None, None, 5e-3, 0.1, 1e-3, "baseline", 2, graph_radius=4)
