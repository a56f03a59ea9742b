"""tests/row_regimes.py against the sources and against itself.  No GPU.

  constants ......... the table's constants equal kBM, kBN, kKC (tgemm.h and graph.hip),
      the split sizes and caps of pure_wg_splits / pinn_wg_splits, split_rows' minimum
      and kMaxSplits, scan_kernel's chunk and tg_block's group as csrc/ writes them: a
      moved threshold fails here until the table, and the sizes around it, move too
  tg_block .......... the restated decode is a bijection on (bx, by, bz) for every grid
      the cases launch and for all T in 1..64 with gridDim.x in 1..5; the GPU tests
      are what show that the kernel has this property
  numbers ........... every figure in a case's `why` recomputed from the restatements
  straddling ........ every boundary has a named case on each side
  mutants ........... a float64 restatement of the split-K weight gradient reproduces
      autograd, and each of its mutants (a split left out, the ragged rows left out,
      a row tile read twice, an output tile unwritten) moves a gradient tensor of every
      PureGNN and PINN case by more than 10x the gradient gate
  reference ......... float32 torch-CPU autograd of the oracle stays within a quarter
      of the gate of its float64 evaluation on every case
"""
import os
import re

import numpy as np
import pytest
import torch

import row_regimes as R
from conftest import PKG_DIR
from oracle import hybrid_oracle as O

CSRC = os.path.join(PKG_DIR, "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_constants_match_the_sources():
    tg, pure, pinn, graph = src("tgemm.h"), src("pure_train.hip"), src("pinn_train.hip"), src("graph.hip")
    # kKC sits in a comma list in both files
    bm, bn, kc = one(r"constexpr\s+int\s+kBM\s*=\s*(\d+)\s*,\s*kBN\s*=\s*(\d+)\s*,\s*kKC\s*=\s*(\d+)\s*;", tg)
    assert (int(bm), int(bn), int(kc)) == (R.TILE_M, R.TILE_N, R.STAGE)
    assert int(one(r"constexpr\s+int\s+kT\s*=\s*\d+\s*,\s*kKC\s*=\s*(\d+)\s*,", graph)) == R.STAGE
    cap, rows = one(r"pure_wg_splits\(int64_t N\)\s*\{\s*return \(int\)std::min<int64_t>\((\d+), "
                    r"std::max<int64_t>\(1, N / (\d+)\)\);", pure)
    assert (int(cap), int(rows)) == (R.PURE_SPLIT_CAP, R.PURE_SPLIT_ROWS)
    cap, m1, rows = one(r"pinn_wg_splits\(int64_t B\)\s*\{\s*return \(int\)std::min<int64_t>\((\d+), "
                        r"std::max<int64_t>\(1, \(B \+ (\d+)\) / (\d+)\)\);", pinn)
    assert (int(cap), int(m1) + 1, int(rows)) == (R.PINN_SPLIT_CAP, R.PINN_SPLIT_ROWS, R.PINN_SPLIT_ROWS)
    assert int(one(r"constexpr\s+int64_t\s+kMaxSplits\s*=\s*(\d+)\s*;", graph)) == R.GENERIC_MAX_SPLITS
    lo, hi = one(r"R = R < (\d+) \? (\d+) : R;", graph)
    assert int(lo) == int(hi) == R.GENERIC_MIN_ROWS
    assert one(r"return \(R \+ kKC - 1\) / kKC \* kKC;", graph)
    scan = graph[graph.index("void scan_kernel"):graph.index("void fill_kernel")]
    assert {int(v) for v in re.findall(r"\b(\d{3,})\b", scan)} == {R.SCAN_CHUNK, R.SCAN_CHUNK - 1}
    assert one(r"dim3\(1\), dim3\((\d+)\), 0, s, deg, N, off, cur\)", graph) == str(R.SCAN_CHUNK)
    g = R.REMAP_GROUP
    assert one(r"if \(L < T - T % (\d+)\) L = 2 \* \(8 \* \(L >> 4\) \+ \(L & 7\)\) \+ \(\(L >> 3\) & 1\);", tg) == str(g)
    # tgemm, tgemm_batch and tgemm_splits round the rows per split the same way
    assert len(re.findall(r"rsplit = \(rsplit \+ kKC - 1\) / kKC \* kKC;", tg)) == 3
    assert len(re.findall(r"int64_t rsplit = \(R \+ splits - 1\) / splits;", tg)) == 3
    # the exact kernels' condition, in tgemm and in tgemm_batch
    assert len(re.findall(r"R > 0 && I % kBM == 0 && J % kBN == 0 && R % kKC == 0", tg)) == 2


def all_launches():
    out = []
    for c in R.PURE_CHAIN:
        out += R.pure_forward_launches(*c) + R.pure_backward_launches(*c)
    for c in R.PINN_GEMM:
        out += R.pinn_forward_launches(*c) + R.pinn_backward_launches(*c)
    return out


def test_tg_block_decode_is_a_bijection():
    grids = {g["grid"] for g in all_launches()}
    for gx in range(1, 6):
        for T in range(1, 65):
            if T % gx == 0:
                grids |= {(gx, 1, T // gx)}
                if T % (2 * gx) == 0:
                    grids |= {(gx, 2, T // (2 * gx))}
    for T in range(1, 65):
        assert sorted(R.tg_decode(L, T) for L in range(T)) == list(range(T)), T
    for grid in sorted(grids):
        gx, gy, gz = grid
        tiles = {R.tg_block(bx, by, bz, grid) for bz in range(gz) for by in range(gy) for bx in range(gx)}
        assert tiles == {(bx, by, bz) for bz in range(gz) for by in range(gy) for bx in range(gx)}, grid
    # and it is the pairing it is meant to be: workgroups b and b + 8 get consecutive tiles
    assert [R.tg_decode(L, 32) for L in (0, 8, 1, 9, 16, 24)] == [0, 1, 2, 3, 16, 17]
    assert [R.tg_decode(L, 17) for L in (15, 16)] == [15, 16] and R.tg_decode(8, 15) == 8


def blocks(g):
    return g["grid"][0] * g["grid"][1] * g["grid"][2]


def by_name(launches):
    return {g["name"]: g for g in launches}


def test_the_numbers_of_the_pure_cases():
    c = (64, 64, 2, 257)
    f, b = by_name(R.pure_forward_launches(*c)), by_name(R.pure_backward_launches(*c))
    N = 257 * 64
    assert N == 16448 and R.pure_wg_splits(N) == 64 == R.PURE_SPLIT_CAP
    assert (b["head_wgrad"]["rsplit"], b["head_wgrad"]["S"]) == (288, 58)
    assert R.split_lengths(N, 288)[-1] == 32 and sorted(set(R.stage_counts(N, 288))) == [1, 9]
    assert blocks(f["msg0"]) == 129 and 129 % R.REMAP_GROUP == 1 and N % R.TILE_M == 64
    assert blocks(b["layers_wgrad"]) == 116 and 116 % R.REMAP_GROUP == 4
    assert not R.ex_ok(b["layers_wgrad"]["I"], b["layers_wgrad"]["J"], N)
    c = (128, 64, 2, 256)
    f, b = by_name(R.pure_forward_launches(*c)), by_name(R.pure_backward_launches(*c))
    N = 16384
    assert (b["head_wgrad"]["rsplit"], b["head_wgrad"]["S"]) == (256, 64) and set(R.stage_counts(N, 256)) == {8}
    assert R.ex_ok(128, 128, N) and R.ex_ok(256, 128, N)
    assert (blocks(f["msg0"]), blocks(b["head_wgrad"]), blocks(b["layers_wgrad"])) == (256, 64, 256)
    c = (128, 16, 1, 1023)
    b = by_name(R.pure_backward_launches(*c))
    N = 16368
    assert N // R.PURE_SPLIT_ROWS == 63 == R.pure_wg_splits(N) and b["head_wgrad"]["S"] == 57
    assert R.split_lengths(N, b["head_wgrad"]["rsplit"])[-1] == 240 and N % R.STAGE == 16 and N % R.TILE_M == 112
    assert R.last_stage_rows(N, b["head_wgrad"]["rsplit"]) == 16 and not R.ex_ok(128, 128, N)
    assert [blocks(R.pure_forward_launches(64, 64, 1, B)[0]) for B in (30, 32, 34)] == [15, 16, 17]
    g = R.pure_forward_launches(128, 64, 1, 34)[0]
    assert g["grid"] == (17, 2, 1) and 34 % R.REMAP_GROUP == 2 and R.ex_ok(128, 128, 34 * 64)
    assert [by_name(R.pure_backward_launches(64, 64, 2, B))["head_wgrad"]["S"] for B in (7, 8)] == [1, 2]
    for c in R.PURE_CHAIN:
        assert R.pure_chain_path(c[0], c[1], c[1] * c[3]), c
    for c in R.PURE_GENERIC:
        assert not R.pure_chain_path(c[0], c[1], c[1] * c[3]), c


def test_the_numbers_of_the_pinn_and_generic_cases():
    f, b = by_name(R.pinn_forward_launches(192, 256, 4, 2000)), by_name(R.pinn_backward_launches(192, 256, 4, 2000))
    assert (b["wgrad0"]["rsplit"], b["wgrad0"]["S"]) == (128, 16) and R.split_lengths(2000, 128)[-1] == 80
    assert R.last_stage_rows(2000, 128) == 16 and blocks(f["fwd0"]) == blocks(f["fwd3"]) == 32
    assert blocks(b["hidden_wgrad"]) == 128 and not R.ex_ok(256, 256, 2000)
    b = by_name(R.pinn_backward_launches(192, 256, 4, 2048))
    assert R.ex_ok(b["hidden_wgrad"]["I"], b["hidden_wgrad"]["J"], 2048) and not R.ex_ok(192, 256, 2048)
    b = by_name(R.pinn_backward_launches(192, 256, 3, 8192))
    assert b["wgrad0"]["S"] == 64 == R.pinn_wg_splits(8192) == R.cdiv(8192, R.PINN_SPLIT_ROWS)
    b = by_name(R.pinn_backward_launches(192, 256, 3, 8193))
    assert R.pinn_wg_splits(8193) == 64 < R.cdiv(8193, R.PINN_SPLIT_ROWS)
    assert (b["wgrad0"]["rsplit"], b["wgrad0"]["S"]) == (160, 52) and R.split_lengths(8193, 160)[-1] == 33
    assert R.last_stage_rows(8193, 160) == 1
    for c in R.PINN_GEMM:
        assert R.pinn_gemm_path(c[0], c[1], c[3]), c
    for c in R.PINN_GENERIC:
        assert not R.pinn_gemm_path(c[0], c[1], c[3]), c
    gen = lambda M: (R.split_rows(M), R.cdiv(M, R.split_rows(M)))  # noqa: E731
    assert gen(682 * 48) == (256, 128) and 682 * 48 == 32736
    assert gen(700 * 48) == (288, 117) and 700 * 48 == 33600
    assert gen(40000) == (320, 125)
    assert gen(R.FLUX_GRAPH["E"]) == (320, 125) and R.cdiv(R.FLUX_GRAPH["N"], R.SCAN_CHUNK) == 3


def test_every_boundary_is_straddled():
    fw = [g for c in R.PURE_CHAIN for g in R.pure_forward_launches(*c)]
    T = {blocks(g) for g in fw}
    g16 = R.REMAP_GROUP
    # the remap: below, at and just above one group; a tail; gridDim.x odd with two column tiles
    assert {g16 - 1, g16, g16 + 1} <= T
    assert any(t > g16 and t % g16 for t in T) and any(t > g16 and t % g16 == 0 for t in T)
    assert any(g["grid"][0] % 2 == 1 and g["grid"][1] == 2 and blocks(g) > g16 for g in fw)
    # every epilogue and view used only by these models runs on a remapped grid (T >= 16) in some case
    for launches, names in ((fw, {"msg0", "out0"}),
                            ([g for c in R.PURE_CHAIN for g in R.pure_backward_launches(*c)],
                             {"head_wgrad", "head_dgrad", "dgrad0", "layers_wgrad"}),
                            ([g for c in R.PINN_GEMM for g in R.pinn_forward_launches(*c)], {"fwd0", "fwd1", "fwd3"}),
                            ([g for c in R.PINN_GEMM for g in R.pinn_backward_launches(*c)],
                             {"dgrad1", "dstate", "wgrad0", "wgrad2", "wgrad3", "hidden_wgrad"})):
        assert names <= {g["name"] for g in launches if blocks(g) >= g16}, names
    # the splits
    for cases, back, want, cap, name in ((R.PURE_CHAIN, R.pure_backward_launches, R.pure_wg_splits, R.PURE_SPLIT_CAP,
                                          "head_wgrad"),
                                         (R.PINN_GEMM, R.pinn_backward_launches, R.pinn_wg_splits, R.PINN_SPLIT_CAP,
                                          "wgrad0")):
        seen = [(want(g["R"]), g["S"], g["R"], g["rsplit"]) for c in cases for g in back(*c) if g["name"] == name]
        req = {s[0] for s in seen}
        assert cap in req and any(r < cap for r in req)                      # below and at the cap
        assert any(s[0] == cap and s[1] < cap for s in seen)                 # above: S below the request
        assert any(s[0] == cap and s[1] == cap for s in seen)                # exactly the cap
        parities = {n % 2 for s in seen for n in R.stage_counts(s[2], s[3])}
        assert parities == {0, 1}
        assert any(len(set(R.stage_counts(s[2], s[3]))) > 1 for s in seen)   # a shorter last split
    S = {by_name(R.pure_backward_launches(*c))["head_wgrad"]["S"] for c in R.PURE_CHAIN}
    assert {1, 2} <= S
    last = {R.last_stage_rows(g["R"], g["rsplit"]) for c in R.PURE_CHAIN for g in R.pure_backward_launches(*c)
            if g.get("wgrad")}
    last |= {R.last_stage_rows(g["R"], g["rsplit"]) for c in R.PINN_GEMM for g in R.pinn_backward_launches(*c)
             if g.get("wgrad")}
    assert {1, 16, 32} <= last
    # EX and clamped weight gradients side by side at size
    big = [g for c in R.PURE_CHAIN for g in R.pure_backward_launches(*c) if g.get("wgrad") and g["R"] >= 16384]
    assert {R.ex_ok(g["I"], g["J"], g["R"]) for g in big} == {True, False}
    big = [g for c in R.PINN_GEMM for g in R.pinn_backward_launches(*c) if g.get("wgrad") and g["R"] >= 2000]
    assert {R.ex_ok(g["I"], g["J"], g["R"]) for g in big} == {True, False}
    # the generic path: both sides of the split cap, a scan of three chunks or more
    edge = R.GENERIC_MIN_ROWS * R.GENERIC_MAX_SPLITS
    assert edge == 32768
    M = [c[1] * c[3] for c in R.PURE_GENERIC] + [c[3] for c in R.PINN_GENERIC] + [R.FLUX_GRAPH["E"]]
    assert any(m <= edge and R.cdiv(m, R.split_rows(m)) == R.GENERIC_MAX_SPLITS for m in M)
    assert any(m > edge and R.split_rows(m) > R.GENERIC_MIN_ROWS for m in M)
    assert R.cdiv(R.FLUX_GRAPH["N"], R.SCAN_CHUNK) >= 3 and R.cdiv(R.PURE_GENERIC[0][1] * R.PURE_GENERIC[0][3],
                                                                   R.SCAN_CHUNK) >= 3
    # every case says why
    for table in (R.PURE_CHAIN_WHY, R.PINN_GEMM_WHY, R.PURE_GENERIC_WHY, R.PINN_GENERIC_WHY):
        assert all(isinstance(c[-1], str) and len(c[-1]) > 10 for c in table)


def test_the_general_graph_is_what_it_says():
    _, nf, ei, up = R.flux_graph_inputs()
    c = R.FLUX_GRAPH
    assert nf.shape == (c["N"], 4) and ei.shape == (2, c["E"]) and up.shape == (c["E"],)
    assert ei.max() < c["first_isolated"] < c["N"] and ei.min() >= 0
    assert (ei[0] == ei[1]).sum() >= 500
    assert len({(a, b) for a, b in ei.T.tolist()}) <= c["E"] - 2000


def test_slide_blocks_lie_where_they_say():
    """Every block of test (c): whole units, at most 256 rows, a start on a stage
    boundary, inside one split; per case a block in split 0's first stage, one that
    ends a split, one in a later split, and the last split's ragged stage where whole
    chains can reach it."""
    for cases, blocks_of, back, unit_of in ((R.PURE_SLIDE, R.pure_slide_blocks, R.pure_backward_launches, lambda c: c[1]),
                                            (R.PINN_SLIDE, R.pinn_slide_blocks, R.pinn_backward_launches, lambda c: 1)):
        for c in cases:
            g = [x for x in back(*c) if x.get("wgrad")][0]
            Rr, rs, unit = g["R"], g["rsplit"], unit_of(c)
            bl = blocks_of(*c)
            assert len(bl) >= 4, (c, bl)
            for start, rows, why in bl:
                assert start % R.STAGE == 0 and start % unit == 0 and rows % unit == 0 and 0 < rows <= 256, (c, why)
                assert start // rs == (start + rows - 1) // rs and start + rows <= Rr, (c, why)
            assert any(s == 0 for s, _, _ in bl)
            assert any((s + n) % rs == 0 for s, n, _ in bl)           # ends a split: its last stage
            assert any(s // rs >= 1 and s % rs == 0 for s, _, _ in bl)  # begins a later split
    # the ragged last stage is reached at N = 16368 (PureGNN) and in both PINN cases; at N = 16448 the
    # 32-row last split is half a chain, which no block of whole chains inside one split can cover
    assert any(s + n == 16368 for s, n, _ in R.pure_slide_blocks(128, 16, 1, 1023))
    assert any(s + n == 16384 and n == 256 for s, n, _ in R.pure_slide_blocks(128, 64, 2, 256))
    assert any(s + n == 2000 and n == 80 for s, n, _ in R.pinn_slide_blocks(192, 256, 4, 2000))
    assert any(s + n == 8193 and n == 33 for s, n, _ in R.pinn_slide_blocks(192, 256, 3, 8193))
    assert any("remap" in w for _, _, w in R.pure_slide_blocks(64, 64, 2, 257))
    # the generic path's blocks, placed by gemm_wgrad's own splits
    for M, unit in ((R.PURE_GENERIC[1][1] * R.PURE_GENERIC[1][3], R.PURE_GENERIC[1][1]), (R.PINN_GENERIC[0][3], 1)):
        rs = R.split_rows(M)
        bl = R.slide_blocks(M, rs, unit, [])
        assert len(bl) >= 4 and rs > R.GENERIC_MIN_ROWS
        for start, rows, why in bl:
            assert start % R.STAGE == 0 and start % unit == 0 and rows % unit == 0 and 0 < rows <= 256, why
            assert start // rs == (start + rows - 1) // rs and start + rows <= M, why
        assert any(s + n == M for s, n, _ in bl) and any(s // rs == 1 for s, _, _ in bl)
    assert R.PURE_TWICE in R.PURE_CHAIN and R.PINN_TWICE in R.PINN_GEMM
    assert set(R.PURE_SLIDE) <= set(R.PURE_CHAIN) and set(R.PINN_SLIDE) <= set(R.PINN_GEMM)


# ------------------------------------------------------------------- the gate is sharp
def moved(got, want):
    return float(np.abs(got - want).max()) / float(np.abs(want).max())


def check_mutants(ops, grads, rsplit, fold, applicable):
    """splitk reproduces autograd on every operand pair; every mutant moves at least
    one tensor by more than 10x the gate."""
    worst = {m: 0.0 for m in R.MUTANTS}
    for k, (A, X) in ops.items():
        H = grads[k].shape[0]
        assert moved(fold(R.splitk(A, X, rsplit), H, k), grads[k]) <= 1e-12, k
        for m in R.MUTANTS:
            got = R.splitk(A, X, rsplit, m)
            if got is not None:
                worst[m] = max(worst[m], moved(fold(got, H, k), grads[k]))
    for m in R.MUTANTS:
        if m in applicable:
            assert worst[m] > 10 * R.REL, (m, worst[m])
        else:
            assert worst[m] == 0.0, m


@pytest.mark.parametrize("H,nx,L,B", R.PURE_CHAIN)
def test_pure_mutants_are_rejected_and_restatement_is_the_oracle(H, nx, L, B):
    sd, nf, up = R.pure_inputs(H, nx, L, B)
    N = B * nx
    d, grads, gnf, ops = R.pure_chain_operands64(sd, nf, up, nx)
    # the per-cell restatement is the oracle's forward on chain_edges
    wd, wg, wnf = R.oracle_run(O.pure_gnn_forward, sd, nf, up, torch.float64, O.chain_edges(nx, B))
    assert np.abs(d - wd).max() <= 1e-12 and moved(gnf, wnf) <= 1e-12
    for k in wg:
        assert moved(grads[k], wg[k]) <= 1e-12, k
    rsplit = R.tgemm_splits(N, R.pure_wg_splits(N))[0]
    fold = lambda gw, Hh, k: R.from_pq(gw, Hh) if k.startswith("update_mlps") else gw  # noqa: E731
    applicable = {"split", "tile", "out"} | ({"ragged"} if N % R.STAGE else set())
    check_mutants(ops, grads, rsplit, fold, applicable)


@pytest.mark.parametrize("D,H,L,B", R.PINN_GEMM)
def test_pinn_mutants_are_rejected_and_restatement_is_the_oracle(D, H, L, B):
    sd, st, up = R.pinn_inputs(D, H, L, B)
    out, grads, gs, ops = R.pinn_operands64(sd, st, up)
    wo, wg, ws = R.oracle_run(O.pinn_forward, sd, st, up, torch.float64)
    assert np.abs(out - wo).max() <= 1e-12 and moved(gs, ws) <= 1e-12
    for k in wg:
        assert moved(grads[k], wg[k]) <= 1e-12, k
    rsplit = R.tgemm_splits(B, R.pinn_wg_splits(B))[0]
    applicable = {"split", "tile", "out"} | ({"ragged"} if B % R.STAGE else set())
    check_mutants(ops, grads, rsplit, lambda gw, Hh, k: gw, applicable)


def test_ragged_mutant_applies_where_the_cases_say():
    assert [c for c in R.PURE_CHAIN if c[1] * c[3] % R.STAGE] == [(128, 16, 1, 1023)]
    assert [c for c in R.PINN_GEMM if c[3] % R.STAGE] == [(192, 256, 4, 2000), (192, 256, 3, 8193)]


# ----------------------------------------------------- the reference alone, f32 vs f64
def reference_noise(forward, sd, x, up, *extra):
    o32, g32, x32 = R.oracle_run(forward, sd, x, up, torch.float32, *extra)
    o64, g64, x64 = R.oracle_run(forward, sd, x, up, torch.float64, *extra)
    assert (np.abs(o32 - o64) <= 0.25 * (2e-6 + 1e-5 * np.abs(o64))).all()
    worst = max([moved(g32[k], g64[k]) for k in g64] + [moved(x32, x64)])
    assert worst <= 0.25 * R.REL, worst
    return worst


@pytest.mark.parametrize("H,nx,L,B", R.PURE_CHAIN + R.PURE_GENERIC)
def test_pure_reference_alone_is_inside_the_gate(H, nx, L, B):
    sd, nf, up = R.pure_inputs(H, nx, L, B)
    reference_noise(O.pure_gnn_forward, sd, nf, up, O.chain_edges(nx, B))


@pytest.mark.parametrize("D,H,L,B", R.PINN_GEMM + R.PINN_GENERIC)
def test_pinn_reference_alone_is_inside_the_gate(D, H, L, B):
    sd, st, up = R.pinn_inputs(D, H, L, B)
    reference_noise(O.pinn_forward, sd, st, up)


def test_flux_graph_reference_alone_is_inside_the_gate():
    sd, nf, ei, up = R.flux_graph_inputs()
    reference_noise(O.flux_gnn_forward, sd, nf, up, torch.from_numpy(ei))
    # kink-free: every ReLU input of the float64 evaluation is well away from 0
    p = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items()}
    h = torch.as_tensor(nf, dtype=torch.float64) @ p["input_mlp.0.weight"].T + p["input_mlp.0.bias"]
    assert float(h.min()) > 1.0
