"""tests/chain_regimes.py against the sources and against itself.  No GPU.

  constants ......... every constant and restated formula of the table as csrc/ writes
      it: a moved threshold fails here until the table, and the sizes around it, move too
  numbers ........... every figure in a case's `why` recomputed from the restatements:
      fused passes and the ragged group (at 256 CUs), trips of the edge kernels, stages
      per split and their parity, short last splits, row tiles, splits below slices
  cases ............. per case, on the float64 reference alone: the seed is the recorded
      one, the layer-by-layer restatement (tape64 / backward64) gives exact_cases'
      flux and gradients bit for bit, every ReLU' mask holds both values on 5 % of its
      entries (among the chains of the last fused pass too), every gradient tensor is
      non-zero on 25 % of its entries, and each mutant that applies to the case's regime
      (chains of a later pass or of the ragged group dropped, a halo row from the
      neighbouring chain, a split's last stage dropped, a mask word from the chain
      4 CUs back) changes a compared tensor, which the bitwise gate then rejects
"""
import os
import re

import numpy as np
import pytest
import torch

import chain_regimes as C
import exact_cases as X
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


def const(name, text):
    return int(one(r"constexpr\s+int(?:64_t)?\s+(?:\w+\s*=\s*\d+\s*,\s*)*" + name + r"\s*=\s*(\d+)\s*[,;]", text))


def test_constants_match_the_sources():
    tc, cc, f32, hi = src("train_chain.hip"), src("chain_common.h"), src("chain_f32.hip"), src("hf_internal.h")
    assert const("kWaves", cc) == C.NW
    core = f32[f32.index("struct CoreF32T"):f32.index("using CoreF32 =")]
    assert one(r"static constexpr int kNW = (\w+);", core) == "kWaves"
    assert int(one(r"static constexpr int kWGPerCU = (\d+);", core)) == C.WG_PER_CU
    assert const("kEdgeBlocks", tc) == C.EDGE_BLOCKS and const("kEbCells", tc) == C.EB_CELLS
    assert const("kWgsSplits", tc) == C.WGS_SPLITS and const("kWsKC", tc) == C.WS_KC == R.STAGE
    assert const("kWsH", tc) == C.FUSED_H == const("kH", hi) and const("kIn", hi) == C.FUSED_IN
    assert const("kMaxChainLayers", hi) == C.MAX_LAYERS
    assert const("kWgradSplits", tc) == C.WGRAD_SPLITS and const("kWgradBatchSplits", tc) == C.BATCH_SPLITS
    assert const("kInputSplits", tc) == C.INPUT_SPLITS and const("kPrSlices", tc) == C.PR_SLICES
    # both edge kernels: kEdgeBlocks blocks of 256 threads, a wave steps by 4 gridDim.x units
    assert len(re.findall(r"edge_backward(?:_h128)?_kernel, dim3\(kEdgeBlocks\), dim3\(256\)", tc)) == 2
    assert len(re.findall(r"\+= \(int64_t\)gridDim\.x \* 4\)", tc)) == 2 and C.EDGE_WAVES == 256 // 64
    assert one(r"const int segs = \(nx \+ kEbCells - 1\) / kEbCells;", tc)
    assert one(r"if \(H == 128\)\s*hipLaunchKernelGGL\(edge_backward_h128_kernel", tc)
    # the fused kernels' grid and their persistent loops
    tb = f32[f32.index("int64_t train_blocks(int64_t B)"):f32.index("hipError_t train_fwd_launch")]
    assert one(r"groups = \(B \+ CoreF32::kNW - 1\) / CoreF32::kNW;", tb)
    assert one(r"res = \(int64_t\)resident_groups\(\) \* CoreF32::kWGPerCU;", tb)
    assert one(r"return groups < res \? groups : res;", tb)
    assert len(re.findall(r"for \(int64_t grp = blockIdx\.x; grp < groups; grp \+= gridDim\.x\)", cc)) >= 3
    fwd = cc[cc.index("void chain_train_fwd_kernel"):cc.index("void chain_train_bwd_kernel")]
    assert one(r"if \(grp \+ gridDim\.x < groups\) load_feat\(grp \+ gridDim\.x, pre\);", fwd)
    assert one(r"T\.mstride = items \* MT \* 64, T\.mrow = b \* MT \* 64", fwd)
    # a mask word: lane group g = lane >> 4 holds channels 4 g + 16 nt + r in bit 4 nt + r (chain_regimes.mask_word)
    assert len(re.findall(r"mbits\[\w+ \* mstride \+ b \* MT \* 64 \+ mt \* 64 \+ lane\]", cc)) == 2
    assert len(re.findall(r"\(mb\[mt\] >> \(4 \* nt \+ r\)\) & 1u", cc)) == 2
    assert one(r"g4 = 4 \* \(lane >> 4\);", cc[cc.index("void chain_train_bwd_kernel"):])
    fo = f32[f32.index("bool chain_train_fused_ok"):]
    assert one(r"w\.in_dim == kIn && w\.hidden == kH && w\.layers >= 0 && w\.layers <= kMaxChainLayers &&\s*"
               r"\(nx == 16 \|\| nx == 32 \|\| nx == 48 \|\| nx == 64\);", fo)
    assert C.FUSED_NX == (16, 32, 48, 64)
    # the launch shapes of the backward
    assert one(r"const bool wgs = wg_batch && nx % kWsKC == 0 && N % kWsKC == 0 && N \* kWsH < \(int64_t\(1\) << 31\);", tc)
    assert one(r"const bool wg_batch = fused && L >= 1;", tc)
    assert one(r"return \(\(N \+ kWgsSplits - 1\) / kWgsSplits \+ kWsKC - 1\) / kWsKC \* kWsKC;", tc)
    assert one(r"wgs_splits\(int64_t N\) \{ return \(N \+ wgs_rsplit\(N\) - 1\) / wgs_rsplit\(N\); \}", tc)
    assert one(r"SB = wgs \? wgs_splits\(N\) : tgemm_splits\(N, kWgradBatchSplits\);", tc)
    assert len(re.findall(r"tgemm_splits\(N, kWgradSplits\)", tc)) == 2
    assert len(re.findall(r"\(N \+ kInputSplits - 1\) / kInputSplits", tc)) == 2
    assert one(r"const int nsp = \(int\)\(\(N \+ rows - 1\) / rows\);", tc)
    assert len(re.findall(r"s0 = \(int\)\(\(int64_t\)S \* q / kPrSlices\), s1 = \(int\)\(\(int64_t\)S \* \(q \+ 1\) / kPrSlices\)",
                          tc)) == 1
    assert one(r"H >= kKC && H <= (\d+) && \(H & \(H - 1\)\) == 0", tc) == "256"
    assert one(r"w\.in_dim <= (\d+) && N > 0 && N \* 2 \* H \+ 2 \* H < \(int64_t\(1\) << 31\)", tc) == "8"
    # wgrad_stencil_kernel: whole stages in pairs plus an odd last one; halo rows wrapped inside the chain
    ws = tc[tc.index("void wgrad_stencil_kernel"):tc.index("inline int64_t wgs_rsplit")]
    assert one(r"for \(; k \+ 2 <= nst; k \+= 2\)", ws) and one(r"if \(k < nst\) stage\(std::integral_constant<int, 0>\{\}, k\);", ws)
    assert one(r"t < 32 \? \(i0 == 0 \? r0 \+ nx - 1 : r0 - 1\) : \(i0 \+ kWsKC == nx \? r0 \+ kWsKC - nx : r0 \+ kWsKC\)", ws)


def reg(nx, B, L, H, in_dim=4):
    r = C.regime(nx, B, L, H, in_dim)
    assert r["ok"], (nx, B, L, H)
    return r


def stages(r):
    _, rsplit, S = r["layers"]
    return R.stage_counts(r["N"], rsplit)


def test_the_numbers_of_the_fused_cases():
    r = reg(64, 1027, 2, 128)
    assert r["fused"] and (r["passes"], r["last_group"], r["last_pass_from"]) == (2, 3, 1024) and C.cdiv(1027, 4) == 257
    assert r["edge_kernel"] == "h128" and r["edge_trips"] == 3
    assert r["layers"] == ("stencil", 544, 121) and stages(r) == [17] * 120 + [14]
    r0 = reg(64, 1027, 0, 128)
    assert r0["fused"] and r0["layers"] is None and (r0["passes"], r0["last_group"]) == (2, 3)
    assert r0["input"] == (129, 510) and r0["edge"] == R.tgemm_splits(65728, 256) == (288, 229)
    r = reg(32, 2051, 2, 128)
    assert (r["passes"], r["last_group"], r["last_pass_from"]) == (3, 3, 2048)
    assert r["layers"] == ("stencil", 544, 121) and stages(r) == [17] * 120 + [11]
    r = reg(32, 131, 2, 128)
    assert r["N"] == 4192 and r["layers"] == ("stencil", 64, 66) and stages(r) == [2] * 65 + [1]
    assert stages(reg(32, 128, 2, 128)) == [1] * 128            # N = 4096: the last size with one stage per split
    r = reg(32, 12, 1, 128)
    assert r["N"] == 384 and r["layers"] == ("stencil", 32, 12) and r["passes"] == 1
    assert sum(a == b for a, b in C.slice_cuts(12)) == 4 and r["input"] == (1, 384)
    assert sum(b - a for a, b in C.slice_cuts(12)) == 12
    r = reg(16, 4100, 1, 128)
    assert r["layers"] == ("batch", 1056, 63) and stages(r) == [33] * 62 + [4]
    assert (r["passes"], r["last_group"], r["edge_trips"]) == (5, 4, 3)
    r = reg(48, 1030, 2, 128)
    assert r["layers"] == ("batch", 800, 62) and stages(r) == [25] * 61 + [20]
    assert (r["passes"], r["last_group"], r["edge_trips"]) == (2, 2, 2)
    assert 800 % 48 and R.STAGE % 48 and r["N"] % R.STAGE == 0   # stages and splits cut chains; whole stages
    r = reg(64, 2000, 4, 128)
    assert (r["passes"], r["last_group"]) == (2, 4) and r["layers"] == ("stencil", 1024, 125) and set(stages(r)) == {32}
    assert r["edge_trips"] == 4


def test_the_numbers_of_the_gemm_cases():
    r = reg(100, 700, 2, 128)
    assert not r["fused"] and r["N"] == 70000 > 8192 and r["row_tiles"] == 547 and 547 % C.REMAP_GROUP == 3
    assert r["layers"] == ("gemm", 288, 244) == ("gemm",) + r["edge"] and stages(r) == [9] * 243 + [1]
    assert R.last_stage_rows(70000, 288) == 16
    assert r["edge_kernel"] == "h128" and r["edge_trips"] == 3 and C.cdiv(100, C.EB_CELLS) == 13 and 100 % C.EB_CELLS == 4
    r = reg(7, 9000, 1, 128)
    assert not r["fused"] and 7 < C.EB_CELLS and r["edge_kernel"] == "h128" and r["edge_trips"] == 3
    assert r["layers"] == ("gemm", 256, 247) and r["row_tiles"] == 493
    for (nx, B, L, H), trips in (((64, 1100, 2, 64), 18), ((64, 1100, 1, 32), 18), ((64, 600, 2, 256), 10)):
        r = reg(nx, B, L, H)
        assert not r["fused"] and r["edge_kernel"] == "any" and r["edge_trips"] == trips and r["row_tiles"] >= 16
        assert r["layers"][0] == "gemm" and r["N"] > 8192 and min(stages(r)[:-1]) >= 2
    for nx, B, L, H, F, _ in C.IN_DIM_WHY:
        r = reg(nx, B, L, H, F)
        assert not r["fused"] and F != C.FUSED_IN and r["layers"][0] == "gemm"


def test_every_regime_is_reached():
    regs = {s: reg(*s) for s in C.SHAPES}
    fused = {s: r for s, r in regs.items() if r["fused"]}
    assert {r["passes"] for r in fused.values()} >= {1, 2, 3}
    assert any(r["passes"] > 1 and r["last_group"] < C.NW and r["last_pass_from"] + r["last_group"] == s[1]
               for s, r in fused.items())                                     # a ragged group in a later pass
    assert any(r["passes"] > 1 and r["layers"] is None for r in fused.values())  # L = 0 with passes
    for kernel in ("h128", "any"):
        assert any(r["edge_kernel"] == kernel and r["edge_trips"] >= 2 for r in regs.values()), kernel
    assert any(s[0] < C.EB_CELLS and r["edge_trips"] >= 2 for s, r in regs.items())
    st = {s: r for s, r in regs.items() if r["layers"] and r["layers"][0] == "stencil"}
    counts = [n for r in st.values() for n in stages(r)]
    assert {n % 2 for n in counts if n > 1} == {0, 1} and 1 in counts and 2 in counts
    assert any(len(set(stages(r))) > 1 for r in st.values())                  # a short last split
    assert any(r["layers"][2] < C.WGS_SPLITS for r in st.values()) and any(r["layers"][2] < C.PR_SLICES for r in st.values())
    assert {s[0] for s in st} == {32, 64}
    assert any(s[0] == 32 and max(stages(r)) > 1 for s, r in st.items())      # both halos wrap, with a hand-over
    bt = {s: r for s, r in regs.items() if r["layers"] and r["layers"][0] == "batch"}
    assert {s[0] for s in bt} == {16, 48} and all(max(stages(r)) > 1 and r["passes"] > 1 for r in bt.values())
    gm = {s: r for s, r in regs.items() if r["layers"] and r["layers"][0] == "gemm"}
    assert {s[3] for s in gm} == {32, 64, 128, 256}
    assert all(r["row_tiles"] >= C.REMAP_GROUP and r["N"] > 8192 for r in gm.values())
    assert all(isinstance(c[-1], str) and len(c[-1]) > 10 for c in C.CASES_WHY + C.IN_DIM_WHY)
    assert set(C.TWICE) <= set(C.SHAPES) and (64, 2000, 4, 128) in C.SHAPES
    # the limits of the issue: L <= 2 above B = 2048, and nothing larger than the benchmark's rows x layers
    assert all(s[2] <= 2 for s in C.SHAPES if s[1] > 2048)
    assert max(s[0] * s[1] * (s[2] + 1) * s[3] for s in C.SHAPES) == 64 * 2000 * 5 * 128


def test_fewer_cus_only_add_passes():
    for nx, B, L, H in C.SHAPES:
        for cus in (64, 128, 192, 240, 256, 304):
            if cus <= C.CUS:
                assert C.fused_passes(B, cus) >= C.fused_passes(B)
    assert C.fused_passes(1024) == 1 and C.fused_passes(1025) == 2 and C.train_blocks(9) == 3


@pytest.mark.parametrize("case", [c for c in C.CASES if c.B * c.nx <= 5000], ids=lambda c: c.name)
def test_small_cases_equal_the_pinned_oracle_in_float32(case):
    b = X.find_case(case)
    p = {k: v.clone().requires_grad_(True) for k, v in O.params_from(b.sd).items()}
    nf = torch.from_numpy(b.nf).clone().requires_grad_(True)
    fe = O.flux_gnn_forward(p, nf, O.chain_edges(case.nx, case.B))
    (fe * torch.from_numpy(b.gup)).sum().backward()
    assert np.array_equal(fe.detach().numpy().astype(np.float64), b.flux.reshape(-1))
    assert np.array_equal(nf.grad.numpy().astype(np.float64), b.grads["node_features"])
    for k, v in p.items():
        assert np.array_equal(v.grad.numpy().astype(np.float64), b.grads[k]), k


def applicable(case):
    r = C.regime(case.nx, case.B, case.layers, case.hidden, case.in_dim)
    want = {"stage0", "stageZ"}
    if case.layers >= 1:
        want.add("halo")
    if r["fused"] and r["passes"] > 1:
        want |= {"pass2", "maskword"}
    if r["fused"] and case.B % C.NW:
        want.add("ragged")
    return want


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_case_conditions_and_mutants(case):
    b = X.find_case(case)
    assert b.seed == case.seed0 == C.SEED0.get(case.name, 0) and X.accept(b) == []
    assert b.grec.max_bound() * 2.0 ** b.grec.m < 2.0 ** 24
    T = C.tape64(b.sd, b.nf, case.B, case.nx)
    assert np.array_equal(T["flux"], b.flux)
    grads, G, dPQ, _ = C.backward64(b.sd, T, b.gup)
    assert set(grads) == set(b.grads)
    for k in grads:
        assert np.array_equal(grads[k].reshape(b.grads[k].shape), b.grads[k]), k
    assert C.extra_conditions(case, b, T) == []
    muts = C.mutants(case, b, T, G, dPQ)
    assert set(muts) == applicable(case)
    for name, moved in muts.items():
        assert moved, name
        changed = {k for k, d in moved.items() if np.any(d != 0)}
        assert changed, (name, "changes no compared tensor")
        if name != "maskword":   # the weight tensors it touches all move: every layer's gate is sharp
            assert changed >= {k for k in moved if k.endswith("weight")}, (name, sorted(set(moved) - changed))


def test_mutant_helpers():
    h = np.arange(12.0).reshape(6, 2)
    rows = np.arange(6)
    want = np.concatenate([h, C.agg(h, 2, 3)], 1)
    assert np.array_equal(C.stencil_rows(h, 2, 3, rows), want)
    got = C.stencil_rows(h, 2, 3, rows, True)
    assert np.array_equal(got[[1, 2, 4, 5]], want[[1, 2, 4, 5]]) and not np.array_equal(got[[0, 3]], want[[0, 3]])
    assert list(C.last_stage_rows(100, 64, 0)) == list(range(32, 64)) and list(C.last_stage_rows(100, 64, 1)) == list(range(96, 100))
    cell, ch = C.mask_word(64, 5, 2)
    assert cell == 5 and len(ch) == 32 and ch[0] == 8 and ch[4] == 24 and ch.max() == 123
    assert sorted(np.concatenate([C.mask_word(64, 0, g)[1] for g in range(4)])) == list(range(128))
