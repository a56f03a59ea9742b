"""What a real stencil radius costs in the fused f32 rollout.

BASELINE cfg3 (4096 ICs x 64 cells, T = 50, float32, run_batch(traj=False) into
a preallocated output) with the same weights at graph radius R = 1, 2, 3: the
radius-R kernels form 2R - 1 adds per value and k-step where radius 1 forms
one (csrc/chain_common.h nb_sum_radius), scheduled between the MFMAs of the
k-step before.  Arms in alternating windows on the same GPU in the same process
(a window = `inner` calls back to back between device synchronisations, host
clock; `inner` chosen so that a window lasts about --window-ms):

  r1, r2, r3   HybridSolver(graph_radius=R).run_batch, one persistent launch
  generic_r3   the only way a radius model could run before: per step
               hf_graph_flux on the radius-3 edge list + hf_unroll_update
               (FV update, Poisson, next node features), sequenced from Python,
               at the same shape (fewer steps: --generic-steps, scaled per step)

Reported per arm: the median window's ms per call, min..max over the windows,
IC-steps/s; the ratios R/1 of the medians with the min..max of the
window-by-window ratios; generic over fused at R = 3 per step.  There is no
gate: the record states what was measured.  --parent DIR (a built checkout of
the parent commit) adds `python bench.py --gpus 1` of this tree against the
same command there, alternating, --bench-runs each.  Every part runs in a child
process under a time limit; after a child that fails or runs out of time no
further child is started.  Prints one JSON line and writes it to --out.

    python tools/bench_radius.py [--windows 9] [--parent DIR] [--out profiles/radius_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnn-plasma-flux_amd"))
sys.path.insert(0, ROOT)


def timed(arms, windows, window_ms, sync):
    def window(fn, n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return (time.perf_counter() - t0) * 1e3 / n

    for fn in arms.values():
        window(fn, 2)
    inner = {k: max(1, int(window_ms / max(window(fn, 2), 1e-3))) for k, fn in arms.items()}
    t_end = time.perf_counter() + 0.3  # back-to-back load before timing: the clock ramps under load
    while time.perf_counter() < t_end:
        for k, fn in arms.items():
            window(fn, inner[k])
    ms = {k: [] for k in arms}
    for _ in range(windows):
        for k, fn in arms.items():
            ms[k].append(window(fn, inner[k]))
    return ms, inner


def stats(v):
    return {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def ratio(num, den, scale=1.0):
    r = [scale * x / y for x, y in zip(num, den)]
    return {"median": round(scale * statistics.median(num) / statistics.median(den), 4), "min": round(min(r), 4),
            "max": round(max(r), 4)}


def child(B, T, Tg, windows, window_ms):
    import numpy as np
    import torch

    import hybridflux as hf
    from hybridflux import engine
    from hybridflux._lib import version
    from hybridflux.graph_constructor import chain_edge_index
    dev = torch.device("cuda", 0)
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_W1_r3.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    ss = {R: hf.HybridSolver(sd, R, nx=64, device=dev, graph_radius=R) for R in (1, 2, 3)}
    ics = ss[1].baseline.initial_conditions(range(1000, 1000 + B), as_tensor=True)
    outs = {R: torch.empty_like(ics) for R in ss}
    grid = ss[3].grid
    dm = ss[3].model.device_model(dev)            # natural-layout weights: the generic path ignores the radius
    ei = chain_edge_index(64, B, dev, radius=3)
    x = grid.on(dev)[0]
    ws = engine.unroll_workspace(B, 64, dev)

    def generic():
        st = ics
        nf = torch.stack([st[:, 0], st[:, 1], st[:, 2], x.expand(B, 64)], dim=-1).reshape(B * 64, 4).contiguous()
        for _ in range(Tg):
            fe = engine.graph_flux(dm, nf, ei).reshape(B, 6 * 64)[:, :128].contiguous()
            st, nf, _ = engine.unroll_update(grid, fe, st, x=x, ws=ws)
        return st

    arms = {f"r{R}": (lambda R=R: ss[R].run_batch(ics, T, traj=False, out=outs[R])) for R in ss}
    arms["generic_r3"] = generic
    ms, inner = timed(arms, windows, window_ms, lambda: torch.cuda.synchronize(dev))
    res = {}
    for k, v in ms.items():
        steps = Tg if k == "generic_r3" else T
        res[k] = dict(stats(v), calls_per_window=inner[k], steps=steps,
                      ic_steps_per_s=round(B * steps / statistics.median(v) * 1e3, 1))
    res["r2_over_r1"] = ratio(ms["r2"], ms["r1"])
    res["r3_over_r1"] = ratio(ms["r3"], ms["r1"])
    res["generic_over_fused_r3_per_step"] = ratio(ms["generic_r3"], ms["r3"], scale=T / Tg)
    spread = (res["r1"]["ms_max"] - res["r1"]["ms_min"]) / res["r1"]["ms"]
    res["r1_window_spread"] = round(spread, 4)
    # the generic path and the fused kernel agree on the states they reach (not bitwise at R = 3: W_b / 6 against mean / 6)
    fused = ss[3].run_batch(ics, Tg, traj=False)["final"]
    res["generic_vs_fused_r3_max_abs_diff"] = float((generic() - fused).abs().max())
    print("RESULT " + json.dumps({"part": "radius", "ics": B, "cells": 64, "steps": T, "precision": "f32",
                                  "windows": windows, "lib": version(), "result": res}))


def run_child(args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--windows", str(args.windows), "--window-ms",
           str(args.window_ms), "--steps", str(args.steps), "--generic-steps", str(args.generic_steps), "--ics",
           str(args.ics)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_radius: the radius arms ran past {args.timeout} s; stopping")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"bench_radius: the radius arms failed (exit {p.returncode}); stopping")
    return json.loads(line[-1][7:])


def bench_headline(tree, args):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "10"]
    env = {k: v for k, v in os.environ.items() if k != "HYBRIDFLUX_LIB"}
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=args.timeout, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"bench_radius: bench.py in {tree} failed (exit {p.returncode}); stopping")
    r = json.loads(lines[-1])
    return float(r["value"]), r.get("build", "")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=150.0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--generic-steps", type=int, default=5)
    ap.add_argument("--ics", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--parent", help="a built checkout of the parent commit (bench.py headline A/B)")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.ics, a.steps, a.generic_steps, a.windows, a.window_ms)
    doc = {"tool": "tools/bench_radius.py", "radius": run_child(a)}
    if a.parent:
        this, parent, builds = [], [], {}
        for _ in range(a.bench_runs):
            for tree, acc, name in ((a.parent, parent, "parent"), (ROOT, this, "this")):
                v, builds[name] = bench_headline(tree, a)
                acc.append(v)
        mt, mp = statistics.median(this), statistics.median(parent)
        spread = max((max(v) - min(v)) / statistics.median(v) for v in (this, parent))
        doc["bench_headline"] = {"steps": a.steps, "runs_each": a.bench_runs, "this": this, "parent": parent,
                                 "builds": builds, "this_over_parent": round(mt / mp, 4),
                                 "largest_run_spread": round(spread, 4),
                                 "within_spread": bool(abs(mt / mp - 1.0) <= spread)}
    else:
        doc["bench_headline"] = "not measured (no --parent)"
    line = json.dumps(doc)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
