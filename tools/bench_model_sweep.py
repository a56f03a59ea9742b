"""One launch for a set of FluxGNN checkpoints against one launch per checkpoint.

The reference's model sweep (scripts/evaluation/evaluate_multi_ic.py:105-136,
evaluate_all.py:177-190): 12 hybrid models of FluxGNN(4,128,4) with distinct
random weights, 50 ICs x 64 cells, T = 50, float32; and the same at 12 x 512
ICs, where one model alone already fills half the GPU.  Arms, in alternating
windows on the same GPU in the same process (a window = `inner` calls back to
back between device synchronisations, host clock; `inner` is chosen so that a
window lasts about --window-ms):

  grouped  HybridEnsemble of the 12 solvers, one call
  loop     the 12 HybridSolvers, one call each

each scored (compare_batch: classical twin, mse, both metric series) and
unscored (run_batch(traj=False, metrics=True), what evaluation.long_rollout
asks for).  The two arms return the same bits (tests/test_gpu_model_set.py gates
it; checked here once more on what was timed).

Two no-regression measurements ride along:

  m1       a set of ONE model against the single-model call at BASELINE cfg3
           (4096 ICs x 64 cells, 50 steps, run_batch(traj=False) into
           preallocated outputs): what the table lookup costs.
  bench    `python bench.py --gpus 1` of this tree against the same command in
           --parent DIR, a built checkout of the parent commit, alternating,
           --bench-runs each: the headline value of both with their spreads.
           Without --parent it is recorded as not measured.

Reported per arm: the median window's ms per call and the min..max over the
windows; per pair the ratio of the medians and the min..max of the
window-by-window ratios.  No ratio is a target: the record states what was
measured.  Each part runs in a child process of its own under a time limit;
after a child that fails or runs out of time no further child is started.
Prints one JSON line and writes it to --out.

    python tools/bench_model_sweep.py [--windows 9] [--parent DIR] [--out FILE]
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


def timed_pairs(arms, windows, window_ms, sync):
    """Alternating windows of every arm: {arm: [ms per call]} and the calls per window."""
    def window(fn, n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return (time.perf_counter() - t0) * 1e3 / n

    for fn in arms.values():  # warm-up of every arm (allocations, first launches, the set's table)
        window(fn, 2)
    inner = {k: max(1, int(window_ms / max(window(fn, 3), 1e-3))) for k, fn in arms.items()}
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


def ratio(num, den):
    r = [x / y for x, y in zip(num, den)]  # window by window, as they alternated
    return {"median": round(statistics.median(num) / statistics.median(den), 4), "min": round(min(r), 4),
            "max": round(max(r), 4)}


def solvers(M, dev, layers=4):
    import torch

    import hybridflux as hf
    out = []
    for i in range(M):
        torch.manual_seed(1000 + i)
        sd = hf.FluxGNN(4, 128, layers).state_dict()
        out.append(hf.HybridSolver(sd, 1, nx=64, device=dev, num_layers=layers))
    return out


def same_bits(a, b):
    import torch
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in ((a[k], b[k]) for k in a))


def child_sweep(B, M, T, windows, window_ms):
    import torch

    import hybridflux as hf
    from hybridflux._lib import version
    dev = torch.device("cuda", 0)
    ss = solvers(M, dev)
    ens = hf.HybridEnsemble(ss)
    ics = ss[0].baseline.initial_conditions(range(1000, 1000 + B), as_tensor=True)
    arms = {
        "grouped_scored": lambda: ens.compare_batch(ics, T),
        "loop_scored": lambda: [s.compare_batch(ics, T) for s in ss],
        "grouped_unscored": lambda: ens.run_batch(ics, T, traj=False, metrics=True),
        "loop_unscored": lambda: [s.run_batch(ics, T, traj=False, metrics=True) for s in ss],
    }
    ms, inner = timed_pairs(arms, windows, window_ms, lambda: torch.cuda.synchronize(dev))
    res = {k: dict(stats(v), calls_per_window=inner[k], ic_steps_per_s=round(M * B * T / statistics.median(v) * 1e3, 1))
           for k, v in ms.items()}
    for kind in ("scored", "unscored"):
        res[f"loop_over_grouped_{kind}"] = ratio(ms[f"loop_{kind}"], ms[f"grouped_{kind}"])
        g, l = arms[f"grouped_{kind}"](), arms[f"loop_{kind}"]()
        res[f"same_bits_{kind}"] = bool(same_bits(g, {k: None if l[0][k] is None else torch.stack([r[k] for r in l])
                                                      for k in l[0]}))
    print("RESULT " + json.dumps({"part": "sweep", "models": M, "ics_per_model": B, "cells": 64, "steps": T,
                                  "precision": "f32", "windows": windows, "lib": version(), "result": res}))


def child_m1(B, T, windows, window_ms):
    import torch

    import hybridflux as hf
    from hybridflux._lib import version
    dev = torch.device("cuda", 0)
    s = solvers(1, dev)[0]
    ens = hf.HybridEnsemble([s])
    ics = s.baseline.initial_conditions(range(1000, 1000 + B), as_tensor=True)
    out1, outm = torch.empty_like(ics), torch.empty(1, *ics.shape, device=dev)
    arms = {"single": lambda: s.run_batch(ics, T, traj=False, out=out1),
            "set_of_one": lambda: ens.run_batch(ics, T, traj=False, out=outm)}
    ms, inner = timed_pairs(arms, windows, window_ms, lambda: torch.cuda.synchronize(dev))
    res = {k: dict(stats(v), calls_per_window=inner[k], ic_steps_per_s=round(B * T / statistics.median(v) * 1e3, 1))
           for k, v in ms.items()}
    res["set_over_single"] = ratio(ms["set_of_one"], ms["single"])
    spread = (res["single"]["ms_max"] - res["single"]["ms_min"]) / res["single"]["ms"]
    res["single_window_spread"] = round(spread, 4)
    res["set_slower_than_single_by"] = round(res["set_over_single"]["median"] - 1.0, 4)
    res["within_spread"] = bool(res["set_over_single"]["median"] - 1.0 <= spread)
    res["same_bits"] = bool(torch.equal(out1.view(torch.int32), outm[0].view(torch.int32)))
    print("RESULT " + json.dumps({"part": "m1", "ics": B, "cells": 64, "steps": T, "precision": "f32",
                                  "windows": windows, "lib": version(), "result": res}))


def run_child(args, extra, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--windows", str(args.windows), "--window-ms",
           str(args.window_ms), "--steps", str(args.steps), "--models", str(args.models)] + extra
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_model_sweep: {what} ran past {args.timeout} s; stopping")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"bench_model_sweep: {what} failed (exit {p.returncode}); stopping")
    return json.loads(line[-1][7:])


def bench_headline(tree, args):
    """One `python bench.py --gpus 1` in `tree`: its result line's value (IC-steps/s)."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "10"]
    env = {k: v for k, v in os.environ.items() if k != "HYBRIDFLUX_LIB"}
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=args.timeout, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"bench_model_sweep: bench.py in {tree} failed (exit {p.returncode}); stopping")
    r = json.loads(lines[-1])
    return float(r["value"]), r.get("build", "")


def bench_pair(args):
    if not args.parent:
        return {"measured": False, "why": "no --parent checkout was given"}
    vals = {"this": [], "parent": []}
    libs = {}
    for _ in range(args.bench_runs):  # alternating: this, parent, this, parent, ...
        for name, tree in (("this", ROOT), ("parent", os.path.abspath(args.parent))):
            v, libs[name] = bench_headline(tree, args)
            vals[name].append(v)
    out = {"measured": True, "command": f"python bench.py --gpus 1 --steps {args.steps} --warmup 10",
           "unit": "IC-steps/s", "runs_each": args.bench_runs, "lib": libs}
    for k, v in vals.items():
        out[k] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                  "spread": round((max(v) - min(v)) / statistics.median(v), 4), "values": v}
    diff = out["this"]["median"] / out["parent"]["median"] - 1.0
    out["this_over_parent_minus_1"] = round(diff, 4)
    out["within_spread"] = bool(abs(diff) <= max(out["this"]["spread"], out["parent"]["spread"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=12)
    ap.add_argument("--ics", type=int, nargs="+", default=[50, 512], help="ICs per model of the sweep")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--m1-ics", type=int, default=4096)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (for the bench.py pair)")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_sweep_bench.json"))
    ap.add_argument("--child", nargs=2, metavar=("PART", "ICS"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.windows < 5:
        raise SystemExit("bench_model_sweep: at least 5 windows (the spread is part of the result)")
    if args.child:
        if args.child[0] == "sweep":
            child_sweep(int(args.child[1]), args.models, args.steps, args.windows, args.window_ms)
        else:
            child_m1(int(args.child[1]), args.steps, args.windows, args.window_ms)
        return
    sweep = [run_child(args, ["--child", "sweep", str(B)], f"sweep at {B} ICs") for B in args.ics]
    m1 = run_child(args, ["--child", "m1", str(args.m1_ics)], "set of one model")
    out = {"metric": "model sweep: ms per rollout call of all models x ICs",
           "arms": {"grouped": "HybridEnsemble of all models: one call (one launch at nx 64)",
                    "loop": "one HybridSolver call per model",
                    "scored": "compare_batch: classical twin, mse, metrics, metrics_classical",
                    "unscored": "run_batch(traj=False, metrics=True)"},
           "note": "alternating windows, same GPU, same process; medians with min..max; ratios window by window; no "
                   "ratio was fixed in advance",
           "sweep": sweep, "m1_at_cfg3": m1, "bench_py_headline": bench_pair(args)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
