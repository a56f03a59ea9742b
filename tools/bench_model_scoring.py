"""Cost of scoring the comparison models' rollouts inside their one-launch kernels.

PureGNN(4,128,4) and PINN(192,256,4) (weights: tests/golden/baselines.npz),
4096 ICs x 64 cells, T = 30 and T = 1000 steps.  Four arms, in alternating
windows on the same GPU in the same run (a window = one rollout call between
device synchronisations, host clock):

  a  plain      model.rollout(traj=False): the unscored one-launch rollout
  b  metrics    the scored rollout, metric series only (no classical twin)
  c  twin       the scored rollout with the classical twin: metrics, mse,
                metrics_classical (what evaluation.multi_ic_mse asks for)
  d  recorded   the same three series from recorded trajectories, as the
                package composed them before the scored rollouts: the model's
                rollout recording its trajectory, BaselineSolver.run_batch
                recording its own (with its metrics), engine.traj_metrics on the
                model's, engine.traj_mse on the pair

Reported per model and T: the median window's ms, the min..max spread, and the
ratios b/a, c/a and d/c (medians; min..max of the window-by-window ratios).
No speed is a target here: the record states what was measured.

Each (model, T) runs in a child process of its own under a time limit; after a
child that fails or runs out of time no further child is started.  Prints one
JSON line and writes it to --out.

    python tools/bench_model_scoring.py [--ics 4096] [--steps 30 1000] [--repeats 7] [--out FILE]
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

ARMS = ("plain", "metrics", "twin", "recorded")
RATIOS = (("metrics_over_plain", "metrics", "plain"), ("twin_over_plain", "twin", "plain"),
          ("recorded_over_twin", "recorded", "twin"))


def child(model_name, B, T, repeats):
    import numpy as np
    import torch

    import hybridflux as hf
    from hybridflux import engine
    from hybridflux._lib import version
    dev = torch.device("cuda", 0)
    b = np.load(os.path.join(ROOT, "tests", "golden", "baselines.npz"))
    base = hf.BaselineSolver(64, device=dev)
    ics = base.initial_conditions(range(1000, 1000 + B), as_tensor=True)
    if model_name == "pure_gnn":
        m = hf.PureGNN(4, 128, 4)
        m.load_state_dict({k[9:]: torch.from_numpy(b[k]) for k in b.files if k.startswith("pure_gnn.")})
        m = m.to(dev)
        roll = lambda **kw: m.rollout(ics, T, base.x, **kw)  # noqa: E731
    else:
        m = hf.PINN(3 * 64, 256, 4)
        m.load_state_dict({k[5:]: torch.from_numpy(b[k]) for k in b.files if k.startswith("pinn.")})
        m = m.to(dev)
        roll = lambda **kw: m.rollout(ics, T, **kw)  # noqa: E731

    def recorded():
        tr = roll(traj=True)["traj"]
        cl = base.run_batch(ics, T, traj=True, metrics=True)
        return engine.traj_metrics(tr), engine.traj_mse(tr, cl["traj"]), cl["metrics"]

    arms = {"plain": lambda: roll(traj=False), "metrics": lambda: roll(traj=False, metrics=True),
            "twin": lambda: roll(traj=False, metrics=True, compare=base), "recorded": recorded}

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    for fn in arms.values():  # warm-up of every arm (allocations, first launches)
        window(fn)
    t_end = time.perf_counter() + 0.3  # back-to-back load before timing: the clock ramps under load
    while time.perf_counter() < t_end:
        for fn in arms.values():
            window(fn)
    ms = {k: [] for k in arms}
    for _ in range(repeats):  # alternating windows
        for k, fn in arms.items():
            ms[k].append(window(fn))
    # the arms computed the same series (bit for bit; tests/test_gpu_model_scoring.py gates it)
    tw, rec = arms["twin"](), recorded()
    same = all(torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
               for x, y in zip((tw["metrics"], tw["mse"], tw["metrics_classical"]), rec))
    res = {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
               "ic_steps_per_s": round(B * T / statistics.median(v) * 1e3, 1)} for k, v in ms.items()}
    for name, num, den in RATIOS:
        r = [x / y for x, y in zip(ms[num], ms[den])]  # window by window, as they alternated
        res[name] = {"median": round(res[num]["ms"] / res[den]["ms"], 4), "min": round(min(r), 4),
                     "max": round(max(r), 4)}
    res["series_equal_to_recorded"] = bool(same)
    print("RESULT " + json.dumps({"model": model_name, "ics": B, "cells": 64, "steps": T, "windows": repeats,
                                  "lib": version(), "result": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ics", type=int, default=4096)
    ap.add_argument("--steps", type=int, nargs="+", default=[30, 1000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per (model, T) child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_scoring_bench.json"))
    ap.add_argument("--child", nargs=2, metavar=("MODEL", "T"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("bench_model_scoring: at least 5 repeats (the spread is part of the result)")
    if args.child:
        child(args.child[0], args.ics, int(args.child[1]), args.repeats)
        return
    runs = []
    for model in ("pure_gnn", "pinn"):
        for T in args.steps:
            cmd = [sys.executable, os.path.abspath(__file__), "--ics", str(args.ics), "--repeats", str(args.repeats),
                   "--child", model, str(T)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"bench_model_scoring: {model} T={T} ran past {args.timeout} s; stopping")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"bench_model_scoring: {model} T={T} failed (exit {p.returncode}); stopping")
            runs.append(json.loads(line[-1][7:]))
    out = {"metric": "rollout scoring of the comparison models: ms per rollout call of all ICs",
           "arms": {"plain": "unscored one-launch rollout, traj=False",
                    "metrics": "scored rollout, metric series only",
                    "twin": "scored rollout with the classical twin: metrics, mse, metrics_classical",
                    "recorded": "model rollout recording its trajectory + BaselineSolver.run_batch recording its own "
                                "+ traj_metrics + traj_mse"},
           "note": "alternating windows of one rollout call each, same GPU, same run; medians with min..max; ratios "
                   "window by window; no speed was fixed in advance",
           "runs": runs}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
