"""Cost of the seeded Gaussian state noise of training (hf_state_noise), in one
run on one GPU.

  call   engine.state_noise on B x 64 states, B = 2000 and 4096: sigma = (1e-2,
         1e-2, 0) with zero mean, once plain (one launch) and once as the
         trainers use it on FluxGNN (E recomputed on the grid: three launches);
         device seeds, so a call has no upload.  Windows of `--calls` calls
         ending in a device synchronise.
  step   the K = 4 unrolled training step of each model on B = 2000 windows,
         batch included (WindowDataset.batch, then the *_unrolled_step), with
         noise= off and on, and a twin of the off step on objects of its own;
         the three alternate window by window.  FluxGNN's noise recomputes E on
         the step's grid; PureGNN's and PINN's carry sigma_E = 5e-3 instead.

Reported: the median window's ms, min..max, on over off window by window, and
the off step's own spread (max / min over its windows), beside which a
difference means something or does not.  Prints one JSON line and writes it to
--out.

    python tools/bench_state_noise.py [--repeats 7] [--steps 10] [--calls 50] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnn-plasma-flux_amd"))
sys.path.insert(0, ROOT)

NX = 64
CALL_BATCHES = (2000, 4096)
SIGMA = (1e-2, 1e-2, 0.0)


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def spread(v):
    return {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def bench_calls(solver, args):
    from hybridflux import engine
    res = {}
    for B in CALL_BATCHES:
        st = solver.initial_conditions(list(range(B)), as_tensor=True)
        seeds = torch.arange(1000, 1000 + B, dtype=torch.int64, device=st.device)
        out = torch.empty_like(st)
        runs = {"plain": lambda: engine.state_noise(st, seeds, SIGMA, out=out),
                "with_poisson": lambda: engine.state_noise(st, seeds, SIGMA, grid=solver.grid, out=out)}
        for fn in runs.values():
            window(fn, args.calls)
        ms = {k: [] for k in runs}
        for _ in range(args.repeats):
            for k, fn in runs.items():
                ms[k].append(window(fn, args.calls))
        res[f"B{B}_nx{NX}"] = {k: dict(spread(v), us_per_state=round(statistics.median(v) / B * 1e3, 4))
                               for k, v in ms.items()}
    return res


def make_steps(hf, data, idx, seeds, x, grid):
    """{model: {"off": step, "on": step, "twin": step}}, every step on a model and optimizer of its own."""
    from hybridflux import training
    calls = {
        "FluxGNN(4,128,4)": (lambda m, opt, w: training.unrolled_step(m, opt, w, x, grid), hf.FluxGNN, (4, 128, 4),
                             training.StateNoise(SIGMA[0], SIGMA[1], grid=grid)),
        "PureGNN(4,128,4)": (lambda m, opt, w: training.pure_unrolled_step(m, opt, w, x), hf.PureGNN, (4, 128, 4),
                             training.StateNoise(SIGMA[0], SIGMA[1], 5e-3)),
        "PINN(192,256,4)": (lambda m, opt, w: training.pinn_unrolled_step(m, opt, w), hf.PINN, (3 * NX, 256, 4),
                            training.StateNoise(SIGMA[0], SIGMA[1], 5e-3)),
    }

    def one(call, cls, dims, noise):
        torch.manual_seed(0)
        m = cls(*dims).to("cuda").flatten_parameters_()
        opt = training.FlatAdam(m.parameters(), lr=1e-4)

        def step():
            win = data.batch(idx) if noise is None else data.batch(idx, noise, seeds)
            loss = call(m, opt, win)
            assert loss is not None
            return loss
        return step
    return {name: {"off": one(call, cls, dims, None), "on": one(call, cls, dims, noise),
                   "twin": one(call, cls, dims, None)}
            for name, (call, cls, dims, noise) in calls.items()}


def bench_steps(hf, solver, args):
    from hybridflux import training
    B, K = args.batch, args.K
    grid = solver.grid
    dev = torch.device("cuda", torch.cuda.current_device())
    x, _ = grid.on(dev)
    ics = solver.initial_conditions(list(range(B)), as_tensor=True)
    traj = solver.run_batch(ics, K, traj=True)["traj"].contiguous()  # [B,K+1,3,nx]: one window per IC
    data = training.WindowDataset(traj, K, dev)
    idx = torch.arange(B, device=dev)
    seeds = torch.arange(1000, 1000 + B, dtype=torch.int64, device=dev)
    models = make_steps(hf, data, idx, seeds, x, grid)
    runs = {(name, mode): step for name, trio in models.items() for mode, step in trio.items()}
    for step in runs.values():
        window(step, args.warmup)
    t_end = time.perf_counter() + 0.3  # back-to-back load before timing: the clock ramps under load
    while time.perf_counter() < t_end:
        for step in runs.values():
            window(step, args.steps)
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):  # alternating windows
        for k, step in runs.items():
            ms[k].append(window(step, args.steps))
    res = {}
    for name in models:
        off, on, twin = ms[(name, "off")], ms[(name, "on")], ms[(name, "twin")]
        ratios = [b / a for a, b in zip(off, on)]
        twins = [b / a for a, b in zip(off, twin)]
        own = max(off) / min(off)
        med = statistics.median(on) / statistics.median(off)
        res[name] = {
            "off": spread(off), "on": spread(on), "twin": spread(twin),
            "on_over_off": {"median": round(med, 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
            "twin_over_off": {"median": round(statistics.median(twin) / statistics.median(off), 4),
                              "min": round(min(twins), 4), "max": round(max(twins), 4)},
            "off_window_spread_max_over_min": round(own, 4),
            "on_over_off_outside_spread": bool(med > own or med < 1.0 / own),
        }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_noise_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_state_noise: no HIP device visible (this benchmark has no CPU path)")
    if args.repeats < 5:
        raise SystemExit("bench_state_noise: at least 5 repeats (the spread is part of the result)")
    import hybridflux as hf
    from hybridflux._lib import version
    solver = hf.BaselineSolver(NX, device="cuda")
    line = json.dumps({"metric": "seeded Gaussian state noise: the call, and the K-step training step with noise off / on",
                       "cells": NX, "sigma": list(SIGMA), "zero_mean": True, "K": args.K, "step_batch": args.batch,
                       "calls_per_window": args.calls, "steps_per_window": args.steps, "windows": args.repeats,
                       "note": "call: engine.state_noise with device seeds into a preallocated output, plain (1 "
                               "launch) and with E recomputed (3 launches); step: WindowDataset.batch + the "
                               "*_unrolled_step, off = noise=None, on = noise= (two copies and the call's launches "
                               "more), twin = a second off step on objects of its own; all alternate window by "
                               "window in one run on the same GPU; a window is a host clock around work ending in "
                               "a device synchronise; the spread is the off step's max / min over its windows",
                       "lib": version(), "call": bench_calls(solver, args), "step": bench_steps(hf, solver, args)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
