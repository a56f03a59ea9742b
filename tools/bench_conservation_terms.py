"""What the energy and charge terms cost the three unrolled training steps.

One "step" = one optimizer step on a batch of B windows of K + 1 classical
states of 64 cells (default B = 2000, K = 4), as tools/bench_unrolled_train.py,
bench_pure_unrolled_train.py and bench_pinn_unrolled_train.py time it:
FluxGNN(4, 128, 4) through the hybrid solver, PureGNN(4, 128, 4) and
PINN(192, 256, 4, state loss) through their own rollouts.  Each step runs three
times in the same process, alternating window by window:

  off  the step as it was: conservation=None
  twin a second `off` step on a model, optimizer and buffers of its own: what two
       step objects that do the same work differ by, the floor of this comparison
  on   conservation=(1, 1), conservation_ref="start": the same launches (the
       _ex kernels: three float64 sums per cell in the forward, one float32
       multiply-add per value in the adjoint) plus one hf_state_moments launch
       per training step

`--repeats` windows of `--steps` steps each after a warm-up of all nine; a window
is a host clock around steps that end in a device synchronise.  The yardstick is
the same step without the terms in the same run.  Reported per model: the median
window's ms/step off and on with their min..max, the on/off ratio window by
window (median, min, max), the same for twin/off, the run's own window-to-window
spread of the off step (max / min), whether the median ratio falls outside that
spread, and the device launches per step, off and on (torch.profiler on one
step; "not measured" if it cannot).  Prints one JSON line and writes it to --out.

    python tools/bench_conservation_terms.py [--batch 2000] [--K 4] [--steps 10] [--repeats 7] [--out FILE]
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

LAM = (1.0, 1.0)


def make_steps(hf, traj, x, grid):
    """{model: {"off": step, "on": step, "twin": step}}, every step on a model and optimizer of its own."""
    from hybridflux import training
    from hybridflux.training import FlatAdam

    def fresh(cls, *dims):
        torch.manual_seed(0)
        m = cls(*dims).to("cuda").flatten_parameters_()
        return m, FlatAdam(m.parameters(), lr=1e-4)

    def one(call, cls, dims, kw):
        m, opt = fresh(cls, *dims)

        def step():
            loss = call(m, opt, **kw)
            assert loss is not None
            return loss
        return step

    calls = {
        "FluxGNN(4,128,4)": (lambda m, opt, **kw: training.unrolled_step(m, opt, traj, x, grid, **kw), hf.FluxGNN,
                             (4, 128, 4)),
        "PureGNN(4,128,4)": (lambda m, opt, **kw: training.pure_unrolled_step(m, opt, traj, x, **kw), hf.PureGNN,
                             (4, 128, 4)),
        "PINN(192,256,4)": (lambda m, opt, **kw: training.pinn_unrolled_step(m, opt, traj, **kw), hf.PINN,
                            (3 * traj.shape[-1], 256, 4)),
    }
    on = dict(conservation=LAM, conservation_ref="start")
    return {name: {"off": one(call, cls, dims, {}), "on": one(call, cls, dims, on), "twin": one(call, cls, dims, {})}
            for name, (call, cls, dims) in calls.items()}


def window(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def launches(step):
    """Device kernels (and memsets / copies) of one step, by torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n if n > 0 else "not measured"
    except Exception:  # a profiler that cannot attach must not cost the timing run
        return "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conservation_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conservation_terms: no HIP device visible (this benchmark has no CPU path)")
    if args.repeats < 5:
        raise SystemExit("bench_conservation_terms: at least 5 repeats (the spread is part of the result)")
    import hybridflux as hf
    from hybridflux._lib import version
    nx, B, K = 64, args.batch, args.K
    solver = hf.BaselineSolver(nx, device="cuda")
    grid = solver.grid
    x, _ = grid.on(torch.device("cuda", torch.cuda.current_device()))
    ics = solver.initial_conditions(list(range(B)), as_tensor=True)
    traj = solver.run_batch(ics, K, traj=True)["traj"].contiguous()  # [B,K+1,3,nx]
    models = make_steps(hf, traj, x, grid)
    runs = {(name, mode): step for name, pair in models.items() for mode, step in pair.items()}
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
        ratios = [b / a for a, b in zip(off, on)]  # window by window, as they alternated
        twins = [b / a for a, b in zip(off, twin)]
        spread = max(off) / min(off)
        med = statistics.median(on) / statistics.median(off)
        res[name] = {
            "off_ms_per_step": round(statistics.median(off), 4), "off_ms_min": round(min(off), 4),
            "off_ms_max": round(max(off), 4),
            "on_ms_per_step": round(statistics.median(on), 4), "on_ms_min": round(min(on), 4),
            "on_ms_max": round(max(on), 4),
            "on_over_off": {"median": round(med, 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
            "twin_ms_per_step": round(statistics.median(twin), 4),
            "twin_over_off": {"median": round(statistics.median(twin) / statistics.median(off), 4),
                              "min": round(min(twins), 4), "max": round(max(twins), 4)},
            "off_window_spread_max_over_min": round(spread, 4),
            "on_over_off_outside_spread": bool(med > spread or med < 1.0 / spread),
            "launches_per_step_off": launches(runs[(name, "off")]),
            "launches_per_step_on": launches(runs[(name, "on")]),
        }
    line = json.dumps({"metric": "unrolled training step with and without the energy and charge terms",
                       "batch": B, "K": K, "cells": nx, "conservation": list(LAM), "conservation_ref": "start",
                       "steps_per_window": args.steps, "windows": args.repeats,
                       "note": "off = conservation=None, on = the terms inside the same launches + one "
                               "hf_state_moments launch per training step, twin = a second off step on objects of "
                               "its own; all alternate window by window in one "
                               "run on the same GPU; a window is a host clock around steps ending in a device "
                               "synchronise; the spread is the off step's max / min over its windows",
                       "lib": version(), "result": res})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
