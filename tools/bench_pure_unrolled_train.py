"""Time of one unrolled training step of PureGNN (through K rollout steps).

One "step" = one optimizer step on a batch of B windows of K + 1 classical
states of 64 cells: K taped PureGNN forwards and residual updates, the K-step
state loss, K adjoint / backward pairs, Adam.  PureGNN(4, 128, 4), default
B = 2000, K = 4.  The windows are classical rollouts of seeded ICs.

  engine    hybridflux.training.pure_unrolled_step: hf_pure_gnn_forward_train +
            hf_pure_unroll_update per forward step, hf_pure_unroll_adjoint +
            hf_pure_gnn_backward per backward step, FlatAdam
  baseline  the same step composed from what the package had before the
            entry points: PureGNN under autograd (its HIP training kernels),
            torch permute / cat / add for the rollout's glue
            (evaluate_multi_ic.py:53-64), torch's MSE, FlatAdam.  It uses none
            of the new entry points, so it runs unchanged on an older checkout
            (there the engine column is "not measured").

Both run in the same process, alternating, `--repeats` windows of `--steps`
steps each after a warm-up of both; a window is a host clock around steps that
end in a device synchronise.  Reported: the median window's ms/step and
samples/s (windows per second), the min..max spread, kernel launches per step
(counted by torch.profiler on one step; "not measured" if it cannot), the
ratio to the baseline, and the engine's fraction of the fp32 MFMA peak under
training.pure_unrolled_train_flop_per_sample: a whole-step rate over peak, not
a kernel's share.  Prints one JSON line and writes it to --out.

    python tools/bench_pure_unrolled_train.py [--batch 2000] [--K 4] [--steps 10] [--repeats 7] [--out FILE]
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

PEAK_TFLOPS = 157.3  # fp32 MFMA peak of the MI355X (as tools/bench_train.py)


def fresh_model(hf):
    from hybridflux.training import FlatAdam
    torch.manual_seed(0)
    m = hf.PureGNN(4, 128, 4).to("cuda").flatten_parameters_()
    return m, FlatAdam(m.parameters(), lr=1e-4)


def make_engine(hf, traj, x):
    from hybridflux import training
    if not hasattr(training, "pure_unrolled_step"):
        return None
    m, opt = fresh_model(hf)

    def step():
        loss = training.pure_unrolled_step(m, opt, traj, x)
        assert loss is not None
        return loss
    return step


def make_baseline(hf, traj, x):
    """The K-step loss from PureGNN's autograd Function and torch ops."""
    from hybridflux.graph_constructor import shared_chain_edge_index
    m, opt = fresh_model(hf)
    B, K1, _, nx = traj.shape
    ei = shared_chain_edge_index(nx, B, traj.device)
    xc = x.repeat(B).unsqueeze(1)

    def step():
        st, loss = traj[:, 0], 0.0
        for j in range(1, K1):
            nf = torch.cat([st.permute(0, 2, 1).reshape(B * nx, 3), xc], dim=1)
            st = st + m(nf, ei).view(B, nx, 3).permute(0, 2, 1)
            loss = loss + torch.mean((st - traj[:, j]) ** 2) / (K1 - 1)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.detach()
    return step


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pure_unrolled_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pure_unrolled_train: no HIP device visible (this benchmark has no CPU path)")
    if args.repeats < 5:
        raise SystemExit("bench_pure_unrolled_train: at least 5 repeats (the spread is part of the result)")
    import hybridflux as hf
    from hybridflux import training
    from hybridflux._lib import version
    nx, B, K = 64, args.batch, args.K
    solver = hf.BaselineSolver(nx, device="cuda")
    x, _ = solver.grid.on(torch.device("cuda", torch.cuda.current_device()))
    ics = solver.initial_conditions(list(range(B)), as_tensor=True)
    traj = solver.run_batch(ics, K, traj=True)["traj"].contiguous()  # [B,K+1,3,nx]
    runs = {"engine": make_engine(hf, traj, x), "baseline": make_baseline(hf, traj, x)}
    runs = {k: v for k, v in runs.items() if v is not None}
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
    for k, v in ms.items():
        med = statistics.median(v)
        res[k] = {"ms_per_step": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                  "samples_per_s": round(B / med * 1e3, 1), "launches_per_step": launches(runs[k])}
    if "engine" in res:
        fps = training.pure_unrolled_train_flop_per_sample(K, nx, 128, 4, 4)
        tf = res["engine"]["samples_per_s"] * fps / 1e12
        res["engine"]["tflops_whole_step"] = round(tf, 3)
        res["engine"]["frac_of_fp32_mfma_peak_whole_step"] = round(tf / PEAK_TFLOPS, 5)
        res["baseline_over_engine"] = round(res["baseline"]["ms_per_step"] / res["engine"]["ms_per_step"], 3)
        ratios = [b / e for b, e in zip(ms["baseline"], ms["engine"])]  # window by window, as they alternated
        res["baseline_over_engine_min"] = round(min(ratios), 3)
        res["baseline_over_engine_max"] = round(max(ratios), 3)
    else:
        fps = "not measured"
        res["engine"] = "not measured"
    line = json.dumps({"metric": "PureGNN unrolled training step (K forwards + updates, K-step loss, K adjoints + "
                                 "backwards, Adam)",
                       "model": "PureGNN(4,128,4) f32", "batch": B, "K": K, "cells": nx,
                       "steps_per_window": args.steps, "windows": args.repeats, "flop_per_sample": fps,
                       "peak_tflops": PEAK_TFLOPS,
                       "note": "whole optimizer step over peak (end to end, not a kernel's share); baseline = PureGNN "
                               "autograd + torch permute / cat / add / MSE + FlatAdam on the same GPU in the same run; "
                               "a sample is one K-step window",
                       "lib": version(), "result": res})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
