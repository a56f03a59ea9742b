"""Time of one unrolled training step (FluxGNN through K hybrid solver steps).

One "step" = one optimizer step on a batch of B windows of K + 1 classical
states of 64 cells: K taped FluxGNN forwards and hybrid updates, the K-step
state loss, K adjoint / backward pairs, Adam.  FluxGNN(4, 128, 4), default
B = 2000, K = 4.  The windows are classical rollouts of seeded ICs.

  engine    hybridflux.training.unrolled_step: hf_graph_forward_train +
            hf_unroll_update per forward step, hf_unroll_adjoint +
            hf_graph_backward per backward step, FlatAdam
  baseline  the same step composed from what the package had before the
            unrolled entry points: FluxGNN under autograd (its HIP training
            kernels), torch ops for the update (torch.roll), torch.fft for a
            differentiable Poisson solve, torch's MSE, FlatAdam.  It uses no
            unrolled entry point, so it runs unchanged on an older checkout
            (there the engine column is "not measured").

Both run in the same process, alternating, `--repeats` windows of `--steps`
steps each after a warm-up of both; a window is a host clock around steps that
end in a device synchronise.  Reported: the median window's ms/step and
samples/s (windows per second), the min..max spread, kernel launches per step
(counted by torch.profiler on one step; "not measured" if it cannot), the
ratio to the baseline, and the engine's fraction of the fp32 MFMA peak under
training.unrolled_train_flop_per_sample: a whole-step rate over peak, not a
kernel's share.  Prints one JSON line and writes it to --out.

    python tools/bench_unrolled_train.py [--batch 2000] [--K 4] [--steps 10] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnn-plasma-flux_amd"))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3  # fp32 MFMA peak of the MI355X (as tools/bench_train.py)


def fresh_model(hf):
    from hybridflux.training import FlatAdam
    torch.manual_seed(0)
    m = hf.FluxGNN(4, 128, 4).to("cuda").flatten_parameters_()
    return m, FlatAdam(m.parameters(), lr=1e-4)


def make_engine(hf, traj, x, grid):
    from hybridflux import training
    if not hasattr(training, "unrolled_step"):
        return None
    m, opt = fresh_model(hf)

    def step():
        loss = training.unrolled_step(m, opt, traj, x, grid)
        assert loss is not None
        return loss
    return step


def make_baseline(hf, traj, x, grid):
    """The K-step loss from FluxGNN's autograd Function and torch ops."""
    from hybridflux.graph_constructor import shared_chain_edge_index
    m, opt = fresh_model(hf)
    B, K1, _, nx = traj.shape
    c, dt = grid.c32, grid.dt32
    k = torch.as_tensor(2.0 * np.pi * np.fft.fftfreq(nx, d=grid.dx), dtype=torch.float32, device="cuda")
    ik = torch.where(k != 0, 1.0 / torch.where(k != 0, k, torch.ones_like(k)), torch.zeros_like(k))
    ei = shared_chain_edge_index(nx, B, traj.device)
    xb = x.expand(B, nx)

    def step():
        st, loss = traj[:, 0], 0.0
        for j in range(1, K1):
            nf = torch.stack([st[:, 0], st[:, 1], st[:, 2], xb], dim=-1).reshape(B * nx, 4)
            fe = m(nf, ei).reshape(B, 2 * nx)
            F = 0.5 * (fe[:, :nx] + fe[:, nx:])
            n, u, E = st[:, 0], st[:, 1], st[:, 2]
            n1 = n - c * (F - torch.roll(F, 1, -1))
            Fu = 0.5 * u * u
            u1 = u - c * (Fu - torch.roll(Fu, 1, -1)) + dt * E
            E1 = torch.fft.ifft(1j * torch.fft.fft(n1 - 1.0, dim=-1) * ik, dim=-1).real
            st = torch.stack([n1, u1, E1], dim=1)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unrolled_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unrolled_train: no HIP device visible (this benchmark has no CPU path)")
    if args.repeats < 5:
        raise SystemExit("bench_unrolled_train: at least 5 repeats (the spread is part of the result)")
    import hybridflux as hf
    from hybridflux import training
    from hybridflux._lib import version
    nx, B, K = 64, args.batch, args.K
    solver = hf.BaselineSolver(nx, device="cuda")
    grid = solver.grid
    x, _ = grid.on(torch.device("cuda", torch.cuda.current_device()))
    ics = solver.initial_conditions(list(range(B)), as_tensor=True)
    traj = solver.run_batch(ics, K, traj=True)["traj"].contiguous()  # [B,K+1,3,nx]
    runs = {"engine": make_engine(hf, traj, x, grid), "baseline": make_baseline(hf, traj, x, grid)}
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
        fps = training.unrolled_train_flop_per_sample(K, nx, 128, 4, 4)
        tf = res["engine"]["samples_per_s"] * fps / 1e12
        res["engine"]["tflops_whole_step"] = round(tf, 3)
        res["engine"]["frac_of_fp32_mfma_peak_whole_step"] = round(tf / PEAK_TFLOPS, 5)
        res["baseline_over_engine"] = round(res["baseline"]["ms_per_step"] / res["engine"]["ms_per_step"], 3)
    else:
        fps = "not measured"
        res["engine"] = "not measured"
    line = json.dumps({"metric": "unrolled training step (K forwards + updates, K-step loss, K adjoints + backwards, Adam)",
                       "model": "FluxGNN(4,128,4) f32", "batch": B, "K": K, "cells": nx,
                       "steps_per_window": args.steps, "windows": args.repeats, "flop_per_sample": fps,
                       "peak_tflops": PEAK_TFLOPS,
                       "note": "whole optimizer step over peak (end to end, not a kernel's share); baseline = FluxGNN "
                               "autograd + torch.roll / torch.fft update + FlatAdam on the same GPU in the same run; "
                               "a sample is one K-step window",
                       "lib": version(), "result": res})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
