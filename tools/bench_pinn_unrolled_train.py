"""Time of one unrolled training step of PINN (through K rollout steps).

One "step" = one optimizer step on a batch of B windows of K + 1 classical
states of 64 cells: K taped PINN forwards, the K-step loss, K adjoint / backward
pairs, Adam.  PINN(192, 256, 4), default B = 2000, K = 4.  The windows are
classical rollouts of seeded ICs.  Two losses: the state loss alone (lambda = 0)
and with the reference's residual weights (0.1, 0.1, 0.01).

  engine    hybridflux.training.pinn_unrolled_step: hf_pinn_forward_train +
            hf_pinn_unroll_loss per forward step, hf_pinn_unroll_adjoint +
            hf_pinn_backward per backward step, FlatAdam
  baseline  the same step composed from training.pinn_forward (the same HIP
            forward / backward kernels under autograd), torch ops for the loss
            (torch.roll and a dense circulant for the residuals), autograd,
            FlatAdam.

All four run in the same process, alternating, `--repeats` windows of `--steps`
steps each after a warm-up of all; a window is a host clock around steps that
end in a device synchronise.  Reported per loss: the median window's ms/step
and samples/s (windows per second), the min..max spread, kernel launches per
step (counted by torch.profiler on one step; "not measured" if it cannot), the
ratio to the baseline window by window, and the engine's fraction of the fp32
MFMA peak under training.pinn_unrolled_train_flop_per_sample: a whole-step rate
over peak, not a kernel's share.  Prints one JSON line and writes it to --out.

    python tools/bench_pinn_unrolled_train.py [--batch 2000] [--K 4] [--steps 10] [--repeats 7] [--out FILE]
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
REF_LAMBDA = (0.1, 0.1, 0.01)
DIMS = (192, 256, 4)


def fresh_model(hf):
    from hybridflux.training import FlatAdam
    torch.manual_seed(0)
    m = hf.PINN(*DIMS).to("cuda").flatten_parameters_()
    return m, FlatAdam(m.parameters(), lr=1e-4)


def make_engine(hf, traj, lam, dx, dt, nu):
    from hybridflux import training
    m, opt = fresh_model(hf)
    kw = {} if lam is None else dict(dx=dx, dt=dt, nu=nu, physics_weights=lam)

    def step():
        loss = training.pinn_unrolled_step(m, opt, traj, **kw)
        assert loss is not None
        return loss
    return step


def make_baseline(hf, traj, lam, dx, dt, nu):
    """The K-step loss from training.pinn_forward and torch ops."""
    from hybridflux import engine, training
    m, opt = fresh_model(hf)
    B, K1, _, nx = traj.shape
    K = K1 - 1
    if lam is not None:
        i = torch.arange(nx, device=traj.device)
        Pm = engine.pinn_loss_plan(nx, nx * dx, traj.device)[:nx][(i[:, None] - i[None, :]) % nx].float()
        keep = torch.ones(nx, device=traj.device)
        keep[0] = 0.0
    up, dn = (lambda f: torch.roll(f, -1, -1)), (lambda f: torch.roll(f, 1, -1))

    def step():
        st, loss = traj[:, 0], 0.0
        for j in range(1, K1):
            p = training.pinn_forward(m, st)
            loss = loss + torch.mean((p - traj[:, j]) ** 2) / K
            if lam is not None:
                n, u, E = st[:, 0], st[:, 1], st[:, 2]
                r_c = (p[:, 0] - n) / dt + (up(n * u) - dn(n * u)) / (2 * dx)
                r_m = (p[:, 1] - u) / dt + u * (up(u) - dn(u)) / (2 * dx) + E - nu * (up(u) - 2 * u + dn(u)) / dx ** 2
                r_p = p[:, 2] + (p[:, 0] @ Pm.T) * keep
                loss = loss + (lam[0] * torch.mean(r_c ** 2) + lam[1] * torch.mean(r_m ** 2)
                               + lam[2] * torch.mean(r_p ** 2)) / K
            st = p
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pinn_unrolled_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pinn_unrolled_train: no HIP device visible (this benchmark has no CPU path)")
    if args.repeats < 5:
        raise SystemExit("bench_pinn_unrolled_train: at least 5 repeats (the spread is part of the result)")
    import hybridflux as hf
    from hybridflux import training
    from hybridflux._lib import version
    nx, B, K = DIMS[0] // 3, args.batch, args.K
    solver = hf.BaselineSolver(nx, device="cuda")
    dx, dt, nu = solver.dx, solver.dt, solver.nu
    ics = solver.initial_conditions(list(range(B)), as_tensor=True)
    traj = solver.run_batch(ics, K, traj=True)["traj"].contiguous()  # [B,K+1,3,nx]
    runs = {}
    for tag, lam in (("state", None), ("physics", REF_LAMBDA)):
        runs[f"engine_{tag}"] = make_engine(hf, traj, lam, dx, dt, nu)
        runs[f"baseline_{tag}"] = make_baseline(hf, traj, lam, dx, dt, nu)
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
    fps = training.pinn_unrolled_train_flop_per_sample(K, *DIMS)
    res = {}
    for k, v in ms.items():
        med = statistics.median(v)
        res[k] = {"ms_per_step": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                  "samples_per_s": round(B / med * 1e3, 1), "launches_per_step": launches(runs[k])}
    for tag in ("state", "physics"):
        e, b = f"engine_{tag}", f"baseline_{tag}"
        tf = res[e]["samples_per_s"] * fps / 1e12
        res[e]["tflops_whole_step"] = round(tf, 3)
        res[e]["frac_of_fp32_mfma_peak_whole_step"] = round(tf / PEAK_TFLOPS, 5)
        ratios = [x / y for x, y in zip(ms[b], ms[e])]  # window by window, as they alternated
        res[f"baseline_over_engine_{tag}"] = {"median": round(res[b]["ms_per_step"] / res[e]["ms_per_step"], 3),
                                              "min": round(min(ratios), 3), "max": round(max(ratios), 3)}
    line = json.dumps({"metric": "PINN unrolled training step (K forwards, K-step loss, K adjoints + backwards, Adam)",
                       "model": "PINN(192,256,4) f32", "batch": B, "K": K, "cells": nx,
                       "physics_weights": list(REF_LAMBDA), "steps_per_window": args.steps, "windows": args.repeats,
                       "flop_per_sample": fps, "peak_tflops": PEAK_TFLOPS,
                       "note": "whole optimizer step over peak (end to end, not a kernel's share); state = the state "
                               "loss alone, physics = with the residual terms; baseline = training.pinn_forward "
                               "under autograd + torch ops for the loss + FlatAdam on the same GPU in the same run; "
                               "a sample is one K-step window",
                       "lib": version(), "result": res})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
