"""Training-step time of PureGNN on the engine against the batched ATen restatement.

One "step" = one optimizer step of scripts/training/train_pure_gnn.py's loop
(:112-145) on a batch of B samples of 64 cells: forward, the state-MSE loss,
backward, Adam.  PureGNN(4, 128, 4) (MODEL_CONFIG's width, :94-98), at B = 32
(the reference's batch) and B = 2000.  Synthetic states (seeded normal; the
time does not depend on the values).

  engine  hybridflux.training.pure_gnn_step: the HIP training forward /
          backward (hf_pure_gnn_forward_train / hf_pure_gnn_backward), the
          fused loss (hf_state_mse) and FlatAdam (hf_adam_flat)
  aten    what a user would otherwise run on the same GPU: the oracle-style
          torch forward on the device over the same batched chain graph, torch
          autograd and torch.optim.Adam.  The comparison, not the code under test.

Both run in the same process, alternating, `--repeats` windows of `--steps`
steps each after a warm-up of both; a window is a host clock around steps
that end in a device synchronise.  Reported per batch: the median window's
ms/step and samples/s, the min..max spread, and the engine's fraction of the
fp32 MFMA peak under the algorithmic FLOP model
(training.pure_gnn_train_flop_per_sample: a whole-step rate over peak, not a
kernel's share).  Prints one JSON line; --out also writes it to a file.

    python tools/bench_pure_gnn_train.py [--batches 32,2000] [--steps 20] [--repeats 7] [--out FILE]
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


def make_engine(hf, B, nx, st, sn, x):
    from hybridflux.training import FlatAdam, pure_gnn_step
    torch.manual_seed(0)
    m = hf.PureGNN(4, 128, 4).to("cuda").flatten_parameters_()
    opt = FlatAdam(m.parameters(), lr=1e-3)
    return lambda: pure_gnn_step(m, opt, st, sn, x)


def make_aten(hf, B, nx, st, sn, x):
    from oracle import hybrid_oracle as O
    from hybridflux.training import pure_gnn_features
    torch.manual_seed(0)
    ref = hf.PureGNN(4, 128, 4)
    p = {k: v.detach().clone().to("cuda").requires_grad_(True) for k, v in ref.state_dict().items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    ei = O.chain_edges(nx, B).to("cuda")
    tgt = sn.permute(0, 2, 1).reshape(-1, 3)

    def step():
        nf = pure_gnn_features(st, x)
        loss = ((nf[:, :3] + O.pure_gnn_forward(p, nf, ei) - tgt) ** 2).mean()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,2000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pure_gnn_train: no HIP device visible (this benchmark has no CPU path)")
    import hybridflux as hf
    from hybridflux._lib import version
    from hybridflux.training import pure_gnn_train_flop_per_sample
    nx = 64
    fps = pure_gnn_train_flop_per_sample(nx, 128, 4, 4)
    x = torch.linspace(0, 2 * np.pi, nx + 1, device="cuda")[:-1].contiguous()
    res = {}
    for B in [int(v) for v in args.batches.split(",") if v]:
        g = torch.Generator().manual_seed(B)
        st = torch.randn(B, 3, nx, generator=g).to("cuda")
        sn = (st + 0.01 * torch.randn(B, 3, nx, generator=g).to("cuda")).contiguous()
        runs = {"engine": make_engine(hf, B, nx, st, sn, x), "aten": make_aten(hf, B, nx, st, sn, x)}
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
        row = {}
        for k, v in ms.items():
            med = statistics.median(v)
            row[k] = {"ms_per_step": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                      "samples_per_s": round(B / med * 1e3, 1)}
        tf = row["engine"]["samples_per_s"] * fps / 1e12
        row["engine"]["tflops"] = round(tf, 3)
        row["engine"]["frac_of_fp32_mfma_peak"] = round(tf / PEAK_TFLOPS, 5)
        row["engine_over_aten"] = round(row["aten"]["ms_per_step"] / row["engine"]["ms_per_step"], 3)
        res[str(B)] = row
        print(f"batch {B}: engine {row['engine']['ms_per_step']} ms/step, aten {row['aten']['ms_per_step']} ms/step",
              file=sys.stderr, flush=True)
    line = json.dumps({"metric": "PureGNN training step (forward, state-MSE loss, backward, Adam)",
                       "model": "PureGNN(4,128,4) f32", "cells": nx, "steps_per_window": args.steps,
                       "windows": args.repeats, "flop_per_sample": fps, "peak_tflops": PEAK_TFLOPS,
                       "note": "whole optimizer step over peak (end to end, not a kernel's share); aten = batched "
                               "torch forward + autograd + torch.optim.Adam on the same GPU in the same run",
                       "lib": version(), "batches": res})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
