"""Training-step time of PINN on the engine against the batched ATen restatement.

One "step" = one optimizer step of scripts/training/train_pinn.py's loop
(:156-179) on a batch of B samples of 64 cells: forward, the physics loss,
backward, Adam.  PINN(192, 256, 4) (the reference's, :133), at B = 32 (the
reference's batch) and B = 2000 x 64 cells.  Synthetic states (seeded normal;
the time does not depend on the values).

  engine          hybridflux.training.pinn_step: hf_pinn_forward_train,
                  hf_pinn_loss, hf_pinn_backward and FlatAdam (hf_adam_flat),
                  launched eagerly
  engine_graphed  the same step captured once as a HIP graph and replayed
                  (training.GraphedPinnStep): what is left when the host's
                  launch work is taken out
  aten            what a user would otherwise run on the same GPU: the oracle's
                  torch forward on the device, the loss of the same formulas in
                  torch ops (rolls, the Poisson operator as a circulant matmul),
                  torch autograd and torch.optim.Adam.  The comparison, not the
                  code under test.

All run in the same process, alternating, `--repeats` windows of `--steps`
steps each after a warm-up of all; a window is a host clock around steps that
end in a device synchronise.  Reported per batch: the median window's ms/step
and samples/s, the min..max spread, the engine's fraction of the fp32 MFMA peak
under the algorithmic FLOP model (training.pinn_train_flop_per_sample: a
whole-step rate over peak, not a kernel's share), and the device kernels and
memsets per step counted by torch.profiler in a separate untimed step
("not measured" when the profiler is unavailable).  Prints one JSON line;
--out also writes it to a file.

    python tools/bench_pinn_train.py [--batches 32,2000] [--steps 20] [--repeats 7] [--out FILE]
"""
import argparse
import json
import math
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
D, H, L, NX = 192, 256, 4, 64
DT, NU, DX = 5e-3, 1e-3, 2 * math.pi / 64
W = (1.0, 0.1, 0.1, 0.01)


def make_engine(hf, st, sn, graphed):
    from hybridflux.training import FlatAdam, GraphedPinnStep, pinn_step
    torch.manual_seed(0)
    m = hf.PINN(D, H, L).to("cuda").flatten_parameters_()
    opt = FlatAdam(m.parameters(), lr=1e-3)
    if not graphed:
        return lambda: pinn_step(m, opt, st, sn, DX, DT, NU, W)
    gs = GraphedPinnStep(m, opt, tuple(st.shape), DX, DT, NU, W, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            gs(st, sn)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gs.capture()
    return lambda: gs(st, sn)


def make_aten(hf, st, sn):
    from ctypes import c_void_p

    from hybridflux._lib import check, lib
    from oracle import hybrid_oracle as O
    torch.manual_seed(0)
    ref = hf.PINN(D, H, L)
    p = {k: v.detach().clone().to("cuda").requires_grad_(True) for k, v in ref.state_dict().items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    col = np.empty(lib().hf_poisson_plan_len(NX), dtype=np.float64)
    check(lib().hf_poisson_coeffs(NX, NX * DX, col.ctypes.data_as(c_void_p)))
    i = np.arange(NX)
    PT = torch.as_tensor(col[:NX][(i[:, None] - i[None, :]) % NX].T.astype(np.float32), device="cuda").contiguous()
    keep = torch.ones(NX, device="cuda")
    keep[0] = 0.0
    n, u, E = st[:, 0], st[:, 1], st[:, 2]

    def step():
        pred = O.pinn_forward(p, st)
        up, dn = torch.roll(u, -1, -1), torch.roll(u, 1, -1)
        f = n * u
        r_c = (pred[:, 0] - n) / DT + (torch.roll(f, -1, -1) - torch.roll(f, 1, -1)) / (2 * DX)
        r_m = (pred[:, 1] - u) / DT + u * (up - dn) / (2 * DX) + E - NU * (up - 2 * u + dn) / DX ** 2
        r_p = pred[:, 2] + (pred[:, 0] @ PT) * keep
        loss = W[0] * ((pred - sn) ** 2).mean() + W[1] * (r_c ** 2).mean() + W[2] * (r_m ** 2).mean() + \
            W[3] * (r_p ** 2).mean()
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


def device_ops_per_step(step):
    """Kernels + memsets + device copies of one step, from torch.profiler (untimed)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n if n > 0 else "not measured"
    except Exception:  # noqa: BLE001  (the count is a by-product; the timing above stands without it)
        return "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,2000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pinn_train: no HIP device visible (this benchmark has no CPU path)")
    import hybridflux as hf
    from hybridflux._lib import version
    from hybridflux.training import pinn_train_flop_per_sample
    fps = pinn_train_flop_per_sample(D, H, L)
    res = {}
    for B in [int(v) for v in args.batches.split(",") if v]:
        g = torch.Generator().manual_seed(B)
        st = torch.stack([1 + 0.1 * torch.randn(B, NX, generator=g), 0.1 * torch.randn(B, NX, generator=g),
                          0.1 * torch.randn(B, NX, generator=g)], dim=1).to("cuda").contiguous()
        sn = (st + 0.01 * torch.randn(B, 3, NX, generator=g).to("cuda")).contiguous()
        runs = {"engine": make_engine(hf, st, sn, False), "engine_graphed": make_engine(hf, st, sn, True),
                "aten": make_aten(hf, st, sn)}
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
        for k in ("engine", "engine_graphed"):
            tf = row[k]["samples_per_s"] * fps / 1e12
            row[k]["tflops"] = round(tf, 4)
            row[k]["frac_of_fp32_mfma_peak"] = round(tf / PEAK_TFLOPS, 6)
        row["engine_over_aten"] = round(row["aten"]["ms_per_step"] / row["engine"]["ms_per_step"], 3)
        row["engine_graphed_over_aten"] = round(row["aten"]["ms_per_step"] / row["engine_graphed"]["ms_per_step"], 3)
        row["engine"]["device_ops_per_step"] = device_ops_per_step(runs["engine"])
        row["aten"]["device_ops_per_step"] = device_ops_per_step(runs["aten"])
        res[str(B)] = row
        print(f"batch {B}: engine {row['engine']['ms_per_step']} ms/step, graphed "
              f"{row['engine_graphed']['ms_per_step']} ms/step, aten {row['aten']['ms_per_step']} ms/step",
              file=sys.stderr, flush=True)
    line = json.dumps({"metric": "PINN training step (forward, physics loss, backward, Adam)",
                       "model": f"PINN({D},{H},{L}) f32", "cells": NX, "steps_per_window": args.steps,
                       "windows": args.repeats, "flop_per_sample": fps, "peak_tflops": PEAK_TFLOPS,
                       "engine_launches_per_step": {"forward": L, "loss": "1 + a memset node", "backward": L + 3,
                                                    "adam": 1},
                       "note": "whole optimizer step over peak (end to end, not a kernel's share); aten = batched "
                               "torch forward + loss in torch ops + autograd + torch.optim.Adam on the same GPU in "
                               "the same run; device_ops_per_step = kernels, memsets and copies seen by "
                               "torch.profiler in one untimed step",
                       "lib": version(), "batches": res})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
