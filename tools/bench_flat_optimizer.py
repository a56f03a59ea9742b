"""Time of the optimizer step, plain and guarded, alone and inside the K-step
training step.

Part 1, the optimizer step alone, on a flat buffer of each model's parameter
count (FluxGNN(4,128,4), PureGNN(4,128,4), PINN(192,256,4)) with one fixed
gradient:

  plain    FlatAdam (hf_adam_flat, one launch)
  guarded  FlatAdam(weight_decay=0.01, max_grad_norm=1.0, skip_nonfinite=True)
           (hf_adam_flat_ex: the norm's launch and the update)
  torch    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(weight_decay=0.01,
           fused=True, capturable=True) on the same flat parameter; it has no
           skip of a non-finite step (that would be further launches)

each timed two ways: "eager" (a host clock around `--steps` steps ending in a
device synchronise: for steps this short it measures the host's launch rate as
much as the device) and "graphed" (`--inner` steps captured as one HIP graph and
replayed `--steps / --inner` times, 5 at least: the device's own time per
step).  All arms of a size run in one process, alternating, `--repeats` windows each after a warm-up of
all; reported are the median window's microseconds per step, the min..max
spread and the launches per step counted by torch.profiler on one eager step.

Part 2, the whole K-step training step of tools/bench_unrolled_train.py (B =
2000 windows x 64 cells, K = 4, FluxGNN(4,128,4), training.unrolled_step) with
the guard on against off, alternating windows as there; the ratio is given for
the medians and window by window.  With the guard off the step is the one
tools/bench_unrolled_train.py times; its committed record
(profiles/unrolled_train_bench.json), when present, is quoted beside it.

Prints one JSON line and writes it to --out.

    python tools/bench_flat_optimizer.py [--steps 200] [--inner 20] [--repeats 7] [--out FILE]
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

GUARD = dict(weight_decay=0.01, max_grad_norm=1.0, skip_nonfinite=True)


def window(step, steps, per=1):
    """Microseconds per optimizer step of `steps` calls of step (each `per` steps)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (steps * per) * 1e6


def launches(step):
    """Device kernels (and memsets / copies) of one warm step, by torch.profiler;
    the device-side copy of torch's "Optimizer.step#..." annotation is no launch
    and is left out.  The kernels' names go to stderr."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()
                 if str(e.device_type).endswith("CUDA") and not e.name.startswith("Optimizer.step")]
        print(f"launches: {len(names)}: {names}", file=sys.stderr)
        return len(names) if names else "not measured"
    except Exception:  # a profiler that cannot attach must not cost the timing run
        return "not measured"


def graphed(step, inner, warmup=3):
    """`inner` calls of step captured as one graph; returns its replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            step()
    return g.replay


def optimizer_arms(n):
    from hybridflux.training import FlatAdam
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen).to("cuda")
    g0 = torch.randn(n, generator=gen).to("cuda")
    arms = {}
    for name, kw in (("plain", {}), ("guarded", GUARD)):
        p = torch.nn.Parameter(p0.clone())
        p.grad = g0.clone()
        arms[name] = FlatAdam([p], lr=1e-3, **kw).step
    p = torch.nn.Parameter(p0.clone())
    p.grad = g0.clone()
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=GUARD["weight_decay"], fused=True, capturable=True)

    def torch_step():
        torch.nn.utils.clip_grad_norm_([p], GUARD["max_grad_norm"])
        opt.step()
    arms["torch"] = torch_step
    return arms


def summary(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def alternate(runs, steps, repeats, per=1):
    """`repeats` alternating windows of every run after a warm-up of all."""
    for step in runs.values():
        window(step, max(3, steps // 10), per)
    t_end = time.perf_counter() + 0.3  # back-to-back load before timing: the clock ramps under load
    while time.perf_counter() < t_end:
        for step in runs.values():
            window(step, max(3, steps // 10), per)
    out = {k: [] for k in runs}
    for _ in range(repeats):
        for k, step in runs.items():
            out[k].append(window(step, steps, per))
    return out


def bench_optimizer(n, steps, inner, repeats):
    arms = optimizer_arms(n)
    res = {k: {} for k in arms}
    for k, v in alternate(arms, steps, repeats).items():
        res[k]["eager_us_per_step"] = summary(v)
    for k, step in arms.items():
        res[k]["launches_per_step"] = launches(step)
    replays = {k: graphed(step, inner) for k, step in arms.items()}
    for k, v in alternate(replays, max(steps // inner, 5), repeats, per=inner).items():
        res[k]["graphed_us_per_step"] = summary(v)
    for mode in ("eager", "graphed"):
        key = f"{mode}_us_per_step"
        res[f"guarded_over_plain_{mode}"] = round(res["guarded"][key]["median"] / res["plain"][key]["median"], 3)
        res[f"torch_over_guarded_{mode}"] = round(res["torch"][key]["median"] / res["guarded"][key]["median"], 3)
    return res


def bench_training_step(batch, K, steps, repeats):
    import hybridflux as hf
    from hybridflux import training
    nx = 64
    solver = hf.BaselineSolver(nx, device="cuda")
    grid = solver.grid
    x, _ = grid.on(torch.device("cuda", torch.cuda.current_device()))
    ics = solver.initial_conditions(list(range(batch)), as_tensor=True)
    traj = solver.run_batch(ics, K, traj=True)["traj"].contiguous()  # [B,K+1,3,nx]
    runs = {}
    for name, kw in (("guard_off", {}), ("guard_on", GUARD)):
        torch.manual_seed(0)
        m = hf.FluxGNN(4, 128, 4).to("cuda").flatten_parameters_()
        opt = training.FlatAdam(m.parameters(), lr=1e-4, **kw)

        def step(m=m, opt=opt):
            loss = training.unrolled_step(m, opt, traj, x, grid)
            assert loss is not None
            return loss
        runs[name] = step
    res = {k: {} for k in runs}
    us = alternate(runs, steps, repeats)
    for k, v in us.items():
        res[k]["ms_per_step"] = summary([t / 1e3 for t in v], 4)
    for k, step in runs.items():
        res[k]["launches_per_step"] = launches(step)
    ratios = [a / b for a, b in zip(us["guard_on"], us["guard_off"])]
    med = {k: statistics.median(v) for k, v in us.items()}
    res["on_over_off"] = {"of_medians": round(med["guard_on"] / med["guard_off"], 4),
                          "window_by_window": summary(ratios, 4)}
    record = os.path.join(ROOT, "profiles", "unrolled_train_bench.json")
    res["committed_record_ms_per_step"] = "not measured"
    if os.path.exists(record) and batch == 2000 and K == 4:
        with open(record) as f:
            old = json.loads(f.readline())
        if isinstance(old.get("result", {}).get("engine"), dict):
            ms = old["result"]["engine"]["ms_per_step"]
            res["committed_record_ms_per_step"] = ms
            res["guard_off_over_committed_record"] = round(res["guard_off"]["ms_per_step"]["median"] / ms, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="optimizer steps per window, part 1")
    ap.add_argument("--inner", type=int, default=20, help="optimizer steps per captured graph, part 1")
    ap.add_argument("--train-steps", type=int, default=10, help="training steps per window, part 2")
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_optimizer_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flat_optimizer: no HIP device visible (this benchmark has no CPU path)")
    if args.repeats < 5:
        raise SystemExit("bench_flat_optimizer: at least 5 repeats (the spread is part of the result)")
    from hybridflux._lib import lib, version
    sizes = {"FluxGNN(4,128,4)": int(lib().hf_model_param_count(4, 128, 4)),
             "PureGNN(4,128,4)": int(lib().hf_pure_gnn_param_count(4, 128, 4)),
             "PINN(192,256,4)": int(lib().hf_pinn_param_count(192, 256, 4))}
    opt_res = {name: dict(n=n, **bench_optimizer(n, args.steps, args.inner, args.repeats)) for name, n in sizes.items()}
    train_res = bench_training_step(args.batch, args.K, args.train_steps, args.repeats)
    line = json.dumps({"metric": "optimizer step on a flat parameter buffer: plain FlatAdam, guarded FlatAdam (clip + "
                                 "weight decay + non-finite skip), clip_grad_norm_ + fused capturable AdamW; and the "
                                 "K-step training step with the guard on against off",
                       "windows": args.repeats, "steps_per_window": args.steps, "steps_per_graph": args.inner,
                       "guard": GUARD,
                       "note": "eager = host clock around synchronised windows (launch-rate bound for steps this "
                               "short); graphed = the same steps captured and replayed (device time); the torch arm "
                               "has no non-finite skip; all arms of a size in one process, alternating windows",
                       "lib": version(), "optimizer_step": opt_res,
                       "training_step": dict(model="FluxGNN(4,128,4) f32", batch=args.batch, K=args.K, cells=64,
                                             steps_per_window=args.train_steps, **train_res)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
