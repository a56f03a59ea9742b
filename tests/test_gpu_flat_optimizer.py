"""GPU tests of the guarded optimizer step (hf_adam_flat_ex behind FlatAdam's
weight_decay / max_grad_norm / skip_nonfinite options and a tensor lr;
csrc/optim.hip).

  1. neutral ..... with neutral options the guarded kernel is the plain one bit for bit
  2. parity ...... every length of optim_cases x clip below / at / above the norm x weight
                   decay, six steps against optim_ref with the kernel's coefficients; the
                   gates are float32 rounding: p (2S+2) 2^-24 max(1, max|p|), m and v
                   3S 2^-24 max|.| (S = 6 steps)
  3. norm ........ float64 accumulation: mixed magnitudes, values whose squares overflow
                   float32, two calls bit-equal
  4. skip ........ one inf / NaN anywhere in the gradient leaves p, m, v and the step count
                   untouched, is counted, and leaves no trace in the next step
  5. schedule .... a torch scheduler on a tensor lr, eager and through a captured PINN step
  6. state_dict .. a round trip through the host continues bit for bit
  7. driver ...... train_unrolled skips a poisoned batch and ends where the run without
                   that batch ends; without the option the parameters are lost
  8. trainers .... the other five trainers: a neutral guard changes no bit and reports
                   the statistics, a real one with a schedule trains finite parameters
"""
import functools
import io

import numpy as np
import pytest
import torch

import optim_cases as C
import optim_ref as R
from conftest import close, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 6
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
U = 2.0 ** -24


@pytest.fixture(scope="module")
def T():
    from hybridflux import _lib, training
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return training


@functools.lru_cache(maxsize=2)
def data(n):
    """(p0, [g_0 .. g_{S-1}]) of optim_cases.gradients on the device, made once per length."""
    p0, gs = C.gradients(n, S)
    return torch.as_tensor(p0, device=DEV), [torch.as_tensor(g, device=DEV) for g in gs]


def make(T, p0, **kw):
    p = torch.nn.Parameter(p0.clone())
    kw.setdefault("lr", LR)
    return p, T.FlatAdam([p], betas=BETAS, eps=EPS, **kw)


def run(p, opt, gs):
    for g in gs:
        p.grad = g
        opt.step()


def pmv(p, opt):
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], st["step"]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------- 1. neutral options
@pytest.mark.parametrize("n", [1025, C.MODEL_SIZES["FluxGNN(4,128,4)"]])
def test_neutral_options_are_the_plain_step_bit_for_bit(T, n):
    p0, gs = data(n)
    pa, oa = make(T, p0)
    run(pa, oa, gs)
    assert oa.last_stats is None and "stats" not in oa.state[pa]
    neutral = [dict(lr=torch.tensor(LR)),                                    # the guarded kernel, no norm launch
               dict(lr=torch.tensor(LR), max_grad_norm=1e30),                # coef clamps to exactly 1
               dict(max_grad_norm=1e30, skip_nonfinite=True, weight_decay=0.0)]
    for kw in neutral:
        pb, ob = make(T, p0, **kw)
        run(pb, ob, gs)
        for a, b, what in zip(pmv(pa, oa), pmv(pb, ob), "pmvt"):
            assert same_bits(a, b), (what, sorted(kw))
        if "max_grad_norm" in kw:
            assert ob.last_stats.tolist()[1:] == [1.0, 0.0, 0.0]
    assert float(oa.state[pa]["step"]) == S


# --------------------------------------------------------------------------- 2. parity
@pytest.mark.parametrize("wd", [0.0, 0.01, 0.1])
@pytest.mark.parametrize("clip", ["below", "at", "above"])
@pytest.mark.parametrize("n", C.LENGTHS)
def test_parity_with_the_float64_reference(T, n, clip, wd):
    p0, gs = data(n)
    # the threshold relative to the norm of the gradient of scale 1 (step 1): well below
    # every norm / equal to that one (the steps of scale 10 clip, those of 0.1 do not) /
    # above every norm
    norm1 = R.grad_norm(gs[1])
    max_norm = float(np.float32({"below": 1e-3, "at": 1.0, "above": 1e3}[clip] * norm1))
    p, opt = make(T, p0, weight_decay=wd, max_grad_norm=max_norm)
    kw = R.kernel_coefficients(LR, BETAS, EPS, wd, max_norm)
    rp, rm, rv, t = p0.double(), torch.zeros_like(p0).double(), torch.zeros_like(p0).double(), 0
    coefs = []
    for g in gs:
        p.grad = g
        opt.step()
        rp, rm, rv, t, stats = R.step(rp, rm, rv, g, t, **kw)
        got = opt.last_stats.tolist()
        coefs.append(stats[1])
        assert abs(got[0] - stats[0]) <= 2 * U * stats[0] and got[2] == 0.0
        assert abs(got[1] - stats[1]) <= 4 * U
    gp, gm, gv, gt = pmv(p, opt)
    assert float(gt) == t == S
    close(gp, rp.cpu().numpy(), (2 * S + 2) * U * max(1.0, float(rp.abs().max())), what="p")
    close(gm, rm.cpu().numpy(), 3 * S * U * float(rm.abs().max()), what="m")
    close(gv, rv.cpu().numpy(), 3 * S * U * float(rv.abs().max()), what="v")
    if n >= C.THREADS - 1:  # (the norms of a few random values scatter; those of many follow the scales)
        if clip == "below":
            assert max(coefs) < 0.1
        if clip == "above":
            assert min(coefs) == 1.0
        if clip == "at":
            assert min(coefs) < 0.2 and max(coefs) == 1.0


# ----------------------------------------------------------------------------- 3. norm
def _norm_of(T, g):
    p, opt = make(T, torch.zeros_like(g), skip_nonfinite=True)
    run(p, opt, [g])
    return opt.last_stats.clone(), p.detach().clone()


@pytest.mark.parametrize("small", [1e-4, 1.0])
def test_norm_is_accumulated_in_float64(T, small):
    """One 1e4 beside 2^20 values of 1e-4, and beside 2^20 ones: there a float32 sum that
    holds the 1e8 first is blind to every further square of 1 (its ulp is 8)."""
    n = (1 << 20) + 1
    g = torch.full((n,), small, device=DEV)
    g[n // 3] = 1e4
    want = np.float32(np.sqrt(float(np.float32(1e4)) ** 2 + (n - 1) * float(np.float32(small)) ** 2))
    stats, p = _norm_of(T, g)
    assert abs(float(stats[0]) - float(want)) <= float(np.spacing(want))
    assert stats.tolist()[2:] == [0.0, 0.0]
    # two calls on the same buffer
    stats2, p2 = _norm_of(T, g)
    assert same_bits(stats, stats2) and same_bits(p, p2)


def test_norm_of_values_whose_squares_overflow_float32(T):
    g = torch.full((4,), 1e30, device=DEV)
    stats, p = _norm_of(T, g)
    want = np.float32(2.0 * float(np.float32(1e30)))
    assert np.isfinite(float(stats[0])) and abs(float(stats[0]) - float(want)) <= float(np.spacing(want))
    assert stats.tolist()[2:] == [0.0, 0.0]  # no spurious skip


# ----------------------------------------------------------------------------- 4. skip
def _positions(n):
    return sorted({i for i in (0, n - 1, C.TILE - 1, C.TILE, C.TILE + 1) if 0 <= i < n})


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("n", [C.TILE + 1, C.MODEL_SIZES["PINN(192,256,4)"]])
def test_nonfinite_gradient_skips_the_step(T, n, bad):
    p0, gs = data(n)
    kw = dict(weight_decay=0.01, max_grad_norm=1.0, skip_nonfinite=True)
    p, opt = make(T, p0, **kw)
    run(p, opt, gs[:2])
    for count, i in enumerate(_positions(n), start=1):
        before = [t.clone() for t in pmv(p, opt)]
        poisoned = gs[2].cpu()
        poisoned[i] = bad  # written from the host side
        run(p, opt, [poisoned.to(DEV)])
        for a, b, what in zip(before, pmv(p, opt), "pmvt"):
            assert same_bits(a, b), (what, i)
        stats = opt.last_stats.tolist()
        assert stats[1:] == [0.0, 1.0, float(count)] and not np.isfinite(stats[0])
        assert float(opt.state[p]["step"]) == 2.0
        assert int(opt.state[p]["done"].view(torch.int32)) == 0
    # the next step, against an optimizer that starts from a copy of that state and never saw a bad gradient
    q, clean = make(T, before[0], **kw)
    for k, t in zip(("exp_avg", "exp_avg_sq", "step"), before[1:]):
        clean.state[q][k].copy_(t)
    run(p, opt, [gs[3]])
    run(q, clean, [gs[3]])
    for a, b, what in zip(pmv(p, opt), pmv(q, clean), "pmvt"):
        assert same_bits(a, b), what
    assert float(opt.state[p]["step"]) == 3.0 and not same_bits(p.detach(), before[0])
    assert opt.last_stats.tolist()[2:] == [0.0, float(count)] and clean.last_stats.tolist()[2:] == [0.0, 0.0]


# ------------------------------------------------------------------------- 5. schedule
def test_scheduler_drives_a_tensor_lr(T):
    n = C.MODEL_SIZES["PureGNN(4,128,4)"]
    p0, gs = data(n)
    pa, oa = make(T, p0, lr=torch.tensor(LR))
    lr_tensor = oa.param_groups[0]["lr"]
    assert lr_tensor.device == torch.device(DEV) and lr_tensor.dtype == torch.float32
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(oa, T_max=3)
    pb, ob = make(T, p0)
    seen = []
    for g in gs[:3]:
        lr = float(oa.param_groups[0]["lr"])
        seen.append(lr)
        ob.param_groups[0]["lr"] = lr
        run(pa, oa, [g])
        run(pb, ob, [g])
        sched.step()
        assert oa.param_groups[0]["lr"] is lr_tensor and lr_tensor.data_ptr() == oa.param_groups[0]["lr"].data_ptr()
    assert seen[0] == float(np.float32(LR)) and seen[0] > seen[1] > seen[2] > 0
    for a, b, what in zip(pmv(pa, oa), pmv(pb, ob), "pmvt"):
        assert same_bits(a, b), what


def test_captured_pinn_step_follows_the_scheduler(T):
    """GraphedPinnStep at batch 8, nx = 16 with clipping and skipping on: three eager
    steps, the capture, three replays, a scheduler step after every one, against the
    same six steps taken eagerly."""
    import hybridflux
    nx, B = 16, 8
    s = hybridflux.BaselineSolver(nx, device=DEV)
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(6):
        st = torch.stack([1 + 0.1 * torch.randn(B, nx, generator=g), 0.1 * torch.randn(B, nx, generator=g),
                          0.1 * torch.randn(B, nx, generator=g)], dim=1)
        batches.append((st.to(DEV), (st + 0.01 * torch.randn(B, 3, nx, generator=g)).to(DEV)))

    def six(graphed):
        torch.manual_seed(11)
        m = hybridflux.PINN(3 * nx, 64, 3).to(DEV).flatten_parameters_()
        opt = T.FlatAdam(m.parameters(), lr=torch.tensor(1e-3), max_grad_norm=1e-3, skip_nonfinite=True)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.7)
        gs = T.GraphedPinnStep(m, opt, (B, 3, nx), s.dx, s.dt, s.nu, device=DEV)
        rows, stats = [], []
        for k, (st, sn) in enumerate(batches):
            if graphed and k == 3:
                torch.cuda.synchronize()
                gs.capture()
            if graphed and gs.graph is None:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    rows.append(gs(st, sn))
                torch.cuda.current_stream().wait_stream(side)
            else:
                rows.append(gs(st, sn))
            stats.append(opt.last_stats.clone())
            sched.step()
        assert graphed == (gs.graph is not None)
        flat = torch.cat([q.detach().reshape(-1) for q in m.parameters()]).clone()
        return torch.stack(rows), torch.stack(stats), flat, opt.state[next(iter(m.parameters()))]["step"].clone()

    rows, stats, flat, step = six(False)
    rows_g, stats_g, flat_g, step_g = six(True)
    assert same_bits(rows, rows_g) and same_bits(stats, stats_g) and same_bits(flat, flat_g)
    assert float(step) == float(step_g) == 6.0
    assert (stats[:, 1] < 1.0).any() and (stats[:, 2] == 0).all()  # clipping was active; nothing skipped
    assert torch.isfinite(flat).all()


# ----------------------------------------------------------------------- 6. state_dict
def test_state_dict_round_trip_through_the_host(T):
    n = C.MODEL_SIZES["FluxGNN(4,128,4)"]
    p0, gs = data(n)
    kw = dict(lr=torch.tensor(LR), weight_decay=0.01, max_grad_norm=1.0, skip_nonfinite=True)
    bad = gs[2].clone()
    bad[n // 2] = float("nan")
    pa, oa = make(T, p0, **kw)
    run(pa, oa, [gs[0], bad, gs[1]])
    buf = io.BytesIO()
    torch.save(oa.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu")
    assert sorted(sd["state"][0]) == ["done", "exp_avg", "exp_avg_sq", "stats", "step"]
    assert all(v.device.type == "cpu" for v in sd["state"][0].values())
    pb, ob = make(T, pa.detach(), **dict(kw, lr=torch.tensor(5.0)))
    held = ob.param_groups[0]["lr"]
    ob.load_state_dict(sd)
    assert ob.param_groups[0]["lr"] is held and float(held) == float(np.float32(LR))  # one address, the loaded value
    rest = [gs[3], bad, gs[4]]
    run(pa, oa, rest)
    run(pb, ob, rest)
    for a, b, what in zip(pmv(pa, oa), pmv(pb, ob), "pmvt"):
        assert same_bits(a, b), what
    assert same_bits(oa.last_stats, ob.last_stats)
    assert float(ob.state[pb]["step"]) == 4.0 and float(ob.last_stats[3]) == 2.0
    assert ob.state[pb]["stats"].device == torch.device(DEV)


# --------------------------------------------------------------------------- 7. driver
def test_train_unrolled_skips_a_poisoned_batch(T, monkeypatch):
    """Three batches A, P, B of two K = 4 windows at nx = 16; one target cell of P is inf."""
    import hybridflux
    from hybridflux import datagen
    nx, K, bs, seed = 16, 4, 2, 0
    w = golden("weights_W1_r2.npz")
    init = {k: w[k] for k in w.files}
    tr = datagen.generate_trajectories(nx=nx, num_initial_conditions=3 * bs, steps_per_ic=K, device=DEV)
    assert tr.shape == (3 * bs, K + 1, 3, nx)  # one window per initial condition
    # the trainer's order of the epoch: batch k holds windows order[k bs : (k + 1) bs]
    order3 = torch.randperm(3 * bs, generator=torch.Generator().manual_seed(seed)).numpy()
    order2 = torch.randperm(2 * bs, generator=torch.Generator().manual_seed(seed)).numpy()
    poisoned = tr.copy()
    poisoned[order3[bs + 1], 2, 0, 5] = np.inf  # a target (time index >= 1) of P's second window
    without = np.empty_like(tr[:2 * bs])        # A and B alone, placed so that the shorter epoch's order finds them
    without[order2[:bs]] = tr[order3[:bs]]
    without[order2[bs:]] = tr[order3[2 * bs:]]

    made = []

    class Spy(T.FlatAdam):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(T, "FlatAdam", Spy)
    s = hybridflux.BaselineSolver(nx, device=DEV)

    def train(data, **kw):
        m, h = T.train_unrolled(data, s.x, s.dt, s.dx, s.nu, K=K, epochs=1, lr=1e-4, batch_size=bs, seed=seed,
                                init=init, device=DEV, save_dir=None, log=None, **kw)
        opt = made[-1]
        flat = torch.cat([q.detach().reshape(-1) for q in m.parameters()]).clone()
        return flat, h, float(opt.state[opt.param_groups[0]["params"][0]]["step"])

    flat_ab, h_ab, steps_ab = train(without)
    assert sorted(h_ab) == ["epoch", "loss", "seconds"] and steps_ab == 2.0  # the defaults: today's keys
    assert torch.isfinite(flat_ab).all() and np.isfinite(h_ab["loss"]).all()
    flat, h, steps = train(poisoned, skip_nonfinite=True)
    assert sorted(h) == ["epoch", "grad_norm_max", "loss", "seconds", "skipped_steps"]
    assert h["skipped_steps"] == [1] and steps == 2.0
    assert torch.isfinite(flat).all() and same_bits(flat, flat_ab)
    assert h["loss"] == h_ab["loss"] and np.isfinite(h["grad_norm_max"]).all() and h["grad_norm_max"][0] > 0
    # sharpness: without the option the same run loses the parameters
    flat_lost, h_lost, steps_lost = train(poisoned)
    assert not torch.isfinite(flat_lost).all() and steps_lost == 3.0
    assert sorted(h_lost) == ["epoch", "loss", "seconds"]


# ------------------------------------------------------------------- 8. the other trainers
def _trainer(T, name):
    """(run(**options) -> (flat parameters, history), the history's default keys) of a small job of trainer `name`."""
    import hybridflux
    from hybridflux import datagen
    flat = lambda m: torch.cat([q.detach().reshape(-1) for q in m.parameters()]).clone()  # noqa: E731
    if name in ("train_model", "train_pure_gnn", "train_pinn"):
        st, ft, sn, x, dt, dx, nu = datagen.generate_dataset(num_initial_conditions=2, steps_per_ic=8, out_path=None,
                                                             device=DEV)
        if name == "train_model":
            return (lambda **kw: T.train_model(st, ft, sn, x, dt, dx, nu, "physics", 2, epochs=2, device=DEV,
                                               batch_size=8, seed=1, save_dir=None, log=None, **kw),
                    flat, ["epoch", "flux_loss", "loss", "seconds"])
        if name == "train_pure_gnn":
            return (lambda **kw: T.train_pure_gnn(st, sn, x, epochs=2, batch_size=8, hidden_dim=64, num_layers=3,
                                                  device=DEV, seed=1, **kw), flat, ["loss"])
        return (lambda **kw: T.train_pinn(st, sn, dx, dt, nu, epochs=2, batch_size=8, hidden_dim=64, num_layers=3,
                                          seed=1, device=DEV, **kw),
                flat, sorted(["loss", "loss_data", "loss_continuity", "loss_momentum", "loss_poisson"]))
    nx = 16
    tr = datagen.generate_trajectories(nx=nx, num_initial_conditions=4, steps_per_ic=6, device=DEV)
    s = hybridflux.BaselineSolver(nx, device=DEV)
    if name == "train_pure_gnn_unrolled":
        return (lambda **kw: T.train_pure_gnn_unrolled(tr, s.x, K=3, epochs=2, batch_size=8, hidden_dim=64,
                                                       num_layers=3, seed=0, device=DEV, save_dir=None, log=None,
                                                       **kw), flat, ["epoch", "loss", "seconds"])
    return (lambda **kw: T.train_pinn_unrolled(tr, s.dx, s.dt, s.nu, K=3, epochs=2, batch_size=8, hidden_dim=64,
                                               num_layers=3, seed=0, device=DEV, save_dir=None, log=None, **kw),
            flat, ["epoch", "loss", "seconds"])


@pytest.mark.parametrize("name", ["train_model", "train_pure_gnn", "train_pinn", "train_pure_gnn_unrolled",
                                  "train_pinn_unrolled"])
def test_trainers_take_the_guard_options(T, name):
    """A neutral guard (a threshold no norm reaches, skipping on) trains the same
    parameters bit for bit and reports the statistics; a real one (clipping, decay and
    a halving schedule) trains other, finite ones."""
    run, flat, keys = _trainer(T, name)
    m0, h0 = run()
    assert sorted(h0) == keys
    m1, h1 = run(max_grad_norm=1e30, skip_nonfinite=True)
    assert sorted(h1) == sorted(keys + ["grad_norm_max", "skipped_steps"])
    assert same_bits(flat(m0), flat(m1))
    assert h1["skipped_steps"] == [0, 0] and all(np.isfinite(v) and v > 0 for v in h1["grad_norm_max"])
    for k in keys:
        if k not in ("epoch", "seconds"):  # (means taken on the host here, on the device there)
            assert np.allclose(h1[k], h0[k], rtol=1e-5, atol=0.0), k
    halve = lambda opt: torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)  # noqa: E731
    m2, h2 = run(max_grad_norm=0.5 * min(h1["grad_norm_max"]), weight_decay=0.01, scheduler=halve)
    assert torch.isfinite(flat(m2)).all() and not same_bits(flat(m0), flat(m2))
    assert h2["skipped_steps"] == [0, 0] and sorted(h2) == sorted(h1)
