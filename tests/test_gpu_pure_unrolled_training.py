"""GPU parity of PureGNN's unrolled training (hf_pure_unroll_update,
hf_pure_unroll_adjoint, hybridflux.training.pure_unrolled_loss /
pure_unrolled_step / train_pure_gnn_unrolled): PureGNN differentiated through K
steps of its own rollout state <- state + PureGNN([n,u,E,x]), against the CPU
oracle, the reference's own trainer run (tests/golden/pure_gnn_train.npz) and
torch-CPU float64 autograd of the same K-step loss.

Tolerances:
  one update given delta ................ bit-equal to the torch expression (one
      float32 add per value; the node features are copies)
  step loss ............................. rtol 1e-6 (an elementwise float32
      difference, squared and summed in float64: <= 2 ulp of float32 relative;
      test_gpu_unrolled_training's gate)
  adjoint kernel alone .................. 2e-5 max|ref| + 1e-12 max|g| per tensor
      (test_gpu_unrolled_training's gate: two or three float32 adds per value)
  K-step loss value ..................... rtol 1e-5 (torch-CPU float32 alone is
      1.3e-7 from float64 on these cases)
  K-step parameter gradients ............ per tensor max(4 d32, 2e-5 max|g64|), d32 the
      error of the same gradient in torch-CPU float32 (measured in the test; at
      most 7.5e-7 max|g64| on these cases, and no tensor's gradient vanishes:
      the smallest max|g64| is 0.033)
  K = 1 against the one-step trainer .... loss rtol 1e-6; six Adam steps: loss rtol
      1e-4, weights atol 2e-5, every element (test_gpu_pure_gnn_training's gate)
  predicted states, K = 4 ............... atol 5e-5 + rtol 5e-5 (test_gpu_baselines' gate
      on PureGNN rollouts; torch-CPU float32 alone is 2.1e-6 from float64)
Every measured error is recorded (conftest `record` / close)."""
import numpy as np
import pytest
import torch

from conftest import close, golden
from nx_regimes import PURE_WIDE
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2e-5
# (nx, B): one cell, two cells, a quarter of a wave, part of a wave, more than a
# wave, several workgroups of one tile each, and a chain of two tiles (1024 + 6 cells);
# then nx_regimes.PURE_WIDE: exactly one tile (1024), a one-cell tail tile (2049) and
# six whole tiles (6144, the other training kernels' limit)
SHAPES = [(1, 2), (2, 3), (16, 3), (48, 3), (100, 3), (64, 9), (1030, 2)] + PURE_WIDE


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    from hybridflux import _lib
    assert _lib.lib().hf_device_count() > 0, "GPU tests need a visible HIP device"
    return hybridflux


def sd128():
    """The reference-trained PureGNN(4,128,4) of baselines.npz."""
    b = golden("baselines.npz")
    return {k[len("pure_gnn."):]: b[k] for k in b.files if k.startswith("pure_gnn.") and "mlp" in k}


def sd64():
    """The PureGNN(4,64,3) starting weights of pure_gnn_train.npz."""
    f = golden("pure_gnn_train.npz")
    return {k[len("init."):]: f[k] for k in f.files if k.startswith("init.")}


def load(hf, sd, dims):
    m = hf.PureGNN(*dims)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(DEV)


def flat_of(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()


def ics(nx, B, seed0=0):
    G = O.Grid(nx)
    return G, np.stack([O.initial_condition(G, seed0 + s) for s in range(B)])


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def xdev(G):
    return dev(G.x.astype(np.float32))


# ------------------------------------------------------------------ 1. update forward
@pytest.mark.parametrize("nx,B", SHAPES)
def test_update(hf, nx, B):
    from hybridflux import _lib, engine
    from hybridflux.training import pure_gnn_features
    G, st = ics(nx, B)
    g = np.random.default_rng(nx * 100 + B)
    delta = g.normal(0, 0.05, (B * nx, 3)).astype(np.float32)
    tgt = (st + g.normal(0, 0.05, st.shape)).astype(np.float32)
    std, dd, x = dev(st), dev(delta), xdev(G)
    out, nf, loss = engine.pure_unroll_update(dd, std, x)
    assert loss is None
    want = std + dd.view(B, nx, 3).permute(0, 2, 1)
    assert torch.equal(out, want)
    assert torch.equal(nf, pure_gnn_features(want, x))
    out2, nf2, _ = engine.pure_unroll_update(dd, std, x, want_nf=False)
    assert nf2 is None and torch.equal(out2, want)
    # the loss term: float64 sum over the same float32 values; two calls, equal bits
    w, K = (1.0, 0.5, 2.0), 4
    scale = 1.0 / (K * 3 * B * nx)
    runs = []
    for _ in range(2):
        out3, nf3, loss = engine.pure_unroll_update(dd, std, x, target=dev(tgt), weights=w, scale=scale)
        runs.append(loss.cpu().numpy().copy())
        assert torch.equal(out3, want) and torch.equal(nf3, nf)
    ref = (np.asarray(w)[None, :, None] * (want.cpu().numpy().astype(np.float64) - tgt.astype(np.float64)) ** 2).mean() / K
    close(runs[0], np.asarray([ref]), 0.0, 1e-6, what="loss")
    assert np.array_equal(runs[0], runs[1])
    # no target: nothing is written to the loss element (and no workspace is needed)
    sentinel = torch.full((1,), 123.5, device=DEV)
    out4 = torch.empty_like(std)
    L = _lib.lib()
    with torch.cuda.device(std.device):
        _lib.check(L.hf_pure_unroll_update(_lib.ptr(dd), _lib.ptr(std), _lib.ptr(x), B, nx, _lib.ptr(out4), None, None,
                                           None, 1.0, _lib.ptr(sentinel), None, 0, engine.stream_of(std.device)))
    assert torch.equal(out4, want) and float(sentinel) == 123.5


def test_update_refuses_bad_tensors(hf):
    """The Python layer checks shape, dtype, device and contiguity (no fall-back)."""
    from hybridflux import engine
    G, st = ics(16, 3)
    std, dd, x = dev(st), torch.zeros(48, 3, device=DEV), xdev(G)
    with pytest.raises(ValueError):
        engine.pure_unroll_update(dd[:47], std, x)
    with pytest.raises(ValueError):
        engine.pure_unroll_update(dd.double(), std, x)
    with pytest.raises(ValueError):
        engine.pure_unroll_update(dd, std.permute(0, 2, 1).contiguous().permute(0, 2, 1), x)
    with pytest.raises(ValueError):
        engine.pure_unroll_update(dd, std, x, out=torch.empty(3, 3, 17, device=DEV))
    with pytest.raises(RuntimeError):
        engine.pure_unroll_update(dd, std.cpu(), x)
    with pytest.raises(ValueError):
        engine.pure_unroll_adjoint(std, std, (1, 1, 1), 1.0, gnf_next=torch.zeros(48, 3, device=DEV))


# ----------------------------------------------------------------- 2. adjoint alone
def adjoint_case(nx, B, mode):
    from hybridflux import engine
    _, st = ics(nx, B, seed0=3)
    g = np.random.default_rng(nx * 10 + B)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    sn = f32(st + g.normal(0, 0.05, st.shape))
    tg = f32(st + g.normal(0, 0.05, st.shape))
    gdn = f32(g.normal(0, 1e-3, (B * nx, 3)))
    gnf = f32(g.normal(0, 1e-3, (B * nx, 4)))
    w, scale = (1.0, 0.5, 2.0), 1.0 / (4 * 3 * B * nx)
    gdn_d = dev(gdn) if mode == "full" else None
    gnf_d = dev(gnf) if mode in ("full", "nf_only") else None
    runs = [engine.pure_unroll_adjoint(dev(sn), dev(tg), w, scale, gdn_d, gnf_d).cpu().numpy() for _ in range(2)]
    # reference: float64 autograd of the torch step, s' = s + delta^T with delta a free tensor
    up = np.zeros((B, 3, nx))
    if gdn_d is not None:
        up = up + gdn.astype(np.float64).reshape(B, nx, 3).transpose(0, 2, 1)
    if gnf_d is not None:
        up = up + gnf.astype(np.float64).reshape(B, nx, 4)[:, :, :3].transpose(0, 2, 1)
    d = torch.zeros(B * nx, 3, dtype=torch.float64, requires_grad=True)
    s1 = torch.as_tensor(sn, dtype=torch.float64) + d.view(B, nx, 3).permute(0, 2, 1)
    wt = torch.as_tensor(w, dtype=torch.float64)[None, :, None]
    (scale * (wt * (s1 - torch.as_tensor(tg, dtype=torch.float64)) ** 2).sum() + (torch.as_tensor(up) * s1).sum()).backward()
    gt = 2.0 * np.asarray(w)[None, :, None] * scale * (sn.astype(np.float64) - tg) + up
    return runs, d.grad.numpy(), float(np.abs(gt).max())


@pytest.mark.parametrize("mode", ["full", "last", "nf_only"])
@pytest.mark.parametrize("nx,B", SHAPES)
def test_adjoint_vs_autograd(hf, record, nx, B, mode):
    runs, want, gmax = adjoint_case(nx, B, mode)
    name = f"test_adjoint_vs_autograd[{nx}-{B}-{mode}]"
    err = float(np.abs(runs[0].astype(np.float64) - want).max())
    lim = REL * float(np.abs(want).max()) + 1e-12 * gmax
    record(name, "grad_delta_err", err)
    record(name, "grad_delta_limit", lim)
    assert np.isfinite(runs[0]).all() and err <= lim, (err, lim)
    assert np.array_equal(runs[0], runs[1])


# --------------------------------------------------------- 3. K-step parameter gradients
def classical_windows(G, B, K):
    _, st = ics(G.nx, B)
    traj, _ = O.classical_run(G, st, K)  # [B,K+1,3,nx], seeds 0..B-1
    return traj


def pure_unrolled_loss_cpu(sd, G, traj, w, dtype, through=True):
    """The K-step loss of oracle.pure_gnn_forward composed K times in torch-CPU
    `dtype`; returns (loss, {name: grad}, states [B,K,3,nx])."""
    p = {k: torch.as_tensor(v, dtype=dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = torch.as_tensor(G.x.astype(np.float32), dtype=dtype)
    tr = torch.as_tensor(traj, dtype=dtype)
    B, K1, _, nx = tr.shape
    ei = O.chain_edges(nx, B)
    wt = torch.as_tensor(w, dtype=dtype)[None, :, None]
    st, L, states = tr[:, 0], 0.0, []
    for j in range(1, K1):
        nf = torch.stack([st[:, 0], st[:, 1], st[:, 2], x.expand(B, nx)], dim=-1).reshape(B * nx, 4)
        st = st + O.pure_gnn_forward(p, nf, ei).view(B, nx, 3).permute(0, 2, 1)
        L = L + (wt * (st - tr[:, j]) ** 2).mean() / (K1 - 1)
        states.append(st.detach().numpy())
        if not through:
            st = st.detach()
    L.backward()
    return float(L.detach()), {k: v.grad.numpy().astype(np.float64) for k, v in p.items()}, np.stack(states, 1)


ONES = (1.0, 1.0, 1.0)
# (nx, B, K, hidden, weights): the fixture PureGNN(4,128,4) on the chain GEMMs, the
# PureGNN(4,64,3) starting weights at chain lengths that take the generic kernels
_GRAD_CASES = [(64, 3, 1, 128, ONES), (64, 3, 4, 128, ONES), (16, 3, 4, 128, ONES), (48, 2, 2, 64, ONES),
               (100, 2, 2, 64, ONES), (64, 3, 4, 128, (0.5, 2.0, 1.0))]
_REF = {}


def grad_reference(nx, B, K, hidden, w, through):
    """(sd, dims, traj, l64, g64, g32, l32), computed once per case and left unchanged."""
    key = (nx, B, K, hidden, w, through)
    if key not in _REF:
        G = O.Grid(nx)
        sd, dims = (sd128(), (4, 128, 4)) if hidden == 128 else (sd64(), (4, 64, 3))
        traj = classical_windows(G, B, K)
        l64, g64, _ = pure_unrolled_loss_cpu(sd, G, traj, w, torch.float64, through)
        l32, g32, _ = pure_unrolled_loss_cpu(sd, G, traj, w, torch.float32, through)
        _REF[key] = (sd, dims, traj, l64, g64, g32, l32)
    return _REF[key]


def gpu_grads(hf, sd, dims, traj, nx, w, through):
    from hybridflux import training
    m = load(hf, sd, dims)
    loss = training.pure_unrolled_loss(m, dev(traj), xdev(O.Grid(nx)), channel_weights=w, through_state=through)
    assert loss.shape == () and loss.requires_grad
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("through", [True, False])
@pytest.mark.parametrize("nx,B,K,hidden,w", _GRAD_CASES)
def test_unrolled_gradients(hf, record, nx, B, K, hidden, w, through):
    sd, dims, traj, l64, g64, g32, l32 = grad_reference(nx, B, K, hidden, w, through)
    loss, got = gpu_grads(hf, sd, dims, traj, nx, w, through)
    name = f"test_unrolled_gradients[{nx}-{B}-{K}-{hidden}-{w}-{through}]"
    record(name, "loss", loss)
    record(name, "loss_rel_err", abs(loss - l64) / abs(l64))
    record(name, "loss_rel_err_cpu32", abs(l32 - l64) / abs(l64))
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    assert set(got) == set(g64)
    for k, want in g64.items():
        err = float(np.abs(got[k].astype(np.float64) - want).max())
        scale = float(np.abs(want).max())
        d32 = float(np.abs(g32[k] - want).max())
        record(name, f"{k}_err", err)
        record(name, f"{k}_d32", d32)
        record(name, f"{k}_max", scale)
        assert np.isfinite(got[k]).all() and scale > 0
        assert err <= max(4 * d32, REL * scale), (k, err, d32, scale)


def test_k1_same_gradient_in_both_modes(hf):
    sd, dims, traj, *_ = grad_reference(64, 3, 1, 128, ONES, True)
    la, a = gpu_grads(hf, sd, dims, traj, 64, ONES, True)
    lb, b = gpu_grads(hf, sd, dims, traj, 64, ONES, False)
    assert la == lb
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------- 4. ties to the reference's own trainer, K = 1
@pytest.fixture(scope="module")
def fx():
    return golden("pure_gnn_train.npz")


def fixture_windows(fx):
    traj, bic, bt = fx["traj"], fx["batch_ic"], fx["batch_t"]
    return [dev(np.stack([traj[bic[j], bt[j]], traj[bic[j], bt[j] + 1]], axis=1)) for j in range(6)]


def test_k1_loss_equals_one_step_loss(hf, fx):
    from hybridflux import training
    m = load(hf, sd64(), (4, 64, 3))
    win, x = fixture_windows(fx)[0], dev(fx["x"])
    st, sn = win[:, 0].contiguous(), win[:, 1].contiguous()
    delta = m(training.pure_gnn_features(st, x), hf.chain_edge_index(64, st.shape[0], DEV))
    one = training.state_mse_loss(delta, st, sn)
    got = training.pure_unrolled_loss(m, win, x)
    close(got, one.detach().cpu().numpy().astype(np.float64), 0.0, 1e-6, what="loss")


def test_six_adam_steps_vs_reference(hf, fx, record, request):
    """Six pure_unrolled_steps at K = 1 on the fixture's six batches of 32 samples
    against the reference's own loop (torch.optim.Adam(lr=1e-3) from init.*)."""
    from hybridflux import training
    m = load(hf, sd64(), (4, 64, 3)).flatten_parameters_()
    opt = training.FlatAdam(m.parameters(), lr=1e-3)
    x = dev(fx["x"])
    losses = []
    for win in fixture_windows(fx):
        loss = training.pure_unrolled_step(m, opt, win, x)
        assert loss is not None
        losses.append(float(loss))
    close(np.array(losses), fx["adam_losses"], 0.0, 1e-4, what="losses")
    sd = m.state_dict()
    worst = 0.0
    for k in sd:
        worst = max(worst, close(sd[k], fx[f"adam_final.{k}"], 2e-5, 0.0, what=k))
    record(request.node.nodeid.split("::", 1)[-1], "weights_max_abs", worst)


# ------------------------------------------------------------- 5. rollout consistency
def test_predicted_states_vs_oracle(hf):
    from hybridflux import training
    nx, B, K = 64, 3, 4
    G = O.Grid(nx)
    sd = sd128()
    traj = classical_windows(G, B, K)
    m = load(hf, sd, (4, 128, 4))
    loss, pred = training.pure_unrolled_loss(m, dev(traj), xdev(G), return_states=True)
    assert loss.requires_grad and not pred.requires_grad and tuple(pred.shape) == (K, B, 3, nx)
    p = O.params_from(sd)
    want = np.stack([O.pure_gnn_rollout(p, G, traj[b, 0], K) for b in range(B)])
    close(pred.permute(1, 0, 2, 3).cpu().numpy(), want[:, 1:], 5e-5, 5e-5, what="states")


# ------------------------------------------------------ 6. direct step vs autograd step
@pytest.mark.parametrize("through", [True, False])
def test_direct_step_equals_autograd_step(hf, through):
    """pure_unrolled_step and pure_unrolled_loss -> backward -> FlatAdam.step() run
    the same launches and add the K parameter gradients in the same order (last
    step first): the parameters agree bit for bit, and so do two direct steps."""
    from hybridflux import training
    nx, B, K = 64, 3, 4
    G = O.Grid(nx)
    traj, x = dev(classical_windows(G, B, K)), xdev(G)

    def fresh():
        m = load(hf, sd128(), (4, 128, 4)).flatten_parameters_()
        return m, training.FlatAdam(m.parameters(), lr=1e-3)

    outs = []
    for _ in range(2):
        m, opt = fresh()
        loss = training.pure_unrolled_step(m, opt, traj, x, through_state=through)
        assert loss is not None and not loss.requires_grad
        outs.append((float(loss), flat_of(m)))
    m, opt = fresh()
    before = flat_of(m)
    la = training.pure_unrolled_loss(m, traj, x, through_state=through)
    opt.zero_grad()
    la.backward()
    opt.step()
    auto = flat_of(m)
    assert outs[0][0] == outs[1][0] == float(la.detach())
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][1], auto)
    assert not np.array_equal(auto, before)
    # not applicable: a model whose parameters do not share one buffer
    m2 = load(hf, sd128(), (4, 128, 4))
    assert training.pure_unrolled_step(m2, training.FlatAdam(fresh()[0].parameters()), traj, x) is None


# ------------------------------------------------------------------------ 7. trainer
def test_train_pure_gnn_unrolled(hf, tmp_path):
    from hybridflux import datagen, training
    nx = 16
    tr = datagen.generate_trajectories(nx=nx, num_initial_conditions=6, steps_per_ic=8, device=DEV)
    assert tr.shape == (6, 9, 3, nx)
    x = hf.BaselineSolver(nx, device=DEV).x
    runs = []
    for r in range(2):
        m, h = training.train_pure_gnn_unrolled(tr, x, K=4, epochs=3, batch_size=8, hidden_dim=64, num_layers=3, seed=0,
                                                device=DEV, save_dir=str(tmp_path / f"run{r}"), log=None)
        runs.append((h, flat_of(m), m))
    h = runs[0][0]
    assert sorted(h) == ["epoch", "loss", "seconds"] and h["epoch"] == [1, 2, 3]
    assert len(h["loss"]) == 3 and np.isfinite(h["loss"]).all() and np.isfinite(h["seconds"]).all()
    assert h["loss"][0] > h["loss"][1] > h["loss"][2]
    assert runs[1][0]["loss"] == h["loss"] and np.array_equal(runs[0][1], runs[1][1])
    sd = torch.load(tmp_path / "run0" / "pure_gnn_unrolled_K4.pt", map_location="cpu")
    fresh = hf.PureGNN(4, 64, 3)
    fresh.load_state_dict(sd)
    assert np.array_equal(flat_of(fresh), runs[0][1])
    ic = dev(tr[:3, 0])
    a = runs[0][2].rollout(ic, 3, x)["traj"]
    b = fresh.to(DEV).rollout(ic, 3, x)["traj"]
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert (tmp_path / "run0" / "history_pure_gnn_unrolled_K4.json").exists()


def test_other_models_refused(hf):
    from hybridflux import training
    G = O.Grid(16)
    traj, x = dev(classical_windows(G, 2, 2)), xdev(G)
    with pytest.raises(TypeError):
        training.pure_unrolled_loss(hf.FluxGNN(4, 128, 4).to(DEV), traj, x)
    with pytest.raises(TypeError):  # and FluxGNN's entry point still refuses PureGNN
        training.unrolled_loss(hf.PureGNN(4, 64, 3).to(DEV), traj, x, hf.BaselineSolver(16, device=DEV).grid)
