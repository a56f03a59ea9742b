"""GPU parity of PureGNN training (scripts/training/train_pure_gnn.py:59-151):
the HIP training forward / backward (hf_pure_gnn_forward_train /
hf_pure_gnn_backward) behind PureGNN's autograd Function, the fused loss
(hf_state_mse) and the batched trainer, against the reference's own autograd
and Adam run (tests/golden/pure_gnn_train.npz, made by make_pure_gnn_train.py)
and torch-CPU autograd of the oracle restatement.

Gates.  Gradients: the project's gradient gate (test_gpu_training.py),
  |got - ref| <= 2e-5 * max|ref| + 1e-9 per tensor;
the reference's own float32 autograd differs from a float64 evaluation by
6.1e-7 * max|ref| on the fixture's graph (f64_graph_grad_rel in the fixture),
so the gate leaves ~30x over the reference's rounding.  Forward values: the
forward gate of test_gpu_baselines.py (atol 2e-6 + rtol 1e-5).  Loss values:
rtol 1e-5.  Six Adam steps: per-step loss rtol 1e-4, final weights atol 2e-5
with no element left out (the reference alone, float32 against float64 over
the six steps: loss rel 9.3e-7, weights max abs 5.9e-8; f64_adam_* in the
fixture).
"""
import numpy as np
import pytest
import torch

from conftest import close, golden
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2e-5


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    return hybridflux


@pytest.fixture(scope="module")
def fx():
    return golden("pure_gnn_train.npz")


def grad_gate(record, request, what, got, want, rel=REL):
    """The gradient gate; the measured error as a fraction of max|ref| is recorded."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    record(request.node.nodeid.split("::", 1)[-1], f"{what}_rel_err", err / scale if scale > 0 else err)
    assert np.isfinite(got).all(), what
    assert err <= rel * scale + 1e-9, (what, err, scale)


def fixture_model(hf, fx, prefix="init."):
    m = hf.PureGNN(4, 64, 3)
    m.load_state_dict({k[len(prefix):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(prefix)})
    return m


@pytest.mark.parametrize("where", ["device", "host"])
def test_random_graph_vs_reference(hf, fx, record, request, where):
    """delta and d sum(g * delta) / d (params, node_features) on the fixture's random
    graph (duplicate edges, self-loops, isolated nodes) equal the reference's, with
    everything on the device and with host tensors and a CPU-resident module
    (the gradients then land on the CPU)."""
    dev = DEV if where == "device" else "cpu"
    m = fixture_model(hf, fx).to(dev)
    nf = torch.as_tensor(fx["graph_nf"], device=dev).requires_grad_(True)
    ei = torch.as_tensor(fx["graph_ei"], device=dev)
    delta = m(nf, ei)
    assert delta.requires_grad and delta.shape == (64, 3) and delta.device.type == torch.device(dev).type
    close(delta, fx["graph_delta"], 2e-6, 1e-5, what="delta")
    (delta * torch.as_tensor(fx["graph_g"], device=dev)).sum().backward()
    assert nf.grad.device.type == torch.device(dev).type
    grad_gate(record, request, "nf", nf.grad, fx["graph_grad_nf"])
    for k, p in m.named_parameters():
        assert p.grad.device == p.device, k
        grad_gate(record, request, k, p.grad, fx[f"graph_grad.{k}"])


def test_reference_smoke_test_lines(hf):
    """examples/smoke_test.py:98-104 verbatim (grad enabled, host tensors, a CPU module)."""
    torch.manual_seed(0)
    model = hf.PureGNN(input_dim=4, hidden_dim=64, num_layers=3)
    node_features = torch.randn(64, 4)
    edge_index = torch.randint(0, 64, (2, 128))
    delta_state = model(node_features, edge_index)
    assert delta_state.shape == (64, 3), f"Wrong delta shape: {delta_state.shape}"
    assert delta_state.requires_grad and torch.isfinite(delta_state).all()


def oracle_grads(sd, nf, ei, up, want_nf=True):
    """torch-CPU autograd of the oracle restatement: (delta, param grads, nf grad)."""
    p = {k: v.clone().requires_grad_(True) for k, v in O.params_from(sd).items()}
    x = torch.from_numpy(nf).clone().requires_grad_(want_nf)
    d = O.pure_gnn_forward(p, x, ei)
    (d * up).sum().backward()
    return d.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()}, x.grad.numpy() if want_nf else None


CHAIN_CASES = [  # H, nx, L, B, in_dim
    (64, 16, 3, 9, 4),     # chain GEMMs, N = 144: a full and a partial 128-row tile
    (128, 64, 4, 3, 4),    # two chains per tile, wrap inside a tile
    (64, 128, 2, 2, 4),    # one chain per tile
    (64, 64, 3, 9, 4),     # N = 576: more than one weight-gradient split
    (192, 32, 1, 5, 4),    # H not a power of two
    (64, 48, 3, 3, 4),     # nx does not divide 128: generic path
    (128, 100, 2, 2, 4),   # nx does not divide 128: generic path
    (32, 16, 2, 3, 4),     # H % 64 != 0: generic path
    (64, 32, 0, 2, 4),     # no message layer
    (64, 1, 1, 3, 4),      # a cell that is its own neighbour
    (64, 2, 1, 4, 4),      # very short chain
    (64, 16, 2, 3, 3),     # input_dim = 3
]


def chain_case(hf, H, nx, L, B, F):
    torch.manual_seed(1000 * H + 10 * nx + L)
    m = hf.PureGNN(F, H, L).to(DEV)
    g = np.random.default_rng(H + nx + L + B)
    nf = g.normal(0, 1, (B * nx, F)).astype(np.float32)
    up = torch.from_numpy(g.normal(0, 1, (B * nx, 3)).astype(np.float32))
    return m, nf, up


def run_backward(m, nf, ei, up, nf_grad=True):
    m.zero_grad()
    x = torch.as_tensor(nf, device=DEV).requires_grad_(nf_grad)
    d = m(x, ei)
    (d * up.to(DEV)).sum().backward()
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    return d.detach().cpu().numpy(), grads, x.grad.cpu().numpy() if nf_grad else None


@pytest.mark.parametrize("H,nx,L,B,F", CHAIN_CASES)
def test_chains_vs_oracle(hf, record, request, H, nx, L, B, F):
    """B tagged chains (the chain GEMMs where nx | 128 and H % 64 == 0, else the
    generic kernels with arithmetic neighbours) and an untagged clone (the generic
    kernels on CSR buckets), both against torch-CPU autograd of the oracle."""
    m, nf, up = chain_case(hf, H, nx, L, B, F)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    wd, wg, wnf = oracle_grads(sd, nf, O.chain_edges(nx, B), up)
    eit = hf.chain_edge_index(nx, B, DEV)
    for tag, ei in (("tagged", eit), ("untagged", eit.clone())):
        d, grads, gnf = run_backward(m, nf, ei, up)
        close(d, wd, 2e-6, 1e-5, what=f"{tag}_delta")
        grad_gate(record, request, f"{tag}_nf", gnf, wnf)
        for k in wg:
            grad_gate(record, request, f"{tag}_{k}", grads[k], wg[k])


def test_features_without_grad(hf):
    """Node features with requires_grad=False: no feature gradient is computed and
    the parameter gradients are the same bits."""
    m, nf, up = chain_case(hf, 64, 16, 3, 9, 4)
    ei = hf.chain_edge_index(16, 9, DEV)
    _, g1, gnf1 = run_backward(m, nf, ei, up, True)
    _, g0, gnf0 = run_backward(m, nf, ei, up, False)
    assert gnf1 is not None and gnf0 is None
    for k in g1:
        assert np.array_equal(g1[k], g0[k]), k


def test_backward_deterministic(hf, fx):
    """Two backward passes of a chain case (chain GEMMs, three weight-gradient
    splits) and of the random graph are bitwise equal."""
    m, nf, up = chain_case(hf, 64, 64, 3, 9, 4)
    ei = hf.chain_edge_index(64, 9, DEV)
    a, b = run_backward(m, nf, ei, up), run_backward(m, nf, ei, up)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k
    m = fixture_model(hf, fx).to(DEV)
    ei, up = torch.as_tensor(fx["graph_ei"], device=DEV), torch.from_numpy(fx["graph_g"])
    a, b = run_backward(m, fx["graph_nf"], ei, up), run_backward(m, fx["graph_nf"], ei, up)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k


def test_training_forward_equals_inference(hf, fx):
    """Under autograd delta equals the no_grad forward's within the forward gate;
    it is bitwise equal on every path, because the training forward issues the
    inference forward's launches with the same arithmetic (the chain GEMMs with
    the message epilogue on tagged chains with nx | 128 and H % 64 == 0; the
    generic linear + gather kernels with arithmetic neighbours on other tagged
    chains, and with CSR buckets on other graphs)."""
    cases = []
    for H, nx, L, B in ((128, 64, 4, 3), (64, 48, 3, 3)):
        m, nf, _ = chain_case(hf, H, nx, L, B, 4)
        eit = hf.chain_edge_index(nx, B, DEV)
        cases += [(m, nf, eit), (m, nf, eit.clone())]
    cases.append((fixture_model(hf, fx).to(DEV), fx["graph_nf"], torch.as_tensor(fx["graph_ei"], device=DEV)))
    for i, (m, nf, ei) in enumerate(cases):
        x = torch.as_tensor(nf, device=DEV)
        train = m(x, ei)
        assert train.requires_grad
        with torch.no_grad():
            infer = m(x, ei)
        assert not infer.requires_grad
        close(train, infer.cpu().numpy(), 2e-6, 1e-5, what=f"case{i}")
        assert torch.equal(train.detach(), infer), i


@pytest.mark.parametrize("B,nx", [(1, 16), (32, 64), (7, 100)])
def test_state_mse_loss_vs_torch(hf, record, request, B, nx):
    """state_mse_loss and its gradient against the torch expression on the CPU."""
    from hybridflux.training import state_mse_loss
    g = np.random.default_rng(B + nx)
    st = torch.from_numpy(g.normal(0, 1, (B, 3, nx)).astype(np.float32))
    sn = st + torch.from_numpy(g.normal(0, 0.1, (B, 3, nx)).astype(np.float32))
    delta = torch.from_numpy(g.normal(0, 0.1, (B * nx, 3)).astype(np.float32))
    dref = delta.clone().requires_grad_(True)
    want = ((st.permute(0, 2, 1).reshape(-1, 3) + dref - sn.permute(0, 2, 1).reshape(-1, 3)) ** 2).mean()
    want.backward()
    d = delta.to(DEV).requires_grad_(True)
    loss = state_mse_loss(d, st.to(DEV), sn.to(DEV))
    assert loss.shape == () and loss.requires_grad
    loss.backward()
    close(loss, want.detach().numpy(), 0.0, 1e-5, what="loss")
    grad_gate(record, request, "d_delta", d.grad, dref.grad.numpy())
    # an upstream factor scales the gradient
    d2 = delta.to(DEV).requires_grad_(True)
    (3.0 * state_mse_loss(d2, st.to(DEV), sn.to(DEV))).backward()
    grad_gate(record, request, "d_delta_x3", d2.grad, 3.0 * dref.grad.numpy())


def _batches(fx):
    traj, bic, bt = fx["traj"], fx["batch_ic"], fx["batch_t"]
    return [(torch.as_tensor(traj[bic[j], bt[j]], device=DEV), torch.as_tensor(traj[bic[j], bt[j] + 1], device=DEV))
            for j in range(6)]


@pytest.mark.parametrize("optim", ["flat_adam", "torch_adam"])
def test_six_adam_steps_vs_reference(hf, fx, record, request, optim):
    """The trainer's step (pure_gnn_step: one batched forward + backward over a
    tagged chain_edge_index, the fused loss, the optimizer) on the fixture's six
    batches of 32 samples, with FlatAdam on flattened parameters and with
    torch.optim.Adam, against the reference's own loop (32 per-sample graph calls
    per batch, torch.optim.Adam(lr=1e-3)): per-step loss rtol 1e-4, final weights
    atol 2e-5, every element.  The reference alone, float32 against float64 over
    the six steps (measured by the generator): loss rel 9.3e-7, weights max abs
    5.9e-8."""
    from hybridflux.training import FlatAdam, pure_gnn_step
    m = fixture_model(hf, fx).to(DEV)
    if optim == "flat_adam":
        opt = FlatAdam(m.flatten_parameters_().parameters(), lr=1e-3)
    else:
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x = torch.as_tensor(fx["x"], device=DEV)
    losses = [float(pure_gnn_step(m, opt, st, sn, x)) for st, sn in _batches(fx)]
    close(np.array(losses), fx["adam_losses"], 0.0, 1e-4, what="losses")
    sd = m.state_dict()
    worst = 0.0
    for k in sd:
        worst = max(worst, close(sd[k], fx[f"adam_final.{k}"], 2e-5, 0.0, what=k))
    record(request.node.nodeid.split("::", 1)[-1], "weights_max_abs", worst)


def test_train_pure_gnn_smoke(hf, fx):
    """train_pure_gnn: 2 epochs on 80 samples, batch size 32 (a partial last
    batch), a fixed order; the history has 2 finite losses, the second lower;
    the returned state dict loads into a fresh module and reproduces rollout()."""
    from hybridflux.training import train_pure_gnn
    traj, bic, bt = fx["traj"], fx["batch_ic"].reshape(-1)[:80], fx["batch_t"].reshape(-1)[:80]
    st, sn = traj[bic, bt], traj[bic, bt + 1]
    order = [np.arange(80), np.arange(80)[::-1].copy()]
    model, hist = train_pure_gnn(st, sn, fx["x"], epochs=2, lr=1e-3, batch_size=32, hidden_dim=64, num_layers=3,
                                 device=DEV, order=order, seed=5)
    assert list(hist) == ["loss"] and len(hist["loss"]) == 2
    assert all(np.isfinite(v) for v in hist["loss"]) and hist["loss"][1] < hist["loss"][0]
    fresh = hf.PureGNN(4, 64, 3)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    ics = torch.as_tensor(traj[:3, 0], device=DEV)
    a = model.rollout(ics, 3, fx["x"])["traj"]
    b = fresh.to(DEV).rollout(ics, 3, fx["x"])["traj"]
    assert torch.isfinite(a).all() and torch.equal(a, b)
