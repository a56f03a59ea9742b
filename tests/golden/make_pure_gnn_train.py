"""Generate tests/golden/pure_gnn_train.npz FROM THE REFERENCE (PureGNN training).

Runs ONLY in the build container (where /root/reference exists), as
make_golden.py does; the GPU box sees only the .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pure_gnn_train.py

Records (float32 unless noted), all from the reference's own PureGNN class
(scripts/training/train_pure_gnn.py:35-76) on the CPU:

init.<key>        PureGNN(4, 64, 3) under torch.manual_seed(21)
graph_nf/ei/g     a random graph (N = 64, E = 128, torch.randint edges: duplicate
                  edges, self-loops and isolated nodes occur) and an upstream
                  gradient g [64,3]
graph_delta       the reference's delta on it; graph_grad.<key>, graph_grad_nf:
                  autograd of sum(g * delta)
traj, x           classical rollouts (BaselineSolver.run, seeds 0..6, 30 steps)
batch_ic/batch_t  six batches of 32 samples: state_t = traj[ic, t], state_next
                  = traj[ic, t + 1]
adam_losses       (float64) the six batch losses of the reference's loop
                  (:112-145: per-sample graphs, the mean of per-sample MSEs,
                  torch.optim.Adam(lr=1e-3)); adam_final.<key>: the weights after
f64_*             the same computations in float64 against the float32 ones:
                  what the reference's own rounding amounts to (the tests'
                  tolerances are stated against these)
torch_version, numpy_version   the versions that made the file (kept in the file itself)
"""
import sys
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(REF / "src"))
sys.path.insert(0, str(REF))
sys.path.insert(0, str(REF / "scripts" / "training"))

import torch  # noqa: E402

torch.set_num_threads(8)

from src.baseline_solver import BaselineSolver  # noqa: E402
from src.graph_constructor import build_chain_graph  # noqa: E402
from train_pure_gnn import PureGNN  # noqa: E402


def sd_np(sd):
    return {k: v.detach().cpu().numpy() for k, v in sd.items()}


def six_steps(model, traj, bic, bt, x, dtype):
    """The reference loop's six optimizer steps on the six batches."""
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    xt = torch.as_tensor(x, dtype=dtype)
    losses = []
    for ics, ts in zip(bic, bt):
        total = 0.0
        for ic, t in zip(ics, ts):
            st, sn = torch.as_tensor(traj[ic, t], dtype=dtype), torch.as_tensor(traj[ic, t + 1], dtype=dtype)
            _, ei = build_chain_graph(traj[ic, t], x, "cpu")
            nf = torch.cat([st.permute(1, 0), xt.unsqueeze(1)], dim=1)
            pred = st.permute(1, 0) + model(nf, ei)
            total = total + torch.mean((pred - sn.permute(1, 0)) ** 2)
        total = total / len(ics)
        opt.zero_grad()
        total.backward()
        opt.step()
        losses.append(total.item())
    return np.array(losses, dtype=np.float64)


def main():
    arrs = {}
    torch.manual_seed(21)
    model = PureGNN(input_dim=4, hidden_dim=64, num_layers=3)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    arrs.update({f"init.{k}": v for k, v in sd_np(init).items()})

    # random graph: delta and autograd gradients, float32 and float64
    g = torch.Generator().manual_seed(22)
    nf = torch.randn(64, 4, generator=g)
    ei = torch.randint(0, 64, (2, 128), generator=g)
    up = torch.randn(64, 3, generator=g)
    arrs["graph_nf"], arrs["graph_ei"], arrs["graph_g"] = nf.numpy(), ei.numpy(), up.numpy()

    def graph_grads(dtype):
        m = PureGNN(4, 64, 3).to(dtype)
        m.load_state_dict({k: v.to(dtype) for k, v in init.items()})
        x_in = nf.detach().clone().to(dtype).requires_grad_(True)
        d = m(x_in, ei)
        (d * up.to(dtype)).sum().backward()
        return d.detach(), {k: p.grad for k, p in m.named_parameters()}, x_in.grad

    d32, gp32, gx32 = graph_grads(torch.float32)
    d64, gp64, gx64 = graph_grads(torch.float64)
    arrs["graph_delta"] = d32.numpy()
    arrs.update({f"graph_grad.{k}": v.numpy() for k, v in gp32.items()})
    arrs["graph_grad_nf"] = gx32.numpy()
    rel = max(float((gp32[k].double() - gp64[k]).abs().max() / gp64[k].abs().max()) for k in gp32)
    rel = max(rel, float((gx32.double() - gx64).abs().max() / gx64.abs().max()))
    arrs["f64_graph_grad_rel"] = np.float64(rel)

    # classical data and six batches of 32
    solver = BaselineSolver(nx=64)
    x = solver.x.astype(np.float32)
    traj = np.stack([solver.run(solver.initial_condition(seed=s), n_steps=30, record_flux=True)[0]
                     for s in range(7)]).astype(np.float32)
    pick = np.random.default_rng(23).permutation(7 * 30)[:192]
    bic, bt = (pick // 30).reshape(6, 32), (pick % 30).reshape(6, 32)
    arrs["traj"], arrs["x"], arrs["batch_ic"], arrs["batch_t"] = traj, x, bic.astype(np.int64), bt.astype(np.int64)

    model.load_state_dict(init)
    losses = six_steps(model, traj, bic, bt, x, torch.float32)
    arrs["adam_losses"] = losses
    arrs.update({f"adam_final.{k}": v for k, v in sd_np(model.state_dict()).items()})
    m64 = PureGNN(4, 64, 3).double()
    m64.load_state_dict({k: v.double() for k, v in init.items()})
    l64 = six_steps(m64, traj, bic, bt, x, torch.float64)
    arrs["f64_adam_loss_rel"] = np.float64(np.abs(losses - l64).max() / np.abs(l64).max())
    arrs["f64_adam_weight_abs"] = np.float64(max(
        float((model.state_dict()[k].double() - v).abs().max()) for k, v in m64.state_dict().items()))
    arrs["torch_version"] = np.array(torch.__version__)
    arrs["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT / "pure_gnn_train.npz", **arrs)
    print("wrote pure_gnn_train.npz", (OUT / "pure_gnn_train.npz").stat().st_size, "bytes")
    for k in ("f64_graph_grad_rel", "f64_adam_loss_rel", "f64_adam_weight_abs"):
        print(k, float(arrs[k]))
    print("losses", losses)


if __name__ == "__main__":
    main()
