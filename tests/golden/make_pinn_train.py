"""Generate tests/golden/pinn_train.npz FROM THE REFERENCE (PINN training).

Runs ONLY in the build container (where /root/reference exists), as
make_golden.py does; the GPU box sees only the .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pinn_train.py

Records (float32 unless noted), all from the reference's own PINN class and
loss functions (scripts/training/train_pinn.py:36-111) on the CPU:

init.<key>        PINN(96, 64, 3) under torch.manual_seed(21)
traj, dx, dt, nu  classical rollouts at nx = 32 (BaselineSolver.run, seeds 0..6,
                  30 steps) and the solver's constants (float64)
batch_ic/batch_t  six batches of 32 samples: state_t = traj[ic, t], state_next
                  = traj[ic, t + 1]
weights           the loss weights of :142-145 (float64)
first_pred        the model's prediction on the first batch; first_losses
                  (float64) = (loss, data, continuity, momentum, poisson) of
                  :163-175; first_grad.<key> = dL/dparams; first_grad_pred =
                  dL/dpred
adam_losses       (float64) [6][5]: the five loss values of the six steps of the
                  reference's loop (:156-179, torch.optim.Adam(lr=1e-3));
                  adam_final.<key>: the weights after
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
from train_pinn import PINN, compute_physics_losses  # noqa: E402

WEIGHTS = (1.0, 0.1, 0.1, 0.01)


def sd_np(sd):
    return {k: v.detach().cpu().numpy() for k, v in sd.items()}


def loss_of(model, st, sn, dx, dt, nu):
    """train_pinn.py:160-175 on one batch: (pred, loss, [data, cont, mom, pois])."""
    pred = model(st)
    data = torch.mean((pred - sn) ** 2)
    cont, mom, pois = compute_physics_losses(st, pred, dx, dt, nu)
    loss = WEIGHTS[0] * data + WEIGHTS[1] * cont + WEIGHTS[2] * mom + WEIGHTS[3] * pois
    return pred, loss, (data, cont, mom, pois)


def batches(traj, bic, bt, dtype):
    for ics, ts in zip(bic, bt):
        yield torch.as_tensor(traj[ics, ts], dtype=dtype), torch.as_tensor(traj[ics, ts + 1], dtype=dtype)


def six_steps(model, traj, bic, bt, dx, dt, nu, dtype):
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    rows = []
    for st, sn in batches(traj, bic, bt, dtype):
        _, loss, terms = loss_of(model, st, sn, dx, dt, nu)
        opt.zero_grad()
        loss.backward()
        opt.step()
        rows.append([loss.item()] + [t.item() for t in terms])
    return np.array(rows, dtype=np.float64)


def first_batch(init, traj, bic, bt, dx, dt, nu, dtype):
    m = PINN(96, 64, 3).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in init.items()})
    st, sn = next(batches(traj, bic, bt, dtype))
    pred, loss, terms = loss_of(m, st, sn, dx, dt, nu)
    pred.retain_grad()
    loss.backward()
    vals = np.array([loss.item()] + [t.item() for t in terms], dtype=np.float64)
    return pred.detach(), vals, {k: p.grad for k, p in m.named_parameters()}, pred.grad


def main():
    arrs = {}
    torch.manual_seed(21)
    model = PINN(input_dim=96, hidden_dim=64, num_layers=3)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    arrs.update({f"init.{k}": v for k, v in sd_np(init).items()})

    solver = BaselineSolver(nx=32)
    dx, dt, nu = float(solver.dx), float(solver.dt), float(solver.nu)
    traj = np.stack([solver.run(solver.initial_condition(seed=s), n_steps=30, record_flux=True)[0]
                     for s in range(7)]).astype(np.float32)
    pick = np.random.default_rng(23).permutation(7 * 30)[:192]
    bic, bt = (pick // 30).reshape(6, 32), (pick % 30).reshape(6, 32)
    arrs["traj"], arrs["batch_ic"], arrs["batch_t"] = traj, bic.astype(np.int64), bt.astype(np.int64)
    arrs["dx"], arrs["dt"], arrs["nu"] = np.float64(dx), np.float64(dt), np.float64(nu)
    arrs["weights"] = np.array(WEIGHTS, dtype=np.float64)

    p32, l32, g32, gp32 = first_batch(init, traj, bic, bt, dx, dt, nu, torch.float32)
    p64, l64, g64, gp64 = first_batch(init, traj, bic, bt, dx, dt, nu, torch.float64)
    arrs["first_pred"], arrs["first_losses"], arrs["first_grad_pred"] = p32.numpy(), l32, gp32.numpy()
    arrs.update({f"first_grad.{k}": v.numpy() for k, v in g32.items()})
    arrs["f64_first_pred_abs"] = np.float64(float((p32.double() - p64).abs().max()))
    arrs["f64_first_loss_rel"] = np.float64(np.abs((l32 - l64) / l64).max())
    rel = max(float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()) for k in g32)
    rel = max(rel, float((gp32.double() - gp64).abs().max() / gp64.abs().max()))
    arrs["f64_first_grad_rel"] = np.float64(rel)

    model.load_state_dict(init)
    rows = six_steps(model, traj, bic, bt, dx, dt, nu, torch.float32)
    arrs["adam_losses"] = rows
    arrs.update({f"adam_final.{k}": v for k, v in sd_np(model.state_dict()).items()})
    m64 = PINN(96, 64, 3).double()
    m64.load_state_dict({k: v.double() for k, v in init.items()})
    r64 = six_steps(m64, traj, bic, bt, dx, dt, nu, torch.float64)
    arrs["f64_adam_loss_rel"] = np.float64(np.abs((rows - r64) / r64).max())
    arrs["f64_adam_weight_abs"] = np.float64(max(
        float((model.state_dict()[k].double() - v).abs().max()) for k, v in m64.state_dict().items()))
    arrs["torch_version"] = np.array(torch.__version__)
    arrs["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT / "pinn_train.npz", **arrs)
    print("wrote pinn_train.npz", (OUT / "pinn_train.npz").stat().st_size, "bytes")
    for k in sorted(a for a in arrs if a.startswith("f64_")):
        print(k, float(arrs[k]))
    print("losses", rows)


if __name__ == "__main__":
    main()
