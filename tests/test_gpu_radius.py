"""The real stencil radius on the GPU: FluxGNN on the radius-R chain graph in the
fused f32 kernels (hf_model_create_ex, HybridSolver(graph_radius=R)), against
tests/radius_cases.py's exact references and the pinned oracle.

Bitwise (array equality, exact integer inputs): hf_chain_flux and its face flux
on every case; FluxGNN.forward on the radius graph (generic kernels, all
2*R*nx edges per IC); rollouts (T steps = T single steps, every step's face
flux = hf_chain_flux on that state); compare_batch = run_batch + classical run
+ traj_mse; small batches = the same ICs inside a large one; radius 1 through
hf_model_create_ex = hf_model_create; ensembles = single models; gradients
through the radius graph on an exact case.

The case table holds the regime rows too (radius_cases._regimes: depths 0..8,
window-count boundaries, the tightest window, a second pass of the persistent
loop, per-step rollouts at nx = 100 / 1024); hf_chain_flux writes them into
buffers filled with NaN, and the persistent rows assert their second pass with
the device's CU count.  The rollout body runs in the tridiagonal Poisson mode
as well.  What is not a row of the table is in tests/test_gpu_radius_regimes.py.

FluxGNN.forward on a tagged radius graph keeps the fused kernels' arithmetic on
the generic kernels (hf_graph_flux_radius: the neighbour sum in edge-list order
times W_b packed as w / (2R)), so the module and the solver share one
definition and the integer reference is met bit for bit at R = 3 too.  The
reference's own float32 mean (sum / 6, one rounding per mean: an untagged copy
of the graph, or the oracle) is NOT bitwise there, by one ulp on 2-6 of ~2000
values on 4 of the 11 R = 3 cases (measured, max 6.1e-05 on fluxes of ~5e3);
for R = 2 (degree 4) the two forms are the same bits, which
test_untagged_copy_takes_the_mean checks.

Against the oracle with random weights (hybrid_run with a flux_fn that runs
flux_gnn_forward on radius_edges and keeps the first 2nx fluxes), R = 2, 3 at
nx = 64 (persistent rollout) and nx = 100 (windowed flux kernel per step), 12
steps, at test_gpu_parity.py's own gates:
  edge fluxes, one evaluation ... atol 2e-6          (measured: see MEASURED)
  hybrid states, 12 steps ....... atol 2e-6 + rtol 2e-6
ablation_loss(graph_radius=2) against a float64 autograd restatement at
test_gpu_training.py's gates: loss rtol 1e-5, each gradient tensor
|got - ref| <= 2e-5 max|ref| + 1e-9.

MEASURED (MI355X, this file's own prints; nx = 64 / nx = 100):
  R = 2: one evaluation 2.4e-07 / 3.6e-07, states 2.4e-07 / 3.6e-07
  R = 3: one evaluation 2.1e-07 / 3.3e-07, states 2.4e-07 / 3.6e-07
  (states: max |err|; max (|err| - 2e-6 |ref|) <= 3.8e-08 against the 2e-6 gate)
  ablation_loss(graph_radius=2): loss 2.983602928e-03 against 2.983602650e-03
  in float64 (9.3e-08 relative), fused and torch forms alike.
"""
import ctypes

import numpy as np
import pytest
import torch

import exact_cases as X
import radius_cases as RC
from conftest import golden
from oracle import hybrid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLUX_ATOL = 2e-6
ROLL_ATOL, ROLL_RTOL = 2e-6, 2e-6
GRAD_REL = 2e-5


@pytest.fixture(scope="module")
def hf():
    import hybridflux
    return hybridflux


def same(got, want, nx=None, what=""):
    if hasattr(got, "detach"):
        got = got.detach().cpu().numpy()
    msg = X.mismatch(got, want, nx)
    assert msg is None, f"{what}: {msg}"


def bits(a, b, what=""):
    a, b = (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t) for t in (a, b))
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} differ"


def device_model(sd, R, precision="f32"):
    from hybridflux import engine
    return engine.DeviceModel(sd, torch.device(DEV), precision, R)


def weights(tag):
    w = golden(f"weights_{tag}.npz")
    return {k: w[k] for k in w.files}


def solver(hf, tag, R, nx=64, **kw):
    return hf.HybridSolver({k: torch.from_numpy(v) for k, v in weights(tag).items()}, R, nx=nx, device=DEV,
                           graph_radius=R, **kw)


def ics(nx, B, seed0=2000):
    G = O.Grid(nx)
    return G, np.stack([O.initial_condition(G, s) for s in range(seed0, seed0 + B)])


def int_states(case, b, T):
    """The integer state of an exact rollout case, and nothing else exact after it."""
    return torch.from_numpy(case.state0(b.nf)).to(DEV)


# --------------------------------------------------------------- 1. hf_chain_flux
@pytest.mark.parametrize("case", RC.cases("flux"), ids=lambda c: c.name)
def test_chain_flux_bitwise(hf, case):
    """hf_chain_flux into buffers filled with NaN beforehand: a flux that is never
    written (a later pass of the persistent loop, a last window) stays NaN."""
    from hybridflux import _lib, engine
    b = RC.find_case(case)
    if case.name.startswith("rpersist"):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        r = case.regime(cus)
        assert r["passes"] >= 2 and r["groups"] > cus * RC.WG_PER_CU, "no second pass of the persistent loop"
    m = device_model(b.sd, case.R)
    dev = torch.device(DEV)
    nf = torch.from_numpy(b.nf).to(dev)
    fe = torch.full((case.B * 2 * case.nx,), float("nan"), device=dev)
    ff = torch.full((case.B, case.nx), float("nan"), device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().hf_chain_flux(m.handle, _lib.ptr(nf), case.B, case.nx, _lib.ptr(fe), _lib.ptr(ff),
                                            engine.stream_of(dev)))
    same(fe.reshape(case.B, 2 * case.nx), b.flux, case.nx, f"{case.name} edges")
    same(ff, b.faces, case.nx, f"{case.name} faces")
    fe2, ff2 = engine.chain_flux(m, nf, case.B, case.nx, flux_face=True)
    bits(fe2, fe, f"{case.name} edges, engine.chain_flux")
    bits(ff2, ff, f"{case.name} faces, engine.chain_flux")


# ------------------------------------------------------------ 2. FluxGNN.forward
@pytest.mark.parametrize("case", RC.cases("flux"), ids=lambda c: c.name)
def test_module_forward_on_the_radius_graph(hf, case):
    """Generic kernels, every edge, against the integer reference: bitwise."""
    from hybridflux.graph_constructor import chain_edge_index
    b = RC.find_case(case)
    m = hf.FluxGNN(4, 128, case.layers)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in b.sd.items()})
    ei = chain_edge_index(case.nx, case.B, DEV, radius=case.R)
    with torch.no_grad():
        fe = m.to(DEV)(torch.from_numpy(b.nf).to(DEV), ei)
    assert fe.shape == (case.B * 2 * case.R * case.nx,)
    got = fe.cpu().numpy().astype(np.float64).reshape(case.B, -1)
    print(f"{case.name}: max |got - integer reference| = {float(np.abs(got - b.flux_all).max()):.3e}, max |flux| = "
          f"{float(np.abs(b.flux_all).max()):.3e}, {int((got != b.flux_all).sum())} of {got.size} differ")
    same(got, b.flux_all, None, case.name)


def test_untagged_copy_takes_the_mean(hf):
    """An untagged copy of a radius-2 graph runs hf_graph_flux (float32 mean, deg 4:
    exact), the tagged graph hf_graph_flux_radius: the same bits; and the tagged
    forward's first 2nx fluxes per IC are hf_chain_flux's."""
    from hybridflux import engine
    from hybridflux.graph_constructor import chain_edge_index
    case = RC.BY_NAME["rflux_nx48_R2_L4"]
    b = RC.find_case(case)
    m = hf.FluxGNN(4, 128, case.layers)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in b.sd.items()})
    m = m.to(DEV)
    nf = torch.from_numpy(b.nf).to(DEV)
    ei = chain_edge_index(case.nx, case.B, DEV, radius=case.R)
    with torch.no_grad():
        tagged, plain = m(nf, ei), m(nf, ei.clone())
    same(plain.reshape(case.B, -1), b.flux_all, None, "untagged")
    bits(tagged, plain, "tagged vs untagged")
    fe = engine.chain_flux(device_model(b.sd, case.R), nf, case.B, case.nx)
    bits(fe.reshape(case.B, -1), tagged.reshape(case.B, -1)[:, :2 * case.nx], "hf_chain_flux vs the module")


# -------------------------------------------------------------------- 3. rollouts
@pytest.mark.parametrize("case", RC.cases("rollout"), ids=lambda c: c.name)
def test_rollout_steps_and_face_flux_bitwise(hf, case):
    rollout_body(case)


def rollout_body(case, poisson="spectral"):
    """T steps = T single steps, every step's face flux = hf_chain_flux on that
    state, the first one the integer reference's.  nx = 16 MT: the persistent
    rollout; any other nx the per-step path (T = 6, at nx = 1024 T = 2)."""
    from hybridflux import engine
    b = RC.find_case(case)
    m = device_model(b.sd, case.R)
    grid = engine.Grid(case.nx, poisson=poisson)
    st = int_states(case, b, 6)
    x = grid.on(torch.device(DEV))[0]
    T = 2 if case.nx >= 1024 else 6
    out = engine.run(m, grid, st, T, traj=True, flux=True)
    same(out["flux"][:, 0], b.faces, case.nx, f"{case.name} first face flux")
    print(f"{case.name} {poisson}: T = {T}, max |state| = {float(out['traj'].abs().max()):.3e}")
    assert torch.isfinite(out["traj"]).all() and torch.isfinite(out["flux"]).all(), "the states left float32's range"
    cur = st
    for t in range(T):
        bits(out["traj"][:, t], cur, f"{case.name} state {t}")
        nf = torch.stack([cur[:, 0], cur[:, 1], cur[:, 2], x.expand(case.B, case.nx)], dim=-1).reshape(-1, 4)
        _, ff = engine.chain_flux(m, nf.contiguous(), case.B, case.nx, flux_face=True)
        nxt, F, _ = engine.step(m, grid, cur, flux_face=True)
        bits(F, out["flux"][:, t], f"{case.name} step {t} face flux (step vs run)")
        bits(ff, F, f"{case.name} step {t} face flux (hf_chain_flux)")
        cur = nxt
    bits(out["traj"][:, T], cur, f"{case.name} state {T}")
    bits(out["final"], cur, f"{case.name} final")


@pytest.mark.parametrize("name", ["rrollout_nx64_R2_L4", "rrollout_nx64_R3_L4", "rrollout_nx100_R2_L4",
                                  "rrollout_nx100_R3_L4"])
def test_rollout_tridiagonal_bitwise(hf, name):
    """The same body with the tridiagonal Poisson plan (engine.Grid(poisson=
    "tridiagonal"), as tests/test_gpu_tridiag.py asks for it): the persistent
    rollout at nx = 64, the per-step path at nx = 100, a radius model in both."""
    from hybridflux import engine
    case = RC.BY_NAME[name]
    rollout_body(case, poisson="tridiagonal")
    b = RC.find_case(case)                                         # the mode is really applied: E differs
    st, m = int_states(case, b, 2), device_model(b.sd, case.R)
    tri, spec = (engine.run(m, engine.Grid(case.nx, poisson=p), st, 2)["final"] for p in ("tridiagonal", "spectral"))
    assert not torch.equal(tri[:, 2], spec[:, 2])


# ------------------------------------------------------------------ 4. the oracle
@pytest.mark.parametrize("nx", [64, 100])
@pytest.mark.parametrize("R", [2, 3])
def test_rollout_vs_oracle(hf, R, nx):
    T, B = 12, 6
    s = solver(hf, f"W1_r{R}", R, nx=nx)
    G, st = ics(nx, B)
    p = O.params_from(weights(f"W1_r{R}"))

    def flux_fn(p, grid, state):
        with torch.no_grad():
            fe = O.flux_gnn_forward(p, O.node_features(grid, state),
                                    torch.from_numpy(RC.radius_edges(grid.nx, state.shape[0], R)))
        return fe.numpy().reshape(state.shape[0], 2 * R * grid.nx)[:, :2 * grid.nx]

    want, fe_want = O.hybrid_run(p, G, st, T, flux_fn=flux_fn)
    out = s.run_batch(st, T, traj=True, flux=True)
    got = out["traj"].cpu().numpy()
    from hybridflux import engine
    nf = O.node_features(G, st).to(DEV)
    fe = engine.chain_flux(s._dm(), nf, B, nx).cpu().numpy().reshape(B, 2 * nx)
    e_flux = float(np.abs(fe - fe_want[:, 0]).max())
    e_roll = float((np.abs(got - want) - ROLL_RTOL * np.abs(want)).max())
    print(f"R={R} nx={nx}: one evaluation max err {e_flux:.3e} (gate {FLUX_ATOL}); states max |err| "
          f"{float(np.abs(got - want).max()):.3e}, max (|err| - rtol |ref|) {e_roll:.3e} (gate {ROLL_ATOL})")
    assert np.isfinite(got).all()
    assert e_flux <= FLUX_ATOL
    assert e_roll <= ROLL_ATOL
    # the radius matters: the same weights on the ±1 chain give another trajectory
    one = hf.HybridSolver({k: torch.from_numpy(v) for k, v in weights(f"W1_r{R}").items()}, R, nx=nx, device=DEV)
    assert float(np.abs(one.run_batch(st, T)["traj"].cpu().numpy() - got).max()) > 1e-4


# ------------------------------------------------------------------- 5. compare
def test_compare_batch_bitwise(hf):
    from hybridflux import engine
    nx, T, B = 32, 5, 7
    s = solver(hf, "W1_r2", 2, nx=nx)
    _, st = ics(nx, B)
    c = s.compare_batch(st, T, metrics=True)
    r = s.run_batch(st, T, traj=True, metrics=True)
    cl = s.baseline.run_batch(st, T, traj=True, metrics=True)
    bits(c["final"], r["final"], "final")
    bits(c["metrics"], r["metrics"], "metrics")
    bits(c["metrics_classical"], cl["metrics"], "classical metrics")
    bits(c["mse"], engine.traj_mse(r["traj"], cl["traj"]), "mse")


# ------------------------------------------------------------ 6. small batches
@pytest.mark.parametrize("R", [2, 3])
def test_small_batch_equals_large_batch(hf, R):
    """B = 3 at nx = 64 would take the cell-split kernels at radius 1; a radius
    model must not (they trade one boundary column per layer)."""
    s = solver(hf, f"W1_r{R}", R)
    _, st = ics(64, 300)
    st = np.ascontiguousarray(st)
    big = s.run_batch(st, 4, traj=True, flux=True)
    small = s.run_batch(st[:3], 4, traj=True, flux=True)
    bits(small["traj"], big["traj"][:3], "traj")
    bits(small["flux"], big["flux"][:3], "flux")
    a, Fa, _ = s.step_batch(st[:3], return_flux=True)
    bits(a, big["traj"][:3, 1], "step")
    bits(Fa, big["flux"][:3, 0], "step flux")


# ------------------------------------------------- 7. radius 1 through the new call
def test_radius_one_is_hf_model_create(hf):
    from hybridflux import _lib, engine
    sd = weights("W1_r1")
    dev = torch.device(DEV)
    a = engine.DeviceModel(sd, dev, "f32", 1)
    b = engine.DeviceModel(sd, dev, "f32")
    with torch.cuda.device(dev):
        _lib.lib().hf_model_destroy(b.handle)
        b.handle = ctypes.c_void_p()
        flat = engine.flatten_params(sd, b.layers)
        _lib.check(_lib.lib().hf_model_create(flat.ctypes.data_as(ctypes.c_void_p), 4, 128, b.layers,
                                              _lib.HF_WDTYPE_F32, b.handle))
    assert _lib.lib().hf_model_radius(a.handle) == 1 == _lib.lib().hf_model_radius(b.handle)
    assert _lib.lib().hf_model_radius(device_model(sd, 3).handle) == 3
    for nx, B in ((64, 5), (64, 300), (100, 4)):
        grid = engine.Grid(nx)
        _, st = ics(nx, B)
        st = torch.from_numpy(st).to(dev)
        ra, rb = (engine.run(m, grid, st, 5, traj=True, flux=True) for m in (a, b))
        bits(ra["traj"], rb["traj"], f"nx {nx} B {B} traj")
        bits(ra["flux"], rb["flux"], f"nx {nx} B {B} flux")


# ------------------------------------------------------------------ 8. ensembles
def test_ensembles(hf):
    from hybridflux import evaluation
    T, B = 5, 9
    _, st = ics(64, B)
    a, b = solver(hf, "W1_r2", 2), solver(hf, "W0", 2)
    ens = hf.HybridEnsemble([a, b])
    r = ens.run_batch(st, T, traj=True, flux=True, metrics=True)
    c = ens.compare_batch(st, T)
    for i, s in enumerate((a, b)):
        ri, ci = s.run_batch(st, T, traj=True, flux=True, metrics=True), s.compare_batch(st, T)
        for k in ("final", "traj", "flux", "metrics"):
            bits(r[k][i], ri[k], f"run model {i} {k}")
        for k in ("final", "mse", "metrics", "metrics_classical"):
            bits(c[k][i], ci[k], f"compare model {i} {k}")
    with pytest.raises(ValueError, match="graph_radius"):
        hf.HybridEnsemble([a, solver(hf, "W1_r3", 3)])
    models = {"r1": solver(hf, "W1_r1", 1), "r2a": a, "r2b": b, "r3": solver(hf, "W1_r3", 3)}
    got = evaluation.compare_models(models, st, T)
    want = evaluation.compare_models(models, st, T, grouped=False)
    assert got == want and list(got) == list(models)
    for k, s in models.items():
        per_ic = evaluation.multi_ic_mse(s, st, T)[0].to(torch.float64).cpu().numpy()
        assert got[k]["mse_per_ic"] == [float(v) for v in per_ic], k
    assert got["r2a"]["mse_per_ic"] != got["r2b"]["mse_per_ic"]


# ------------------------------------------------------------------- 9. training
def test_gradients_through_the_radius_graph_bitwise(hf):
    """Exact case at R = 2 (nx = 16, B = 5): FluxGNN's autograd Function on the
    generic kernels; the upstream gradient is zero on the long edges."""
    from hybridflux.graph_constructor import chain_edge_index
    case = RC.BY_NAME["rflux_nx16_R2_L4"]
    b = RC.find_case(case)
    E = b.ei.shape[1]
    gup = X.upstream(E, b.seed).reshape(case.B, -1)
    gup[:, 2 * case.nx:] = 0
    gup = np.ascontiguousarray(gup.reshape(-1))
    flux64, grads, grec = X.grads64(b.sd, b.nf, case.B, case.nx, gup, edge_index=b.ei)
    assert grec.valid("f32") and np.array_equal(flux64.reshape(case.B, -1), b.flux_all)
    m = hf.FluxGNN(4, 128, case.layers)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in b.sd.items()})
    m = m.to(DEV)
    nf = torch.from_numpy(b.nf).to(DEV).requires_grad_(True)
    flux = m(nf, chain_edge_index(case.nx, case.B, DEV, radius=case.R))
    (flux * torch.from_numpy(gup).to(DEV)).sum().backward()
    same(flux, flux64, None, "flux")
    for k, q in m.named_parameters():
        same(q.grad, grads[k], None, f"d {k}")
    same(nf.grad, grads["node_features"], None, "d node_features")


def _loss64(sd, st, ft, sn, G, cfg, R):
    """ablation_loss (no rollout term) restated in float64 torch autograd on the
    radius graph: the model's forward on radius_edges, the first 2nx fluxes, the
    torch expressions of training.ablation_loss with a detached float64 Poisson."""
    f64 = torch.float64
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in sd.items()}
    B, _, nx = st.shape
    x = torch.from_numpy(O.node_features(G, st).numpy().astype(np.float64))
    ei = torch.from_numpy(RC.radius_edges(nx, B, R))
    row, col = ei[0], ei[1]
    lin = torch.nn.functional.linear
    h = torch.relu(lin(x, p["input_mlp.0.weight"], p["input_mlp.0.bias"]))
    deg = torch.bincount(row, minlength=h.shape[0]).to(f64).unsqueeze(-1)
    for l in range(X.n_layers(sd)):
        agg = torch.zeros_like(h).index_add_(0, row, h[col]) / deg
        h = torch.relu(lin(torch.cat([h, agg], -1), p[f"update_mlps.{l}.0.weight"], p[f"update_mlps.{l}.0.bias"]))
    z = torch.relu(lin(torch.cat([h[row], h[col]], -1), p["edge_mlp.0.weight"], p["edge_mlp.0.bias"]))
    fe = lin(z, p["edge_mlp.2.weight"], p["edge_mlp.2.bias"]).squeeze(-1).reshape(B, 2 * R * nx)[:, :2 * nx]
    st, ft, sn = (torch.from_numpy(np.asarray(a, np.float64)) for a in (st, ft, sn))
    mse = lambda a, c: torch.mean((a - c) ** 2)
    F = 0.5 * (fe[:, :nx] + fe[:, nx:])
    flux_loss = mse(F, ft)
    n_next = st[:, 0] - (G.dt / G.dx) * (F - torch.roll(F, 1, dims=-1))
    loss = flux_loss + cfg["lambda_state"] * mse(n_next, sn[:, 0])
    rho_hat = np.fft.fft(n_next.detach().numpy() - 1.0, axis=-1)
    E_hat = np.zeros_like(rho_hat)
    keep = G.k != 0
    E_hat[..., keep] = 1j * rho_hat[..., keep] / G.k[keep]
    E_pred = torch.from_numpy(np.real(np.fft.ifft(E_hat, axis=-1)))
    loss = loss + cfg["lambda_poisson"] * mse(E_pred, sn[:, 2])
    loss = loss + cfg["lambda_charge"] * mse(torch.sum(n_next - 1.0, -1) * G.dx, torch.sum(st[:, 0] - 1.0, -1) * G.dx)
    e_p = 0.5 * torch.mean(sn[:, 1] ** 2 + E_pred ** 2, -1)
    e_t = 0.5 * torch.mean(sn[:, 1] ** 2 + sn[:, 2] ** 2, -1)
    loss = loss + cfg["lambda_energy_one"] * mse(e_p, e_t)
    loss.backward()
    return float(loss.detach()), float(flux_loss.detach()), {k: v.grad.numpy() for k, v in p.items()}


def test_ablation_loss_radius_vs_float64(hf):
    from hybridflux.training import ablation_loss
    R, nx = 2, 64
    cl = golden("classical.npz")
    S, Fl = cl["b16_states"], cl["b16_fluxes"]
    picks = [(0, 3), (5, 17), (9, 28), (12, 8)]
    st, ft, sn = (np.stack([a[ic, t + d] for ic, t in picks]) for a, d in ((S, 0), (Fl, 0), (S, 1)))
    sd = weights("W1_r2")
    cfg = hf.ABLATION_CONFIGS["physics"]
    G = O.Grid(nx)
    want, want_fl, grads = _loss64(sd, st, ft, sn, G, cfg, R)
    m = hf.FluxGNN(4, 128, 4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV)
    base = hf.BaselineSolver(nx, device=DEV)
    x = torch.as_tensor(base.x, dtype=torch.float32, device=DEV)
    t = [torch.as_tensor(a, device=DEV) for a in (st, ft, sn)]
    for fused in (True, False):
        m.zero_grad()
        loss, fl = ablation_loss(m, t[0], t[1], t[2], x, base.dt, base.dx, cfg, base.grid, fused=fused, graph_radius=R)
        loss.backward()
        print(f"fused={fused}: loss {loss.item():.9e} vs {want:.9e}, flux loss {fl.item():.9e} vs {want_fl:.9e}")
        assert abs(loss.item() - want) <= 1e-5 * abs(want) and abs(fl.item() - want_fl) <= 1e-5 * abs(want_fl)
        for k, q in m.named_parameters():
            g = q.grad.detach().cpu().numpy().astype(np.float64)
            scale, err = float(np.abs(grads[k]).max()), float(np.abs(g - grads[k]).max())
            assert err <= GRAD_REL * scale + 1e-9, (k, err, scale)
    # the radius matters here too
    m.zero_grad()
    one, _ = ablation_loss(m, t[0], t[1], t[2], x, base.dt, base.dx, cfg, base.grid)
    assert abs(one.item() - want) > 1e-3 * abs(want)


def test_train_model_takes_the_radius(hf, tmp_path):
    """Two epochs of train_model(graph_radius=2): the autograd step runs (the
    direct step declines), the loss is finite and falls, the checkpoint keeps its
    name, keys and shapes and loads into HybridSolver(graph_radius=2)."""
    from hybridflux import training
    cl = golden("classical.npz")
    S, Fl = cl["b16_states"], cl["b16_fluxes"]
    st, ft, sn = S[:4, :8].reshape(-1, 3, 64), Fl[:4, :8].reshape(-1, 64), S[:4, 1:9].reshape(-1, 3, 64)
    base = hf.BaselineSolver(64, device=DEV)
    assert training.direct_step(None, None, None, None, None, None, None, 0, 0, None, None, graph_radius=2) is None
    model, hist = training.train_model(st, ft, sn, base.x, base.dt, base.dx, 1e-3, "physics", 2, epochs=2, lr=1e-3,
                                       device=DEV, batch_size=8, seed=0, save_dir=str(tmp_path), log=None,
                                       graph_radius=2)
    assert np.isfinite(hist["loss"]).all() and hist["loss"][1] < hist["loss"][0]
    path = tmp_path / "hybrid_physics_r2.pt"
    sd = torch.load(path, map_location="cpu", weights_only=True)
    ref = hf.FluxGNN(4, 128, 4).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    s = hf.HybridSolver(str(path), 2, device=DEV, graph_radius=2)
    assert torch.isfinite(s.run_batch(S[:3, 0], 3)["final"]).all()


# ------------------------------------------------------------------ 10. refusals
def test_refusals(hf):
    from hybridflux import _lib, engine, training
    sd = weights("W1_r2")
    for prec in ("bf16", "f16x3"):
        with pytest.raises(_lib.HybridFluxError) as e:
            device_model(sd, 2, prec)
        assert e.value.code == _lib.HF_EUNSUPPORTED
    with pytest.raises(_lib.HybridFluxError) as e:
        device_model(sd, 4)
    assert e.value.code == _lib.HF_EINVAL
    m = device_model(sd, 3)
    dev = torch.device(DEV)
    with pytest.raises(_lib.HybridFluxError) as e:
        engine.chain_flux(m, torch.zeros(2 * 6, 4, device=dev), 2, 6)
    assert e.value.code == _lib.HF_EINVAL and "2R + 1" in str(e.value)
    grid = engine.Grid(6)
    st = torch.ones(2, 3, 6, device=dev)
    for call in (lambda: engine.step(m, grid, st), lambda: engine.run(m, grid, st, 2),
                 lambda: engine.run_compare(m, grid, st, 2)):
        with pytest.raises(_lib.HybridFluxError) as e:
            call()
        assert e.value.code == _lib.HF_EINVAL
    engine.chain_flux(m, torch.zeros(2 * 7, 4, device=dev), 2, 7)          # nx = 7 is the smallest legal chain
    with pytest.raises(ValueError, match="one radius"):                     # a set of two radii
        engine.DeviceModelSet([device_model(sd, 2), m])
    a, b = device_model(sd, 2), m
    arr = (ctypes.c_void_p * 2)(a.handle.value, b.handle.value)
    out = ctypes.c_void_p()
    assert _lib.lib().hf_model_set_create(arr, 2, out) == _lib.HF_EUNSUPPORTED
    with pytest.raises(ValueError, match="graph_radius"):
        training.train_unrolled(np.zeros((2, 6, 3, 64), np.float32), np.zeros(64), 5e-3, 0.1, 1e-3, K=4,
                                device=DEV, save_dir=None, graph_radius=2)
