"""CPU-side checks of the PINN training entry points of the C ABI
(hf_pinn_tape_bytes, hf_pinn_backward_workspace_bytes,
hf_pinn_loss_workspace_bytes, hf_pinn_forward_train, hf_pinn_backward,
hf_pinn_loss): they are declared, exported and in SIGNATURES, the size queries
answer, and bad arguments are refused before any device call (no kernel is
launched here; the dummy pointers are never dereferenced), with an
hf_last_error() message that names the function."""
import ctypes
import os
import re

import numpy as np
import torch

from conftest import ROOT, close, golden
from hybridflux import _lib

D = ctypes.c_void_p(1)
NAMES = ("hf_pinn_tape_bytes", "hf_pinn_backward_workspace_bytes", "hf_pinn_loss_workspace_bytes",
         "hf_pinn_forward_train", "hf_pinn_backward", "hf_pinn_loss")


def test_declared_exported_and_in_signatures():
    with open(os.path.join(ROOT, "include", "hybridflux.h")) as f:
        header = f.read()
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\(", header), n
        assert n in _lib.SIGNATURES, n
        assert getattr(L, n) is not None, n
    with open(os.path.join(ROOT, "gnn-plasma-flux_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS :=.*\bpinn_train\.hip\b", f.read(), re.M)


def test_size_queries():
    L = _lib.lib()
    for fn in (L.hf_pinn_tape_bytes, L.hf_pinn_backward_workspace_bytes):
        assert fn(192, 256, 4, 32) > 0
        assert fn(15, 16, 2, 3) > 0
        assert fn(192, 256, 8, 32) > 0
        assert fn(192, 256, 1, 32) == -1     # < 2 layers
        assert fn(192, 256, 9, 32) == -1     # > 8 layers
        assert fn(0, 256, 4, 32) == -1
        assert fn(192, 0, 4, 32) == -1
        assert fn(192, -1, 4, 32) == -1
        assert fn(192, 256, 4, 0) == -1      # B = 0
        assert fn(192, 256, 4, -5) == -1
    # the tape holds the layers - 1 tanh activations [B][hidden], each 256-byte aligned
    assert L.hf_pinn_tape_bytes(192, 256, 4, 32) == 3 * 32 * 256 * 4
    assert L.hf_pinn_tape_bytes(15, 16, 2, 3) == 256
    assert L.hf_pinn_tape_bytes(192, 256, 5, 32) > L.hf_pinn_tape_bytes(192, 256, 4, 32)
    # the backward keeps layers - 1 gradients [B][hidden] and every layer's weight-gradient partials
    assert L.hf_pinn_backward_workspace_bytes(192, 256, 4, 32) >= \
        3 * 32 * 256 * 4 + 4 * (2 * 192 * 256 + 2 * 256 * 256)
    assert L.hf_pinn_backward_workspace_bytes(192, 256, 4, 4096) > L.hf_pinn_backward_workspace_bytes(192, 256, 4, 32)
    # the loss: an arrival counter and four float64 partial sums per IC
    assert L.hf_pinn_loss_workspace_bytes(32, 64) >= 4 + 32 * 4 * 8
    assert L.hf_pinn_loss_workspace_bytes(1, 1) > 0
    assert L.hf_pinn_loss_workspace_bytes(0, 64) == -1
    assert L.hf_pinn_loss_workspace_bytes(32, 0) == -1
    assert L.hf_pinn_loss_workspace_bytes(-1, 64) == -1


def _fwd(L, dim=192, hidden=256, layers=4, B=32, params=D, state=D, out=ctypes.c_void_p(2), tape=D):
    return L.hf_pinn_forward_train(params, dim, hidden, layers, state, B, out, tape, None)


def _bwd(L, dim=192, hidden=256, layers=4, B=32, params=D, state=D, tape=D, go=D, gp=D, gs=None, ws=D, nb=None):
    if nb is None:
        nb = int(L.hf_pinn_backward_workspace_bytes(192, 256, 4, 32))
    return L.hf_pinn_backward(params, dim, hidden, layers, state, B, tape, go, gp, gs, ws, nb, None)


def _loss(L, B=3, nx=64, dt=5e-3, dx=0.1, pred=D, st=D, sn=D, w=D, plan=D, losses=D, gp=D, ws=D, nb=None):
    if nb is None:
        nb = int(L.hf_pinn_loss_workspace_bytes(3, 64))
    return L.hf_pinn_loss(pred, st, sn, B, nx, dt, dx, 1e-3, w, plan, losses, gp, ws, nb, None)


def _refused(L, rc, fn, code=_lib.HF_EINVAL, word=None):
    assert rc == code, (fn, rc)
    msg = L.hf_last_error()
    assert fn.encode() in msg, msg
    if word:
        assert word.encode() in msg, msg


def test_forward_train_validates_before_device():
    L, fn = _lib.lib(), "hf_pinn_forward_train"
    for kw in ("params", "state", "out", "tape"):
        _refused(L, _fwd(L, **{kw: None}), fn, word="NULL")
    _refused(L, _fwd(L, B=0), fn)
    _refused(L, _fwd(L, B=-3), fn)
    _refused(L, _fwd(L, layers=1), fn, word="layers")
    _refused(L, _fwd(L, layers=9), fn, word="layers")
    _refused(L, _fwd(L, dim=0), fn)
    _refused(L, _fwd(L, hidden=0), fn)
    _refused(L, _fwd(L, hidden=-256), fn)
    _refused(L, _fwd(L, out=D), fn, word="alias")      # dev_out == dev_state


def test_backward_validates_before_device():
    L, fn = _lib.lib(), "hf_pinn_backward"
    for kw in ("params", "state", "tape", "go", "gp", "ws"):
        _refused(L, _bwd(L, **{kw: None}), fn, word="NULL")
    _refused(L, _bwd(L, B=0), fn)
    _refused(L, _bwd(L, layers=1), fn, word="layers")
    _refused(L, _bwd(L, layers=9), fn, word="layers")
    _refused(L, _bwd(L, dim=0), fn)
    _refused(L, _bwd(L, hidden=0), fn)
    need = int(L.hf_pinn_backward_workspace_bytes(192, 256, 4, 32))
    _refused(L, _bwd(L, nb=need - 1), fn, word="workspace")
    _refused(L, _bwd(L, nb=0), fn, word="workspace")


def test_loss_validates_before_device():
    L, fn = _lib.lib(), "hf_pinn_loss"
    for kw in ("pred", "st", "sn", "w", "plan", "losses", "gp", "ws"):
        _refused(L, _loss(L, **{kw: None}), fn, word="NULL")
    _refused(L, _loss(L, B=0), fn)
    _refused(L, _loss(L, nx=0), fn)
    _refused(L, _loss(L, nx=-64), fn)
    _refused(L, _loss(L, dt=0.0), fn)
    _refused(L, _loss(L, dx=0.0), fn)
    need = int(L.hf_pinn_loss_workspace_bytes(3, 64))
    _refused(L, _loss(L, nb=need - 1), fn, word="workspace")
    # nx beyond the one-workgroup-per-IC LDS plan: unsupported, not invalid
    big = int(L.hf_pinn_loss_workspace_bytes(3, 6145))
    _refused(L, _loss(L, nx=6145, nb=big), fn, code=_lib.HF_EUNSUPPORTED, word="6144")
    assert _lib.HF_EUNSUPPORTED != _lib.HF_EINVAL


def test_restatement_matches_the_reference():
    """The loss restatement that tests/test_gpu_pinn_training.py checks shapes
    against, evaluated in float64 on the fixture's first prediction with the engine's
    Poisson column (hf_poisson_coeffs, a host helper), equals the reference's own loss
    values (rtol 1e-5) and dL/dpred (the gradient gate): the formulas, the sign and
    cell-0 rule of X and the operator P are the reference's."""
    from test_gpu_pinn_training import fixture_batch, grad_close, poisson_column, restated_loss
    fx = golden("pinn_train.npz")
    dx, dt, nu = float(fx["dx"]), float(fx["dt"]), float(fx["nu"])
    st, sn = (t.double() for t in fixture_batch(fx, 0))
    pred = torch.from_numpy(fx["first_pred"]).double().requires_grad_(True)
    vals = restated_loss(pred, st, sn, dx, dt, nu, fx["weights"], poisson_column(32, 32 * dx))
    vals[0].backward()
    close(np.array([float(v.detach()) for v in vals]), fx["first_losses"], 0.0, 1e-5, what="losses")
    grad_close(pred.grad, fx["first_grad_pred"], "grad_pred")
