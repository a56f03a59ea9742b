"""CPU-side checks of PINN's unrolled-training entry points of the C ABI
(hf_pinn_unroll_workspace_bytes, hf_pinn_unroll_loss, hf_pinn_unroll_adjoint):
the symbols, the size query, and that bad arguments are refused before any
device call with the function's name in hf_last_error() (no kernel is launched
here; the dummy pointers are never dereferenced), as test_abi_pure_unroll_cpu.py
does for PureGNN's."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from hybridflux import _lib


def P(v):
    return ctypes.c_void_p(v)


W = np.ones(3, dtype=np.float32)
WP = W.ctypes.data_as(ctypes.c_void_p)
LAM = np.asarray([0.1, 0.1, 0.01], dtype=np.float32)
LP = LAM.ctypes.data_as(ctypes.c_void_p)
NAMES = ("hf_pinn_unroll_workspace_bytes", "hf_pinn_unroll_loss", "hf_pinn_unroll_adjoint")


def test_declared_exported_and_in_signatures():
    with open(os.path.join(ROOT, "include", "hybridflux.h")) as f:
        header = f.read()
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\(", header), n
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    with open(os.path.join(ROOT, "gnn-plasma-flux_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS :=.*\bpinn_unroll\.hip\b", f.read(), re.M)


def test_workspace_query():
    L = _lib.lib()
    for B, nx in ((3, 16), (4096, 64), (2, 300), (1, 1), (2, 6144)):
        assert L.hf_pinn_unroll_workspace_bytes(B, nx) > 0
    assert L.hf_pinn_unroll_workspace_bytes(32, 64) >= 4 + 32 * 4 * 8          # a counter, four float64 partials per IC
    assert L.hf_pinn_unroll_workspace_bytes(2 ** 31 - 1, 64) > 4 * 8 * (2 ** 31 - 1)   # no int overflow
    assert L.hf_pinn_unroll_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) > 4 * 8 * (2 ** 31 - 1)
    for B, nx in ((0, 64), (3, 0), (-1, 64), (3, -7), (-2 ** 31, -2 ** 31)):
        assert L.hf_pinn_unroll_workspace_bytes(B, nx) == -1


def _loss(L, B=3, nx=16, ws_short=0, dt=5e-3, dx=0.1, **kw):
    a = dict(pred=P(16), st=P(32), tg=P(48), w=WP, phys=LP, plan=P(64), losses=P(80), ws=P(256))
    a.update(kw)
    nb = int(L.hf_pinn_unroll_workspace_bytes(max(B, 1), max(nx, 1))) - ws_short
    return L.hf_pinn_unroll_loss(a["pred"], a["st"], a["tg"], B, nx, a["w"], 1.0, a["phys"], 1.0, dt, dx, 1e-3,
                                 a["plan"], a["losses"], a["ws"], nb, None)


def _adjoint(L, B=3, nx=16, dt=5e-3, dx=0.1, **kw):
    a = dict(pred=P(16), st=P(32), tg=P(48), nxt=P(96), carry=P(112), w=WP, phys=LP, plan=P(64), g=P(128))
    a.update(kw)
    return L.hf_pinn_unroll_adjoint(a["pred"], a["st"], a["tg"], a["nxt"], a["carry"], B, nx, a["w"], 1.0, a["phys"],
                                    1.0, dt, dx, 1e-3, a["plan"], a["g"], None)


def _refused(L, rc, name, word=None, code=_lib.HF_EINVAL):
    assert rc == code, (name, rc)
    err = L.hf_last_error()
    assert name in err, err
    if word:
        assert word in err, err


def test_loss_validates_before_device():
    L, name = _lib.lib(), b"hf_pinn_unroll_loss"
    for kw in ("pred", "tg", "w", "losses", "ws"):            # every required pointer
        _refused(L, _loss(L, **{kw: None}), name, b"NULL")
    for kw in ("plan", "st"):                                  # required once phys is given
        _refused(L, _loss(L, **{kw: None}), name, b"phys")
    for B in (0, -2, -2 ** 31):
        _refused(L, _loss(L, B=B), name)
    for nx in (0, -1, -2 ** 31):
        _refused(L, _loss(L, nx=nx), name)
    _refused(L, _loss(L, dt=0.0), name)
    _refused(L, _loss(L, dx=-1.0), name)
    _refused(L, _loss(L, ws_short=1), name, b"workspace")
    _refused(L, _loss(L, nx=6145), name, b"6144", code=_lib.HF_EUNSUPPORTED)
    _refused(L, _loss(L, nx=6145, phys=None, st=None, plan=None), name, b"6144", code=_lib.HF_EUNSUPPORTED)


def test_adjoint_validates_before_device():
    L, name = _lib.lib(), b"hf_pinn_unroll_adjoint"
    for kw in ("pred", "tg", "w", "g"):                        # every required pointer
        _refused(L, _adjoint(L, **{kw: None}), name, b"NULL")
    for kw in ("plan", "st"):
        _refused(L, _adjoint(L, **{kw: None}), name, b"phys")
    for B in (0, -1, -2 ** 31):
        _refused(L, _adjoint(L, B=B), name)
    for nx in (0, -4, -2 ** 31):
        _refused(L, _adjoint(L, nx=nx), name)
    for kw in ("pred", "st", "tg", "nxt", "carry"):            # dev_grad_out aliasing any input
        _refused(L, _adjoint(L, **{kw: P(128)}), name, b"alias")
    _refused(L, _adjoint(L, nx=6145), name, b"6144", code=_lib.HF_EUNSUPPORTED)


def test_pinn_unrolled_flop_model():
    """K times the one-step count, plus the first layer's data gradient for the
    K - 1 steps that hand a state gradient back."""
    from hybridflux.training import pinn_train_flop_per_sample, pinn_unrolled_train_flop_per_sample
    one = pinn_train_flop_per_sample()
    assert pinn_unrolled_train_flop_per_sample(1) == one
    assert pinn_unrolled_train_flop_per_sample(4) == 4 * one + 3 * 2 * 192 * 256
    assert pinn_unrolled_train_flop_per_sample(2, D=48, H=64, L=3) == 2 * pinn_train_flop_per_sample(48, 64, 3) + 2 * 48 * 64


def test_python_layer_refuses_bad_calls():
    """pinn_unrolled_loss is PINN's; dx, dt, nu go with physics_weights exactly."""
    import torch

    import hybridflux
    from hybridflux import training
    traj = torch.zeros(2, 3, 3, 16)
    with pytest.raises(TypeError):
        training.pinn_unrolled_loss(hybridflux.PureGNN(4, 64, 1), traj)
    with pytest.raises(ValueError):
        training.pinn_unrolled_loss(hybridflux.PINN(48, 32, 2), traj, physics_weights=(0.1, 0.1, 0.01))
    with pytest.raises(ValueError):
        training.pinn_unrolled_loss(hybridflux.PINN(48, 32, 2), traj, dx=0.1, dt=5e-3, nu=1e-3)
    with pytest.raises(ValueError):
        training.pinn_unrolled_loss(hybridflux.PINN(48, 32, 2), traj, 0.1, 5e-3, 1e-3, physics_weights=(0.1, 0.1))
    assert training.pinn_unrolled_step(hybridflux.PureGNN(4, 64, 1), None, traj) is None
    assert training.pure_unrolled_step(hybridflux.PINN(48, 32, 2), None, traj, torch.zeros(16)) is None
