"""CPU-side checks of PureGNN's unrolled-training entry points of the C ABI
(hf_pure_unroll_workspace_bytes, hf_pure_unroll_update, hf_pure_unroll_adjoint):
the symbols, the size query, and that bad arguments are refused before any
device call with the function's name in hf_last_error() (no kernel is launched
here; the dummy pointers are never dereferenced), as test_abi_unroll_cpu.py
does for FluxGNN's."""
import ctypes

import numpy as np

from hybridflux import _lib

D = ctypes.c_void_p(1)
W = np.ones(3, dtype=np.float32)
WP = W.ctypes.data_as(ctypes.c_void_p)
NAMES = ("hf_pure_unroll_workspace_bytes", "hf_pure_unroll_update", "hf_pure_unroll_adjoint")


def test_symbols_exported():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(L, n), n


def test_workspace_query():
    L = _lib.lib()
    for B, nx in ((3, 16), (4096, 64), (3, 256), (2, 1030), (1, 1)):
        assert L.hf_pure_unroll_workspace_bytes(B, nx) > 0
    assert L.hf_pure_unroll_workspace_bytes(4096, 64) >= 4096 * 8      # one float64 partial per workgroup
    assert L.hf_pure_unroll_workspace_bytes(3, 10000) >= 3 * 10 * 8    # ten tiles of 1024 cells per IC
    assert L.hf_pure_unroll_workspace_bytes(2 ** 31 - 1, 1024) > 8 * (2 ** 31 - 1)   # no int overflow
    assert L.hf_pure_unroll_workspace_bytes(0, 64) == -1
    assert L.hf_pure_unroll_workspace_bytes(3, 0) == -1
    assert L.hf_pure_unroll_workspace_bytes(-1, 64) == -1
    assert L.hf_pure_unroll_workspace_bytes(3, -7) == -1
    assert L.hf_pure_unroll_workspace_bytes(2 ** 31 - 1, 1025) == -1   # more workgroups than a grid holds


def _update(L, B=3, nx=16, ws_short=0, **kw):
    a = dict(delta=D, st=D, x=D, out=ctypes.c_void_p(2), nf=D, tg=D, w=WP, loss=D, ws=D)
    a.update(kw)
    nb = int(L.hf_pure_unroll_workspace_bytes(max(B, 1), max(nx, 1))) - ws_short
    return L.hf_pure_unroll_update(a["delta"], a["st"], a["x"], B, nx, a["out"], a["nf"], a["tg"], a["w"], 1.0,
                                   a["loss"], a["ws"], nb, None)


def _adjoint(L, B=3, nx=16, **kw):
    a = dict(sn=D, tg=D, w=WP, gdn=D, gnf=D, gd=D)
    a.update(kw)
    return L.hf_pure_unroll_adjoint(a["sn"], a["tg"], a["w"], 1.0, a["gdn"], a["gnf"], B, nx, a["gd"], None)


def _refused(L, rc, name, word=None):
    assert rc == _lib.HF_EINVAL
    err = L.hf_last_error()
    assert name in err, err
    if word:
        assert word in err, err


def test_update_validates_before_device():
    L = _lib.lib()
    name = b"hf_pure_unroll_update"
    for kw in ("delta", "st", "x", "out"):                    # every required pointer
        _refused(L, _update(L, **{kw: None}), name, b"NULL")
    for kw in ("w", "loss", "ws"):                             # required once a target is given
        _refused(L, _update(L, **{kw: None}), name, b"NULL")
    for B in (0, -2, -2 ** 31):
        _refused(L, _update(L, B=B), name)
    for nx in (0, -1, -2 ** 31):
        _refused(L, _update(L, nx=nx), name)
    _refused(L, _update(L, ws_short=1), name, b"workspace")
    _refused(L, _update(L, out=D), name, b"alias")            # state_next == state
    assert L.hf_pure_unroll_update(D, D, D, 2 ** 31 - 1, 1025, ctypes.c_void_p(2), None, None, None, 1.0, None, None, 0,
                                   None) == _lib.HF_EINVAL    # more workgroups than a grid holds
    assert name in L.hf_last_error()


def test_adjoint_validates_before_device():
    L = _lib.lib()
    name = b"hf_pure_unroll_adjoint"
    for kw in ("sn", "tg", "w", "gd"):                         # every required pointer
        _refused(L, _adjoint(L, **{kw: None}), name, b"NULL")
    for B in (0, -1, -2 ** 31):
        _refused(L, _adjoint(L, B=B), name)
    for nx in (0, -4, -2 ** 31):
        _refused(L, _adjoint(L, nx=nx), name)
    _refused(L, _adjoint(L, B=2 ** 31 - 1, nx=1025), name)


def test_pure_unrolled_flop_model():
    """K times the one-step count, plus the input layer's data gradient for the
    K - 1 steps that pass a state gradient back."""
    from hybridflux.training import pure_gnn_train_flop_per_sample, pure_unrolled_train_flop_per_sample
    one = pure_gnn_train_flop_per_sample()
    assert pure_unrolled_train_flop_per_sample(1) == one
    assert pure_unrolled_train_flop_per_sample(4) == 4 * one + 3 * 2 * 4 * 128 * 64
    assert pure_unrolled_train_flop_per_sample(2, nx=16, H=64, L=3, F=4) == \
        2 * pure_gnn_train_flop_per_sample(nx=16, H=64, L=3, F=4) + 2 * 4 * 64 * 16


def test_python_layer_refuses_other_models():
    """pure_unrolled_loss is PureGNN's (input_dim 4); unrolled_loss stays FluxGNN's."""
    import pytest
    import torch

    import hybridflux
    from hybridflux import training
    traj, x = torch.zeros(2, 3, 3, 16), torch.zeros(16)
    with pytest.raises(TypeError):
        training.pure_unrolled_loss(hybridflux.FluxGNN(4, 128, 4), traj, x)
    with pytest.raises(ValueError):
        training.pure_unrolled_loss(hybridflux.PureGNN(3, 64, 1), traj, x)
    assert training.pure_unrolled_step(hybridflux.FluxGNN(4, 128, 4), None, traj, x) is None
