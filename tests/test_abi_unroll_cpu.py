"""CPU-side checks of the unrolled-training entry points of the C ABI
(hf_unroll_workspace_bytes, hf_unroll_update, hf_unroll_adjoint): the size
query, and that bad arguments are refused before any device call with the
function's name in hf_last_error() (no kernel is launched here; the dummy
pointers are never dereferenced)."""
import ctypes

import numpy as np

from hybridflux import _lib

D = ctypes.c_void_p(1)
W = np.ones(3, dtype=np.float32)
WP = W.ctypes.data_as(ctypes.c_void_p)
SPECTRAL, TRIDIAG = _lib.HF_POISSON_SPECTRAL, _lib.HF_POISSON_TRIDIAG


def test_workspace_query():
    L = _lib.lib()
    for B, nx in ((3, 16), (4096, 64), (3, 256)):
        assert L.hf_unroll_workspace_bytes(B, nx) > 0
    assert L.hf_unroll_workspace_bytes(4096, 64) >= 4096 * 8      # one float64 partial per IC
    assert L.hf_unroll_workspace_bytes(0, 64) == -1
    assert L.hf_unroll_workspace_bytes(3, 0) == -1
    assert L.hf_unroll_workspace_bytes(-1, 64) == -1


def _update(L, B=3, nx=16, pm=SPECTRAL, ws_short=0, **kw):
    a = dict(fe=D, st=D, x=D, pc=D, out=ctypes.c_void_p(2), nf=D, tg=D, w=WP, loss=D, ws=D)
    a.update(kw)
    nb = int(L.hf_unroll_workspace_bytes(max(B, 1), max(nx, 1))) - ws_short
    return L.hf_unroll_update(a["fe"], a["st"], a["x"], a["pc"], pm, B, nx, 0.05, 5e-3, a["out"], a["nf"], a["tg"],
                              a["w"], 1.0, a["loss"], a["ws"], nb, None)


def _adjoint(L, B=3, nx=16, pm=SPECTRAL, **kw):
    a = dict(st=D, sn=D, tg=D, w=WP, din=D, gnf=D, pc=D, gfe=D, dout=D)
    a.update(kw)
    return L.hf_unroll_adjoint(a["st"], a["sn"], a["tg"], a["w"], 1.0, a["din"], a["gnf"], a["pc"], pm, B, nx, 0.05,
                               5e-3, a["gfe"], a["dout"], None)


def _refused(L, rc, code, name, word=None):
    assert rc == code
    err = L.hf_last_error()
    assert name in err, err
    if word:
        assert word in err, err


def test_update_validates_before_device():
    L = _lib.lib()
    name = b"hf_unroll_update"
    for kw in ("fe", "st", "x", "pc", "out", "ws"):           # every required pointer
        _refused(L, _update(L, **{kw: None}), _lib.HF_EINVAL, name, b"NULL")
    for kw in ("w", "loss"):                                   # required once a target is given
        _refused(L, _update(L, **{kw: None}), _lib.HF_EINVAL, name, b"NULL")
    _refused(L, _update(L, B=0), _lib.HF_EINVAL, name)
    _refused(L, _update(L, B=-2), _lib.HF_EINVAL, name)
    _refused(L, _update(L, nx=0), _lib.HF_EINVAL, name)
    _refused(L, _update(L, ws_short=1), _lib.HF_EINVAL, name, b"workspace")
    _refused(L, _update(L, out=D), _lib.HF_EINVAL, name, b"alias")     # state_next == state
    _refused(L, _update(L, pm=7), _lib.HF_EINVAL, name, b"mode")
    _refused(L, _update(L, nx=6145), _lib.HF_EUNSUPPORTED, name, b"6144")
    _refused(L, _update(L, pm=TRIDIAG), _lib.HF_EUNSUPPORTED, name, b"tridiagonal")


def test_adjoint_validates_before_device():
    L = _lib.lib()
    name = b"hf_unroll_adjoint"
    for kw in ("st", "sn", "tg", "w", "pc", "gfe"):            # every required pointer
        _refused(L, _adjoint(L, **{kw: None}), _lib.HF_EINVAL, name, b"NULL")
    _refused(L, _adjoint(L, B=0), _lib.HF_EINVAL, name)
    _refused(L, _adjoint(L, nx=0), _lib.HF_EINVAL, name)
    _refused(L, _adjoint(L, nx=-4), _lib.HF_EINVAL, name)
    _refused(L, _adjoint(L, pm=7), _lib.HF_EINVAL, name, b"mode")
    _refused(L, _adjoint(L, nx=6145), _lib.HF_EUNSUPPORTED, name, b"6144")
    _refused(L, _adjoint(L, pm=TRIDIAG), _lib.HF_EUNSUPPORTED, name, b"tridiagonal")


def test_unrolled_flop_model():
    """K forwards + K backwards of the one-step count's GEMMs, plus the input
    layer's data gradient for the K - 1 steps that pass a state gradient back."""
    from hybridflux.training import train_flop_per_sample, unrolled_train_flop_per_sample
    one = train_flop_per_sample("baseline")
    assert unrolled_train_flop_per_sample(1) == one
    assert unrolled_train_flop_per_sample(4) == 4 * one + 3 * 2 * 4 * 128 * 64
    assert unrolled_train_flop_per_sample(2, nx=16, H=64, L=3, F=4) == \
        2 * train_flop_per_sample("baseline", nx=16, H=64, L=3, F=4) + 2 * 4 * 64 * 16
