"""CPU-side checks of the model-set entry points of the C ABI
(hf_model_set_create / _destroy / _size, hf_run_set, hf_run_compare_set,
hf_set_workspace_need): the symbols and their declarations, and that every bad
argument is refused before any device call with the function's name in
hf_last_error() (no kernel is launched here; the dummy pointers are never
dereferenced)."""
import ctypes
import os
import re

import pytest

from hybridflux import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, E = ctypes.c_void_p(256), ctypes.c_void_p(512)
NAMES = ("hf_model_set_create", "hf_model_set_destroy", "hf_model_set_size", "hf_run_set", "hf_run_compare_set",
         "hf_set_workspace_need")


def err():
    return _lib.lib().hf_last_error().decode()


def test_symbols_declared_and_exported():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hybridflux.h")).read()
    assert "typedef struct hf_model_set *hf_model_set_t;" in header
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(L, n), n
        m = re.search(rf"\b(int64_t|int|void)\s+{n}\(([^;]*)\);", header)
        assert m, f"{n} is not declared in include/hybridflux.h"
        res, args = _lib.SIGNATURES[n]
        assert {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "void": None}[m.group(1)] is res, n
        assert len(args) == len(m.group(2).split(",")), n        # one ctypes argument per declared parameter
    # model_stride (int64) follows dev_state0; the four float scalars and workspace_bytes sit where the header puts them
    for n in ("hf_run_set", "hf_run_compare_set"):
        a = _lib.SIGNATURES[n][1]
        assert len(a) == 20 and a[2] is ctypes.c_int64 and a[18] is ctypes.c_int64
        assert [i for i, t in enumerate(a) if t is ctypes.c_float] == [10, 11, 12, 13]
        assert [i for i, t in enumerate(a) if t is ctypes.c_int] == [6, 7, 8, 9]


def test_create_refuses_bad_arguments():
    L = _lib.lib()
    out = ctypes.c_void_p(8)
    none = (ctypes.c_void_p * 2)(None, None)
    for models, M, o in ((None, 2, out), (none, 0, out), (none, -1, out), (none, 2, None), (none, 2, out)):
        assert L.hf_model_set_create(models, M, o) == _lib.HF_EINVAL
        assert "hf_model_set_create" in err()
    assert out.value is None                      # cleared on failure
    L.hf_model_set_destroy(None)                  # a no-op
    assert L.hf_model_set_size(None) == 0


def _call(name, set_=None, s0=D, stride=0, fin=E, B=3, nx=64, T=5, pm=0, mse=D):
    L = _lib.lib()
    if name == "hf_run_set":
        return L.hf_run_set(set_, s0, stride, fin, D, D, pm, B, nx, T, 0.05, 5e-3, 1e-3, 0.01, None, None, None,
                            None, 0, None)
    return L.hf_run_compare_set(set_, s0, stride, fin, D, D, pm, B, nx, T, 0.05, 5e-3, 1e-3, 0.01, mse, None, None,
                                None, 0, None)


@pytest.mark.parametrize("name", ["hf_run_set", "hf_run_compare_set"])
def test_run_refuses_bad_arguments(name):
    bad = [
        (dict(), "NULL model set"),
        (dict(B=-1), "B >= 0"), (dict(nx=0), "nx >= 1"), (dict(nx=-64), "nx >= 1"), (dict(T=-1), "T >= 0"),
        (dict(stride=1), "model_stride"), (dict(stride=3 * 3 * 64 + 1), "model_stride"),
        (dict(stride=-3 * 3 * 64), "model_stride"), (dict(stride=3 * 64), "model_stride"),
        (dict(B=2 ** 31 - 1, nx=2 ** 31 - 1, stride=8), "model_stride"),   # B*3*nx past 2^63
        (dict(fin=D), "alias"),                                              # shared ICs rolled out in place
        (dict(stride=3 * 3 * 64, fin=D), "NULL model set"),                  # in place with ICs per model is allowed
        (dict(stride=3 * 3 * 64), "NULL model set"),
    ]
    for kw, what in bad:
        assert _call(name, **kw) == _lib.HF_EINVAL, kw
        assert name + ":" in err() and what in err(), (kw, err())


def test_workspace_need_refuses_bad_arguments():
    L = _lib.lib()
    for op in (_lib.HF_OP_STEP, _lib.HF_OP_RUN, _lib.HF_OP_COMPARE, 7, -1):
        assert L.hf_set_workspace_need(None, op, 3, 64, 5, 0) == -1
    assert L.hf_set_workspace_need(None, _lib.HF_OP_RUN, -1, 64, 5, 0) == -1
