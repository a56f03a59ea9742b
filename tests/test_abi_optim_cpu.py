"""The guarded optimizer step's entry points (hf_adam_flat_workspace_bytes,
hf_adam_flat_ex) refuse what include/hybridflux.h says they refuse, before any
HIP call: runs without a GPU, the dummy pointers are never dereferenced."""
import ctypes
import math

import pytest

from hybridflux import _lib

D = ctypes.c_void_p(64)
INF = float("inf")


def call(n=10, p=D, g=D, m=D, v=D, step=D, done=D, dev_lr=None, lr=1e-3, wd=0.0, max_norm=INF, skip=0, ws=D,
         stats=None):
    return _lib.lib().hf_adam_flat_ex(p, g, m, v, n, step, done, dev_lr, lr, 0.9, 0.999, 1e-8, wd, max_norm, skip, ws,
                                      stats, None)


def refused(**kw):
    rc = call(**kw)
    return rc == _lib.HF_EINVAL and b"hf_adam_flat_ex" in _lib.lib().hf_last_error()


def test_constant_matches_the_header():
    import os
    import re

    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "hybridflux.h")).read()
    assert int(re.search(r"#define HF_OPT_NUM_STATS (\d+)", text).group(1)) == _lib.HF_OPT_NUM_STATS == 4


def test_negative_n():
    assert refused(n=-1)
    assert refused(n=-(2 ** 63))


@pytest.mark.parametrize("which", ["p", "g", "m", "v", "step", "done"])
def test_null_pointer_with_values(which):
    assert refused(**{which: None})


@pytest.mark.parametrize("max_norm", [0.0, -1.0, -INF, math.nan])
def test_max_norm_must_be_positive(max_norm):
    assert refused(max_norm=max_norm)
    assert refused(max_norm=max_norm, n=0)


@pytest.mark.parametrize("wd", [-1e-3, -INF, math.nan])
def test_weight_decay_must_not_be_negative(wd):
    assert refused(wd=wd)
    assert refused(wd=wd, n=0)


def test_missing_workspace():
    """dev_ws may be NULL only when nothing needs the norm."""
    assert refused(ws=None, max_norm=1.0)
    assert refused(ws=None, skip=1)
    assert refused(ws=None, stats=D)
    assert refused(ws=None, max_norm=3.0e38, skip=1, stats=D)


def test_empty_buffer_is_a_no_op():
    """n == 0 is HF_OK without a launch, as for hf_adam_flat, whatever the pointers."""
    assert call(n=0, p=None, g=None, m=None, v=None, step=None, done=None, ws=None) == _lib.HF_OK
    assert call(n=0, max_norm=1.0, wd=0.1, skip=1, stats=D, dev_lr=D) == _lib.HF_OK


def test_workspace_bytes_monotone_multiple_of_8():
    q = _lib.lib().hf_adam_flat_workspace_bytes
    assert q(-1) == -1 and q(-(2 ** 63)) == -1
    ns = [0, 1, 255, 256, 1023, 1024, 1025, 4096, 165249, 230336, 2048 * 1024 - 1, 2048 * 1024, 2048 * 1024 + 1025,
          2 ** 31, 2 ** 40, 2 ** 63 - 1]
    sizes = [q(n) for n in ns]
    assert all(s >= 8 and s % 8 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes[0] == 8 and sizes[-1] == 8 * 2048
