"""CPU-side checks of the scored-rollout entry points of the C ABI
(hf_pure_gnn_score_workspace_bytes, hf_pure_gnn_run_scored,
hf_pinn_score_workspace_bytes, hf_pinn_run_scored): the symbols and their
declarations, the workspace sizes, and that every bad argument is refused
before any device call with the function's name in hf_last_error() (no kernel
is launched here; the dummy pointers are never dereferenced)."""
import ctypes
import os
import re

import pytest

from hybridflux import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = ctypes.c_void_p(1)
NAMES = ("hf_pure_gnn_score_workspace_bytes", "hf_pure_gnn_run_scored", "hf_pinn_score_workspace_bytes",
         "hf_pinn_run_scored")


def test_symbols_declared_and_exported():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hybridflux.h")).read()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(L, n), n
        m = re.search(rf"\b(int64_t|int) {n}\(([^;]*)\);", header)
        assert m, f"{n} is not declared in include/hybridflux.h"
        res, args = _lib.SIGNATURES[n]
        assert (res is ctypes.c_int64) == (m.group(1) == "int64_t")
        assert len(args) == len(m.group(2).split(",")), n        # one ctypes argument per declared parameter
    # the scalar arguments sit where the header puts them
    pg, pn = _lib.SIGNATURES["hf_pure_gnn_run_scored"][1], _lib.SIGNATURES["hf_pinn_run_scored"][1]
    assert [i for i, a in enumerate(pg) if a is ctypes.c_float] == [11, 12, 13, 14]
    assert [i for i, a in enumerate(pn) if a is ctypes.c_float] == [10, 11, 12, 13]
    assert pg[20] is ctypes.c_int64 and pn[19] is ctypes.c_int64 and pn[8] is ctypes.c_int64   # workspace bytes; PINN's B


def test_workspace_sizes():
    L = _lib.lib()
    # the one-launch shapes: exactly the unscored rollout's need
    for H in (64, 128):
        for nx in (16, 32, 48, 64):
            for B, T in ((1, 0), (3, 1), (4096, 1000)):
                assert L.hf_pure_gnn_score_workspace_bytes(H, B, nx, T) == L.hf_pure_gnn_run_workspace_bytes(H, B, nx, T)
    for B, T in ((1, 0), (17, 5), (4096, 1000)):
        assert L.hf_pinn_score_workspace_bytes(192, 256, B, T) == L.hf_pinn_workspace_bytes(192, 256, B)
    # every other shape: at least two [B][T+1][3][nx] float trajectories more
    for H, nx, B, T in ((64, 20, 2, 5), (32, 32, 2, 5), (128, 100, 3, 0), (64, 80, 7, 40)):
        assert L.hf_pure_gnn_score_workspace_bytes(H, B, nx, T) >= \
            L.hf_pure_gnn_run_workspace_bytes(H, B, nx, T) + 2 * 4 * B * (T + 1) * 3 * nx
    for dim, H, B, T in ((48, 32, 3, 5), (192, 128, 5, 0), (96, 256, 33, 12)):
        assert L.hf_pinn_score_workspace_bytes(dim, H, B, T) >= \
            L.hf_pinn_workspace_bytes(dim, H, B) + 2 * 4 * B * (T + 1) * dim
    assert L.hf_pure_gnn_score_workspace_bytes(64, 0, 20, 5) == 0
    # bad arguments
    for a in ((0, 3, 64, 5), (64, -1, 64, 5), (64, 3, 0, 5), (64, 3, 64, -1), (-2 ** 31,) * 4,
              (64, 2 ** 31 - 1, 20, 2 ** 31 - 1)):
        assert L.hf_pure_gnn_score_workspace_bytes(*a) == -1, a
    for a in ((50, 32, 3, 5), (0, 32, 3, 5), (48, 0, 3, 5), (48, 32, -1, 5), (48, 32, 3, -1), (48, 32, 2 ** 40, 2 ** 31 - 1)):
        assert L.hf_pinn_score_workspace_bytes(*a) == -1, a


def _pure(L, hidden=128, layers=4, B=3, nx=64, T=5, pm=0, ws_short=0, **kw):
    a = dict(params=D, s0=D, fin=D, x=D, plan=D, traj=D, met=D, mse=D, mcl=D, ws=D)
    a.update(kw)
    nb = int(L.hf_pure_gnn_score_workspace_bytes(hidden, B, nx, T))
    nb = (1 << 20) if nb < 0 else nb
    return L.hf_pure_gnn_run_scored(a["params"], hidden, layers, a["s0"], a["fin"], a["x"], a["plan"], pm, B, nx, T,
                                    0.05, 5e-3, 1e-3, 0.01, a["traj"], a["met"], a["mse"], a["mcl"], a["ws"],
                                    nb - ws_short, None)


def _pinn(L, dim=192, hidden=256, layers=4, B=3, T=5, pm=0, ws_short=0, **kw):
    a = dict(params=D, s0=D, fin=D, plan=D, traj=D, met=D, mse=D, mcl=D, ws=D)
    a.update(kw)
    nb = int(L.hf_pinn_score_workspace_bytes(dim, hidden, B, T))
    nb = (1 << 20) if nb < 0 else nb
    return L.hf_pinn_run_scored(a["params"], dim, hidden, layers, a["s0"], a["fin"], a["plan"], pm, B, T, 0.05, 5e-3,
                                1e-3, 0.01, a["traj"], a["met"], a["mse"], a["mcl"], a["ws"], nb - ws_short, None)


def _refused(L, rc, name, word=None, code=_lib.HF_EINVAL):
    assert rc == code, (rc, L.hf_last_error())
    err = L.hf_last_error()
    assert name in err, err
    if word:
        assert word in err, err


@pytest.mark.parametrize("call,name", [(_pure, b"hf_pure_gnn_run_scored"), (_pinn, b"hf_pinn_run_scored")])
def test_shared_refusals(call, name):
    L = _lib.lib()
    for kw in ("params", "s0", "fin", "plan"):                       # required pointers (the plan: with dev_mse)
        _refused(L, call(L, **{kw: None}), name, b"NULL")
    _refused(L, call(L, met=None, mse=None, mcl=None), name, b"nothing to score")
    _refused(L, call(L, mse=None), name, b"dev_metrics_classical")   # the twin's series without the twin
    _refused(L, call(L, B=0, met=None, mse=None), name, b"nothing to score")
    _refused(L, call(L, ws=None), name, b"workspace")
    _refused(L, call(L, ws_short=1), name, b"workspace")             # one byte short
    for kw in ({"B": -1}, {"T": -1}, {"T": -2 ** 31}, {"pm": -1}, {"pm": 2}, {"layers": -1}, {"hidden": 0}):
        _refused(L, call(L, **kw), name)
    assert call(L, B=0) == _lib.HF_OK                                # an empty batch is a valid call


def test_pure_gnn_refusals():
    L = _lib.lib()
    name = b"hf_pure_gnn_run_scored"
    _refused(L, _pure(L, x=None), name, b"NULL")
    for nx in (0, -1, -2 ** 31):
        _refused(L, _pure(L, nx=nx), name)
    _refused(L, _pure(L, nx=20, ws_short=1), name, b"workspace")    # a shape that sequences the existing kernels
    _refused(L, _pure(L, nx=20, ws=None), name, b"workspace")
    _refused(L, _pure(L, nx=20000, pm=_lib.HF_POISSON_TRIDIAG), name, code=_lib.HF_EUNSUPPORTED)


def test_pinn_refusals():
    L = _lib.lib()
    name = b"hf_pinn_run_scored"
    for dim in (50, 191, 193):
        _refused(L, _pinn(L, dim=dim), name, b"3 * nx")
    for dim in (0, -3):
        _refused(L, _pinn(L, dim=dim), name)
    for layers in (1, 9):
        _refused(L, _pinn(L, layers=layers), name)
    _refused(L, _pinn(L, dim=48, hidden=32, ws_short=1), name, b"workspace")


def test_python_layer_without_a_device():
    """The adapter's refusals that need no device."""
    import torch

    import hybridflux
    from hybridflux import evaluation

    class _Base:  # a BaselineSolver's grid without its device
        grid = hybridflux.engine.Grid(16)

        def _upload(self, s):
            return s
    m = evaluation.ModelRollout(hybridflux.PureGNN(4, 64, 1), _Base())
    with pytest.raises(ValueError):
        m.run_batch(torch.zeros(1, 3, 16), 2, flux=True)
    assert m.grid is _Base.grid and len(m.x) == 16
    assert evaluation.compare_models({}, torch.zeros(1, 3, 16), 2) == {}
    with pytest.raises(ValueError):                                   # scoring builds [n,u,E,x] node features
        hybridflux.PureGNN(5, 64, 1).rollout(torch.zeros(1, 3, 16), 2, _Base.grid.x, metrics=True)
