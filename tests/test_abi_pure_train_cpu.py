"""CPU-side checks of the PureGNN training entry points of the C ABI
(hf_pure_gnn_tape_bytes, hf_pure_gnn_backward_workspace_bytes,
hf_pure_gnn_forward_train, hf_pure_gnn_backward, hf_state_mse_workspace_bytes,
hf_state_mse): the size queries, and that bad arguments are refused with
HF_EINVAL before any device call (no kernel is launched here; the dummy
pointers are never dereferenced)."""
import ctypes

from hybridflux import _lib

D = ctypes.c_void_p(1)


def test_size_queries():
    L = _lib.lib()
    for fn in (L.hf_pure_gnn_tape_bytes, L.hf_pure_gnn_backward_workspace_bytes):
        assert fn(4, 64, 3, 64, 128) > 0
        assert fn(4, 64, 0, 64, 0) > 0          # no message layer, no edges
        assert fn(4, 64, 9, 64, 128) == -1      # > 8 layers
        assert fn(0, 64, 3, 64, 128) == -1
        assert fn(4, 0, 3, 64, 128) == -1
        assert fn(4, 64, -1, 64, 128) == -1
        assert fn(4, 64, 3, 0, 0) == -1         # N = 0
        assert fn(4, 64, 3, 64, -1) == -1
    # the tape holds h_0..h_L, z and every message: it grows with the layers and the edges
    assert L.hf_pure_gnn_tape_bytes(4, 64, 3, 64, 128) > L.hf_pure_gnn_tape_bytes(4, 64, 2, 64, 128)
    assert L.hf_pure_gnn_tape_bytes(4, 64, 3, 64, 256) >= L.hf_pure_gnn_tape_bytes(4, 64, 3, 64, 128) + 3 * 128 * 64 * 4
    assert L.hf_state_mse_workspace_bytes(32, 64) > 0
    assert L.hf_state_mse_workspace_bytes(0, 64) == -1
    assert L.hf_state_mse_workspace_bytes(32, 0) == -1


def _fwd(L, N=64, E=128, chain_nx=0, layers=3, params=D, nf=D, ei=D, delta=D, tape=D):
    return L.hf_pure_gnn_forward_train(params, 4, 64, layers, nf, N, ei, E, chain_nx, delta, tape, None)


def _bwd(L, N=64, E=128, chain_nx=0, layers=3, params=D, nf=D, ei=D, tape=D, gd=D, gp=D, gnf=None, ws=D):
    return L.hf_pure_gnn_backward(params, 4, 64, layers, nf, N, ei, E, chain_nx, tape, gd, gp, gnf, ws, None)


def test_forward_train_validates_before_device():
    L = _lib.lib()
    assert _fwd(L, chain_nx=24) == _lib.HF_EINVAL            # chain_nx does not divide N
    assert b"hf_pure_gnn_forward_train" in L.hf_last_error() and b"chain_nx" in L.hf_last_error()
    assert _fwd(L, E=127, chain_nx=16) == _lib.HF_EINVAL     # E != 2N on a chain
    assert b"hf_pure_gnn_forward_train" in L.hf_last_error()
    assert _fwd(L, N=0, E=0) == _lib.HF_EINVAL               # N = 0
    assert b"hf_pure_gnn_forward_train" in L.hf_last_error()
    assert _fwd(L, layers=9) == _lib.HF_EINVAL
    assert _fwd(L, N=-1) == _lib.HF_EINVAL
    assert _fwd(L, tape=None) == _lib.HF_EINVAL              # NULL tape
    assert b"hf_pure_gnn_forward_train" in L.hf_last_error() and b"NULL" in L.hf_last_error()
    for kw in ("params", "nf", "ei", "delta"):
        assert _fwd(L, **{kw: None}) == _lib.HF_EINVAL, kw


def test_backward_validates_before_device():
    L = _lib.lib()
    assert _bwd(L, chain_nx=24) == _lib.HF_EINVAL
    assert b"hf_pure_gnn_backward" in L.hf_last_error() and b"chain_nx" in L.hf_last_error()
    assert _bwd(L, E=130, chain_nx=16) == _lib.HF_EINVAL
    assert _bwd(L, N=0, E=0) == _lib.HF_EINVAL
    assert b"hf_pure_gnn_backward" in L.hf_last_error()
    assert _bwd(L, layers=9) == _lib.HF_EINVAL
    assert _bwd(L, tape=None) == _lib.HF_EINVAL              # NULL tape
    assert b"hf_pure_gnn_backward" in L.hf_last_error() and b"NULL" in L.hf_last_error()
    assert _bwd(L, ws=None) == _lib.HF_EINVAL                # NULL workspace
    for kw in ("params", "nf", "ei", "gd", "gp"):
        assert _bwd(L, **{kw: None}) == _lib.HF_EINVAL, kw


def test_state_mse_validates_before_device():
    L = _lib.lib()
    ws = int(L.hf_state_mse_workspace_bytes(32, 64))
    assert L.hf_state_mse(D, D, D, 32, 64, D, D, D, ws - 1, None) == _lib.HF_EINVAL   # workspace too small
    assert b"hf_state_mse" in L.hf_last_error() and b"workspace" in L.hf_last_error()
    assert L.hf_state_mse(D, D, D, 0, 64, D, D, D, ws, None) == _lib.HF_EINVAL
    assert L.hf_state_mse(D, D, D, 32, 0, D, D, D, ws, None) == _lib.HF_EINVAL
    assert L.hf_state_mse(D, D, D, 32, 64, D, D, None, ws, None) == _lib.HF_EINVAL    # NULL workspace
    assert b"hf_state_mse" in L.hf_last_error() and b"NULL" in L.hf_last_error()
    for k in (0, 1, 2, 5, 6):
        a = [D, D, D, 32, 64, D, D, D, ws, None]
        a[k] = None
        assert L.hf_state_mse(*a) == _lib.HF_EINVAL, k
