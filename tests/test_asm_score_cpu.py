"""Compiled device code of the scored rollout kernels (no GPU needed;
tools/asm_wait_scan.py compiles baselines.hip for gfx950 with the library's
flags): pure_score_kernel and pinn_score_kernel run their layers on the matrix
core like the unscored kernels they share a body with, and the scoring wave's
twin, metric sums and Poisson row add no scratch (spill) operation."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")


@pytest.fixture(scope="module")
def stats(tmp_path_factory):
    import asm_wait_scan
    return asm_wait_scan.scan(os.path.join(asm_wait_scan.CSRC, "baselines.hip"), str(tmp_path_factory.mktemp("asm")))


def _kernels(stats, part):
    hits = {k: v for k, v in stats.items() if part in k}
    assert hits, part
    return hits


def test_pure_score_kernels(stats):
    hits = _kernels(stats, "pure_score_kernel")
    assert len(hits) == 16                                   # H in {64, 128} x nx / 16 in 1..4 x packed or not
    for k, v in hits.items():
        assert v["mfma"] > 0 and v["scratch"] == 0, (k, v)


def test_pinn_score_kernel(stats):
    hits = _kernels(stats, "pinn_score_kernel")
    assert len(hits) == 1
    for k, v in hits.items():
        assert v["mfma"] > 0 and v["scratch"] == 0, (k, v)


def test_scored_names_stay_clear_of_the_pinned_kernels(stats):
    """test_asm_hazards_cpu.py pins every kernel whose name contains these strings."""
    for k in list(_kernels(stats, "pure_score_kernel")) + list(_kernels(stats, "pinn_score_kernel")):
        assert "pinn_run_kernel" not in k and "pure_run_kernelILi128ELi4ELb1" not in k, k
