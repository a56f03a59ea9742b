"""Every handle-free size query returns what tests/workspace_sizes.json recorded.

The table (tools/dump_workspace_sizes.py) holds each public `hf_*bytes*` /
`hf_*need*` query's value over a grid that crosses its branch boundaries,
`-1` and `0` cases included.  The library produces a size by running the code
that carves the buffer on a NULL base, so a layout that moves shows up here as a
changed value.  The rows that need a model handle are replayed on a device by
tests/test_gpu_workspace_lanes.py.
"""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dump_workspace_sizes as table  # noqa: E402

with open(os.path.join(ROOT, "tests", "workspace_sizes.json")) as _f:
    SIZES = json.load(_f)
HANDLE_FREE = sorted(k for k in SIZES if k != "device")


@pytest.mark.parametrize("name", HANDLE_FREE)
def test_recorded_sizes(name):
    from hybridflux._lib import lib
    f = getattr(lib(), name)
    null = (None,) if name == "hf_workspace_need" else ()  # NULL model: the classical solver
    rows = SIZES[name]
    assert rows
    bad = [(row[:-1], row[-1], got) for row in rows for got in [f(*null, *row[:-1])] if got != row[-1]]
    assert not bad, f"{name}: {len(bad)} of {len(rows)} rows differ (args, recorded, got): {bad[:5]}"


def test_table_is_the_tools_grid():
    want = table.handle_free_args()
    assert sorted(want) == HANDLE_FREE
    for name, rows in want.items():
        assert [list(a) for a in rows] == [row[:-1] for row in SIZES[name]], name
    assert {k: [r[:-1] for r in v] for k, v in SIZES["device"].items()} == \
        {k: [list(a) for a in v] for k, v in table.device_args().items()}


def test_every_size_query_is_covered():
    with open(os.path.join(ROOT, "include", "hybridflux.h")) as f:
        header = f.read()
    declared = set(re.findall(r"^int64_t\s+(hf_\w*(?:bytes|need)\w*)\s*\(", header, flags=re.M))
    assert len(declared) >= 26
    covered = set(HANDLE_FREE) | set(table.HANDLE_QUERIES)
    assert declared <= covered, sorted(declared - covered)
    assert set(table.HANDLE_QUERIES) <= declared and set(SIZES["device"]) == set(table.HANDLE_QUERIES)
