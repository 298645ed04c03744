"""-m "not gpu": the pruned forms of the length-aware furthest point sampling.  The three new entry points
(mcp_fps_lengths_pruned_workspace_bytes, mcp_fps_lengths_form, mcp_furthest_point_sampling_lengths_unpruned) are declared, exported
and bound; the workspace query and the dispatch rule -- a pure function of the padded shape and the workspace size, the function
the dispatcher itself calls -- answer without a GPU; the unpruned entry point validates its arguments as the pruned one does."""
import os
import re

import pytest

from mocopci_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mocopci_hip.h")
ARGS = {"mcp_fps_lengths_pruned_workspace_bytes": 3, "mcp_fps_lengths_form": 4, "mcp_furthest_point_sampling_lengths_unpruned": 10}
BAD_ARG, UNSUPPORTED = 10001, 10002
RESIDENT, SPATIAL, TILED, STREAMING = 0, 1, 2, 3


def test_entry_points_are_declared_exported_and_bound():
    with open(HEADER) as fh:
        header = re.sub(r"\s+", " ", fh.read())
    assert "size_t mcp_fps_lengths_pruned_workspace_bytes(int b, int n, int m);" in header
    assert "int mcp_fps_lengths_form(int b, int n, int m, size_t workspace_bytes);" in header
    assert ("int mcp_furthest_point_sampling_lengths_unpruned(int b, int n, int m, const float *xyz, const int *len, int *idx, "
            "float *sampled_xyz, void *workspace, size_t workspace_bytes, mcp_stream_t stream);") in header
    for name, value in (("RESIDENT", RESIDENT), ("SPATIAL", SPATIAL), ("TILED", TILED), ("STREAMING", STREAMING)):
        assert f"#define MCP_FPS_LENGTHS_{name} {value} " in header + " "
    lib = _lib.load()
    for name, nargs in ARGS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name]) == nargs, (name, len(_lib.SIGNATURES[name]))
    # the two calls take the same arguments
    assert _lib.SIGNATURES["mcp_furthest_point_sampling_lengths_unpruned"] == _lib.SIGNATURES["mcp_furthest_point_sampling_lengths"]


def test_pruned_workspace_query():
    lib = _lib.load()
    query, plain = lib.mcp_fps_lengths_pruned_workspace_bytes, lib.mcp_fps_lengths_workspace_bytes
    assert query(8, 8192, 2048) == 0
    assert query(8, 16384, 64) == 0
    assert query(2, 20000, 16) == 2 * 20032 * 20
    assert query(8, 65536, 2048) == 8 * 65536 * 20
    assert query(1, 65537, 16) == plain(1, 65537, 16) == 65537 * 4
    assert query(2, 20000, 16) == lib.mcp_fps_workspace_bytes(2, 20000, 16)      # the length-free tiled kernel's figure
    assert query(0, 20000, 16) == 0
    assert plain(3, 20000, 32) == 3 * 20000 * 4                                  # the existing query keeps its value


def pruned_figure():
    return _lib.load().mcp_fps_lengths_pruned_workspace_bytes(3, 20000, 32)


@pytest.mark.parametrize("args,want", [
    ((8, 100, 16, 0), RESIDENT),
    ((8, 1023, 16, 0), RESIDENT),
    ((8, 8192, 1, 0), RESIDENT),
    ((8, 1024, 2, 0), SPATIAL),
    ((8, 16384, 64, 0), SPATIAL),
    ((3, 20000, 32, 3 * 20000 * 4), STREAMING),
    ((3, 20000, 32, "pruned"), TILED),
    ((3, 20000, 32, "pruned-1"), STREAMING),
    ((3, 20000, 32, 3 * 20000 * 4 - 1), UNSUPPORTED),
    ((1, 65537, 16, 65537 * 4), STREAMING),
])
def test_dispatch_rule(args, want):
    b, n, m, ws = args
    if ws == "pruned":
        ws = pruned_figure()
    elif ws == "pruned-1":
        ws = pruned_figure() - 1
    assert pruned_figure() == 3 * 20032 * 20 > 3 * 20000 * 4
    assert _lib.load().mcp_fps_lengths_form(b, n, m, ws) == want


def test_form_validates_its_shape():
    form = _lib.load().mcp_fps_lengths_form
    assert form(0, 100, 16, 0) == BAD_ARG and form(8, 0, 16, 0) == BAD_ARG and form(-1, 100, 16, 0) == BAD_ARG


def test_unpruned_argument_validation_equals_the_pruned_one():
    lib = _lib.load()
    tail = (None, None, 0, None)                               # sampled_xyz, workspace, workspace_bytes, stream
    calls = [(1, 16, 4, None, 8, 8), (1, 16, 4, 8, 8, None), (0, 16, 4, 8, 8, 8), (-1, 16, 4, 8, 8, 8), (1, 0, 4, 8, 8, 8),
             (1, -5, 4, 8, 8, 8), (1, 16, 4, None, None, 8),
             (1, 16, 0, 8, 8, 8), (1, 16, -3, 8, 8, 8), (1, 16, 0, 8, None, 8),      # m <= 0: nothing is launched, no pointer followed
             (3, 20000, 32, 8, 8, 8)]                                                # no workspace where one is needed
    want = [BAD_ARG] * 7 + [0] * 3 + [UNSUPPORTED]
    for args, code in zip(calls, want):
        got = lib.mcp_furthest_point_sampling_lengths_unpruned(*args, *tail)
        assert got == code == lib.mcp_furthest_point_sampling_lengths(*args, *tail), args
    # a workspace below b*n*4 is refused by both before anything is launched
    small = (3, 20000, 32, 8, 8, 8, None, 8, 3 * 20000 * 4 - 1, None)
    assert lib.mcp_furthest_point_sampling_lengths_unpruned(*small) == UNSUPPORTED == lib.mcp_furthest_point_sampling_lengths(*small)
