"""-m "not gpu": the host side of the pruned search under per-cloud lengths -- the four entry points are exported and bound with
the header's argument counts, their argument validation needs no device, and the size rule of HipBackend.knn with lengths is a pure
function of the padded shapes."""
import os
import re

import pytest

from mocopci_amd import _lib, ops

ENTRY_POINTS = {"mcp_build_cloud_lengths": 8, "mcp_morton_codes_lengths": 7, "mcp_tile_boxes_lengths": 6, "mcp_knn_pruned_lengths": 15}
BAD_ARG, UNSUPPORTED = 10001, 10002


def test_library_exports_and_binds_the_entry_points_with_the_headers_argument_counts():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mocopci_hip.h")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name]) == nargs
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in the header"
        assert len(decl.group(1).split(",")) == nargs


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    p = 8   # any non-null pointer: nothing is launched
    assert lib.mcp_build_cloud_lengths(1, 1, None, p, p, p, p, None) == BAD_ARG
    assert lib.mcp_build_cloud_lengths(1, 1, None, None, p, p, p, None) == BAD_ARG        # null lengths: the plain entry point's check
    assert lib.mcp_build_cloud_lengths(1, 0, p, p, p, p, p, None) == BAD_ARG
    assert lib.mcp_build_cloud_lengths(1, 1, p, p, p, p, None, None) == BAD_ARG
    assert lib.mcp_build_cloud_lengths(1, 16385, p, p, p, p, p, None) == UNSUPPORTED
    assert lib.mcp_build_cloud_lengths(1, 16385, p, None, p, p, p, None) == UNSUPPORTED
    assert lib.mcp_morton_codes_lengths(1, 1, p, None, p, p, None) == BAD_ARG
    assert lib.mcp_morton_codes_lengths(0, 1, p, p, p, p, None) == BAD_ARG
    assert lib.mcp_morton_codes_lengths(1, 1, p, p, None, None, None) == BAD_ARG
    assert lib.mcp_tile_boxes_lengths(1, 1, None, p, p, None) == BAD_ARG
    assert lib.mcp_tile_boxes_lengths(1, 1, p, p, None, None) == BAD_ARG
    assert lib.mcp_tile_boxes_lengths(1, 0, p, None, p, None) == BAD_ARG
    search = lambda b, q, n, k, form, *ptrs: lib.mcp_knn_pruned_lengths(b, q, n, k, form, *ptrs, None)
    assert search(1, 1, 1, 1, 0, None, p, p, p, p, p, p, p, None) == BAD_ARG               # no queries
    assert search(1, 1, 1, 1, 0, p, p, p, None, p, p, p, p, None) == BAD_ARG               # no reference perm
    assert search(1, 1, 1, 1, 0, p, p, p, p, p, p, p, None, None) == BAD_ARG               # no idx
    assert search(1, 1, 1, 1, 0, p, p, p, p, p, None, None, None, None) == BAD_ARG         # ... through the plain entry point
    assert search(1, 1, 0, 1, 0, p, p, p, p, p, p, p, p, None) == BAD_ARG
    assert search(1, 1, 1, 1, 2, p, p, p, p, p, p, p, p, None) == BAD_ARG                  # no such distance form
    assert search(1, 1, 1, 64, 0, p, p, p, p, p, p, p, p, None) == UNSUPPORTED
    assert search(1, 1, 1, 33, 1, p, p, p, p, p, p, None, p, None) == UNSUPPORTED
    assert search(1, 1, 65537, 1, 1, p, p, p, p, p, None, p, p, None) == UNSUPPORTED       # 16-bit candidate indices
    assert search(1, 1, 65537, 1, 1, p, p, p, p, p, None, None, p, None) == UNSUPPORTED


def test_the_size_rule_is_a_function_of_the_padded_shapes():
    cls = ops.HipBackend
    rule = cls.prunes_with_lengths
    nq, nr = cls.PRUNE_LENGTHS_MIN_QUERIES, cls.PRUNE_LENGTHS_MIN_REFS
    assert rule(nq, nr, 1) and rule(nq, nr, 32) and rule(10 ** 6, nr, 1)
    assert not rule(nq - 1, nr, 1) and not rule(nq, nr - 1, 1) and not rule(nq, nr, 33)
    assert rule(nq, 65536, 1) and not rule(nq, 65537, 1) and rule(65537, 65536, 32)
    assert rule(nq, 16384, 32) and rule(nq, 16385, 32)   # either builder route


def test_the_rule_follows_its_own_class_attributes(monkeypatch):
    cls = ops.HipBackend
    monkeypatch.setattr(cls, "PRUNE_LENGTHS_MIN_REFS", 4096)
    monkeypatch.setattr(cls, "PRUNE_LENGTHS_MIN_QUERIES", 2048)
    assert not cls.prunes_with_lengths(2047, 4096, 1) and not cls.prunes_with_lengths(2048, 4095, 1) and cls.prunes_with_lengths(2048, 4096, 1)
    assert cls.PRUNE_MIN_REFS == 2048 and cls.PRUNE_MIN_QUERIES == 1024   # the length-free rule keeps its own
