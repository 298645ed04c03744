"""-m "not gpu": the host side of ball query under per-cloud lengths -- the three entry points (mcp_ball_query_lengths,
mcp_query_and_group_lengths, mcp_ball_query_pruned) are exported and bound with the header's argument counts, their argument
validation needs no device, the route rule of HipBackend.ball_query is a pure function of the padded shapes, and malformed host
lengths are refused by every new Python function before anything touches a device."""
import os
import re

import pytest
import torch

from mocopci_amd import _lib, compat, ops
from mocopci_amd import pointnet2_utils as pu

ENTRY_POINTS = {"mcp_ball_query_lengths": 12, "mcp_query_and_group_lengths": 14, "mcp_ball_query_pruned": 14}
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
    exhaustive = lambda b, n, m, ns, *ptrs: lib.mcp_ball_query_lengths(b, n, m, 1.0, ns, *ptrs, None)
    assert exhaustive(1, 1, 1, 1, None, p, p, p, p, p) == BAD_ARG          # no centres
    assert exhaustive(1, 1, 1, 1, p, None, p, p, p, p) == BAD_ARG          # no cloud
    assert exhaustive(1, 1, 1, 1, p, p, p, p, None, p) == BAD_ARG          # no idx
    assert exhaustive(1, 1, 1, 1, p, p, None, None, None, None) == BAD_ARG
    assert exhaustive(1, 0, 1, 1, p, p, p, p, p, p) == BAD_ARG             # n == 0
    assert exhaustive(1, 1, 0, 1, p, p, p, p, p, p) == BAD_ARG
    assert exhaustive(0, 1, 1, 1, p, p, p, p, p, p) == BAD_ARG
    assert exhaustive(1, 1, 1, 0, p, p, p, p, p, p) == BAD_ARG             # nsample == 0
    group = lambda b, n, m, c, ns, use_xyz, *ptrs: lib.mcp_query_and_group_lengths(b, n, m, c, 1.0, ns, use_xyz, *ptrs, None)
    assert group(1, 1, 1, 1, 1, 1, None, p, p, p, p, p) == BAD_ARG         # no cloud
    assert group(1, 1, 1, 1, 1, 1, p, None, p, p, p, p) == BAD_ARG         # no centres
    assert group(1, 1, 1, 1, 1, 1, p, p, p, p, p, None) == BAD_ARG         # no output
    assert group(1, 1, 1, 0, 1, 0, p, p, None, p, p, p) == BAD_ARG         # neither features nor coordinates: nothing to group
    assert group(1, 1, 1, 0, 1, 1, p, p, p, p, p, p) == BAD_ARG            # features without channels
    assert group(1, 0, 1, 1, 1, 1, p, p, p, p, p, p) == BAD_ARG            # n == 0
    assert group(1, 1, 1, 1, 0, 1, p, p, p, p, p, p) == BAD_ARG            # nsample == 0
    assert group(1, 1, 1, 1, 65, 1, p, p, p, p, p, p) == UNSUPPORTED
    assert group(1, 1, 1, 1, 65, 1, p, p, p, None, None, p) == UNSUPPORTED
    pruned = lambda b, n, m, ns, *ptrs: lib.mcp_ball_query_pruned(b, n, m, 1.0, ns, *ptrs, None)
    assert pruned(1, 1, 1, 1, None, p, p, p, p, p, p, p) == BAD_ARG        # no centres
    assert pruned(1, 1, 1, 1, p, None, p, p, p, p, p, p) == BAD_ARG        # no sorted cloud
    assert pruned(1, 1, 1, 1, p, p, None, p, p, p, p, p) == BAD_ARG        # no perm
    assert pruned(1, 1, 1, 1, p, p, p, None, p, p, p, p) == BAD_ARG        # no boxes
    assert pruned(1, 1, 1, 1, p, p, p, p, p, p, None, p) == BAD_ARG        # no idx
    assert pruned(1, 0, 1, 1, p, p, p, p, p, p, p, p) == BAD_ARG           # n == 0
    assert pruned(1, 1, 1, 0, p, p, p, p, p, p, p, p) == BAD_ARG           # nsample == 0
    assert pruned(1, 1, 1, 65, p, p, p, p, p, p, p, p) == UNSUPPORTED      # one list entry per lane
    assert pruned(1, 65537, 1, 1, p, p, p, p, p, p, p, p) == UNSUPPORTED   # 16 tile bounds per lane
    assert pruned(1, 65537, 1, 1, p, p, p, p, None, None, p, None) == UNSUPPORTED


def test_the_route_rule_is_a_function_of_the_padded_shapes(monkeypatch):
    cls = ops.HipBackend
    rule = cls.prunes_ball
    # the product's constants: no class of shapes is routed to a fresh cloud build, whatever the supported size
    assert not rule(2048, 16384, 16) and not rule(10 ** 6, 65536, 1) and not rule(2048, 40960, 8)
    assert cls.ball_prunable(65536, 64) and not cls.ball_prunable(65537, 64) and not cls.ball_prunable(65536, 65)
    monkeypatch.setattr(cls, "BALL_PRUNE_MIN_REFS", 8192)
    monkeypatch.setattr(cls, "BALL_PRUNE_MIN_CENTRES", 1024)
    assert rule(1024, 8192, 1) and rule(1024, 8192, 64) and rule(10 ** 6, 8192, 16)
    assert not rule(1023, 8192, 16) and not rule(1024, 8191, 16) and not rule(1024, 8192, 65)
    assert rule(1024, 65536, 16) and not rule(1024, 65537, 16)


def test_the_rule_follows_its_own_class_attributes(monkeypatch):
    cls = ops.HipBackend
    monkeypatch.setattr(cls, "BALL_PRUNE_MIN_REFS", 100)
    monkeypatch.setattr(cls, "BALL_PRUNE_MIN_CENTRES", 7)
    assert not cls.prunes_ball(6, 100, 8) and not cls.prunes_ball(7, 99, 8) and cls.prunes_ball(7, 100, 8) and not cls.prunes_ball(7, 100, 65)
    monkeypatch.setattr(cls, "BALL_PRUNE_MIN_REFS", 1 << 30)
    assert not cls.prunes_ball(10 ** 6, 65536, 1)
    assert cls.PRUNE_LENGTHS_MIN_REFS == 8192 and cls.PRUNE_MIN_REFS == 2048   # the KNN rules keep their own


@pytest.mark.parametrize("bad", [[3], [1, 2, 3], [1, 11], [-1, 2], [1.0, 2.0], torch.tensor([True, False])])
def test_lengths_errors_surface_from_the_new_python_functions(bad):
    """lengths_tensor validates host lengths (one integer per element, 0 <= len <= the padded size) before any tensor is checked or
    any kernel is launched, so CPU tensors are enough to see its error."""
    xyz, new_xyz = torch.zeros(2, 10, 3), torch.zeros(2, 10, 3)
    calls = [lambda: ops.HipBackend().ball_query(xyz, new_xyz, 1.0, 4, xyz_lengths=bad),
             lambda: ops.HipBackend().ball_query(xyz, new_xyz, 1.0, 4, new_xyz_lengths=bad),
             lambda: pu.ball_query(1.0, 4, xyz, new_xyz, bad, None),
             lambda: pu.ball_query(1.0, 4, xyz, new_xyz, None, bad),
             lambda: pu.QueryAndGroup(1.0, 4)(xyz, new_xyz, None, xyz_lengths=bad),
             lambda: pu.QueryAndGroup(1.0, 4)(xyz, new_xyz, None, new_xyz_lengths=bad),
             lambda: pu.three_nn(new_xyz, xyz, bad, None),
             lambda: pu.three_nn(new_xyz, xyz, None, bad),
             lambda: compat.ball_query(new_xyz, xyz, lengths1=bad, K=4, radius=1.0),
             lambda: compat.ball_query(new_xyz, xyz, lengths2=bad, K=4, radius=1.0)]
    for call in calls:
        with pytest.raises(RuntimeError, match="lengths"):
            call()
