"""-m "not gpu": the length-aware furthest point sampling (mcp_furthest_point_sampling_lengths, mcp_fps_lengths_workspace_bytes) is
declared, exported and bound; its argument checks and its workspace query answer without a GPU; HipBackend.fps validates host
lengths before it loads anything; compat.sample_farthest_points has pytorch3d's signature and refuses a random start."""
import inspect
import os
import re

import pytest
import torch

from mocopci_amd import _lib, compat, data, ops

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mocopci_hip.h")
ARGS = {"mcp_fps_lengths_workspace_bytes": 3, "mcp_furthest_point_sampling_lengths": 10}
BAD_ARG = 10001


def test_entry_points_are_declared_exported_and_bound():
    with open(HEADER) as fh:
        header = re.sub(r"\s+", " ", fh.read())
    assert "size_t mcp_fps_lengths_workspace_bytes(int b, int n, int m);" in header
    assert ("int mcp_furthest_point_sampling_lengths(int b, int n, int m, const float *xyz, const int *len, int *idx, float *sampled_xyz, "
            "void *workspace, size_t workspace_bytes, mcp_stream_t stream);") in header
    lib = _lib.load()
    for name, nargs in ARGS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name]) == nargs, (name, len(_lib.SIGNATURES[name]))


def test_argument_validation_needs_no_gpu():
    fps = _lib.load().mcp_furthest_point_sampling_lengths
    tail = (None, None, 0, None)                               # sampled_xyz, workspace, workspace_bytes, stream
    assert fps(1, 16, 4, None, 8, 8, *tail) == BAD_ARG         # NULL xyz
    assert fps(1, 16, 4, 8, 8, None, *tail) == BAD_ARG         # NULL idx
    assert fps(0, 16, 4, 8, 8, 8, *tail) == BAD_ARG
    assert fps(-1, 16, 4, 8, 8, 8, *tail) == BAD_ARG
    assert fps(1, 0, 4, 8, 8, 8, *tail) == BAD_ARG
    assert fps(1, -5, 4, 8, 8, 8, *tail) == BAD_ARG
    assert fps(1, 16, 4, None, None, 8, *tail) == BAD_ARG      # ... also on the way to the length-free call
    # m <= 0 is the reference's early return (nothing is launched, no pointer is followed)
    assert fps(1, 16, 0, 8, 8, 8, *tail) == 0
    assert fps(1, 16, -3, 8, 8, 8, *tail) == 0
    assert fps(1, 16, 0, 8, None, 8, *tail) == 0


def test_workspace_query():
    lib = _lib.load()
    query = lib.mcp_fps_lengths_workspace_bytes
    assert query(8, 16384, 64) == 0 and query(1, 1, 1) == 0 and query(8, 2100, 48) == 0
    assert query(8, 16385, 64) == 8 * 16385 * 4
    assert query(3, 20000, 32) == 3 * 20000 * 4
    assert query(40000, 20000, 32) == 40000 * 20000 * 4        # beyond 2^31 bytes: the result is a size_t
    assert query(0, 20000, 32) == 0


@pytest.mark.parametrize("bad", [[9, 8], [8, -1], [8], [8, 8, 8], torch.tensor([8, 9]), torch.tensor([1.0, 2.0])])
def test_backend_validates_host_lengths_before_anything_is_loaded(bad, monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the lengths were validated")
    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(RuntimeError, match="lengths"):
        ops.HipBackend().fps(torch.zeros(2, 8, 3), 4, lengths=bad)
    with pytest.raises(RuntimeError, match="lengths"):
        ops.HipBackend().fps(torch.zeros(2, 8, 3), 4, with_points=True, lengths=bad)


def test_backend_signature_keeps_the_length_free_call():
    p = inspect.signature(ops.HipBackend.fps).parameters
    assert list(p) == ["self", "xyz", "npoint", "with_points", "lengths"]
    assert p["with_points"].default is False and p["lengths"].default is None


def test_compat_sample_farthest_points_signature():
    p = inspect.signature(compat.sample_farthest_points).parameters
    assert list(p) == ["points", "lengths", "K", "random_start_point"]
    assert p["lengths"].default is None and p["K"].default == 50 and p["random_start_point"].default is False
    with pytest.raises(NotImplementedError, match="random_start_point"):
        compat.sample_farthest_points(torch.zeros(1, 8, 3), None, 4, random_start_point=True)
    assert "tie rule" in compat.sample_farthest_points.__doc__


def test_data_path_switches():
    p = inspect.signature(data.evaluate).parameters
    assert p["gt_points"].default is None and p["raw_gt"].default is False and p["raw_emd"].default is False
    assert list(inspect.signature(data.downsample_padded).parameters) == ["clouds", "lengths", "num_points"]
