"""-m "not gpu": the length-aware EMD entry points (mcp_emd_lengths, mcp_emd_keep_lengths, mcp_emd_grad_lengths) are exported, bound
and validate their arguments without a GPU; the Python layer keeps the length-free autograd function as it was and evaluate()
has its raw_emd switch off by default."""
import inspect

import pytest
import torch

from mocopci_amd import _lib

ARGS = {"mcp_emd_lengths": 11, "mcp_emd_keep_lengths": 11, "mcp_emd_grad_lengths": 12}


def test_length_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name, nargs in ARGS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name]) == nargs, (name, len(_lib.SIGNATURES[name]))


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    none = (None,) * 8
    # the checks of mcp_emd / mcp_emd_keep / mcp_emd_grad: positive sizes, non-NULL clouds, cost, workspace, levels, grad_cost
    assert lib.mcp_emd_lengths(0, 16, 16, *none) == 10001
    assert lib.mcp_emd_lengths(1, 0, 16, *none) == 10001
    assert lib.mcp_emd_lengths(1, 16, -1, *none) == 10001
    assert lib.mcp_emd_lengths(1, 16, 16, *none) == 10001
    assert lib.mcp_emd_keep_lengths(0, 16, 16, *none) == 10001
    assert lib.mcp_emd_keep_lengths(1, 16, 16, *none) == 10001
    assert lib.mcp_emd_grad_lengths(1, 0, 16, *none, None) == 10001
    assert lib.mcp_emd_grad_lengths(1, 16, 16, *none, None) == 10001


def test_evaluate_has_raw_emd_off_by_default():
    from mocopci_amd import data
    p = inspect.signature(data.evaluate).parameters
    assert "raw_emd" in p and p["raw_emd"].default is False
    assert p["raw_gt"].default is False


def test_length_free_function_keeps_its_two_inputs():
    from mocopci_amd import emd
    assert list(inspect.signature(emd.EarthMoverDistanceFunction.forward).parameters) == ["ctx", "xyz1", "xyz2"]
    assert list(inspect.signature(emd.EarthMoverDistanceLengthsFunction.forward).parameters) == ["ctx", "xyz1", "xyz2", "len1", "len2"]
    for fn in (emd.earth_mover_distance, emd.approxmatch_forward, emd.EMD):
        p = inspect.signature(fn).parameters
        assert p["lengths1"].default is None and p["lengths2"].default is None, fn.__name__


def test_training_emd_loss_takes_gt_lengths():
    from mocopci_amd import training
    assert inspect.signature(training.emd_loss).parameters["gt_lengths"].default is None


def test_lengths_reject_host_clouds_and_bad_lengths():
    from mocopci_amd import emd, ops
    x, y = torch.zeros(2, 8, 3), torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError, match="float32 CUDA"):
        emd.earth_mover_distance(x, y, transpose=False, lengths1=[8, 8])
    with pytest.raises(RuntimeError, match="lengths"):
        ops.lengths_tensor([9, 8], 2, 8, "cpu")
    with pytest.raises(RuntimeError, match="lengths"):
        ops.lengths_tensor([8], 2, 8, "cpu")
