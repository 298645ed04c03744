"""-m "not gpu": the host side of the per-cloud lengths -- the two new entry points are exported and bound, host-side length
validation, the padded collate, and whole ground-truth frames from the dataset without disturbing the inputs' sample."""
import numpy as np
import pytest
import torch

from mocopci_amd import _lib, data, ops


def test_library_exports_and_binds_the_length_entry_points():
    lib = _lib.load()
    for name, nargs in (("mcp_knn_lengths", 12), ("mcp_chamfer_nn_lengths", 10)):
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name]) == nargs


def test_argument_validation_of_the_length_entry_points_needs_no_gpu():
    lib = _lib.load()
    assert lib.mcp_knn_lengths(1, 1, 1, 1, 0, None, None, None, None, None, None, None) == 10001
    assert lib.mcp_knn_lengths(1, 1, 0, 1, 0, 8, 8, 8, 8, 8, None, None) == 10001
    assert lib.mcp_knn_lengths(1, 1, 1, 1, 2, 8, 8, 8, 8, 8, None, None) == 10001     # no such distance form
    assert lib.mcp_knn_lengths(1, 1, 1, 33, 0, 8, 8, 8, 8, 8, None, None) == 10002
    assert lib.mcp_chamfer_nn_lengths(1, 1, 1, 8, 8, 8, 8, None, 8, None) == 10001
    assert lib.mcp_chamfer_nn_lengths(1, 0, 1, 8, 8, 8, 8, 8, 8, None) == 10001


@pytest.mark.parametrize("bad", [[3, -1], [3, 11], [3], [1, 2, 3], torch.tensor([3, 11]), torch.tensor([2.0, 3.0])])
def test_host_lengths_are_validated(bad):
    """A negative length, one beyond the cloud, a wrong count, a float tensor: RuntimeError before anything touches a device."""
    with pytest.raises(RuntimeError):
        ops.lengths_tensor(bad, 2, 10, "cpu")


def test_no_lengths_is_none():
    assert ops.lengths_tensor(None, 2, 10, "cpu") is None


def test_collate_padded():
    g = torch.Generator().manual_seed(0)
    sizes = [(300, 257, 900), (5, 1000, 900), (120, 1, 0)]
    batch = [([torch.rand(64, 3, generator=g) for _ in range(4)], [torch.rand(n, 3, generator=g) + 1 for n in row]) for row in sizes]
    inp, gt, lens = data.collate_padded(batch)
    assert len(inp) == 4 and all(t.shape == (3, 64, 3) for t in inp)
    for i in range(4):
        for b in range(3):
            assert torch.equal(inp[i][b], batch[b][0][i])
    assert [tuple(t.shape) for t in gt] == [(3, 300, 3), (3, 1000, 3), (3, 900, 3)]
    for j in range(3):
        assert lens[j].dtype == torch.int32 and lens[j].tolist() == [row[j] for row in sizes]
        for b in range(3):
            n = sizes[b][j]
            assert torch.equal(gt[j][b, :n], batch[b][1][j])
            assert not gt[j][b, n:].any()


def make_files(tmp_path, sizes=(900, 700, 400, 1200, 300, 257, 900)):
    rng = np.random.default_rng(3)
    names = []
    for i, n in enumerate(sizes):
        name = f"scene00_seq0001_frame{i:02d}.bin"
        data.write_frame(tmp_path / name, rng.normal(size=(n, 3)).astype(np.float32) * 20)
        names.append(name)
    lst = tmp_path / "list.txt"
    lst.write_text(" ".join(names) + "\n")
    return str(tmp_path), str(lst), names


def test_raw_gt_leaves_the_inputs_alone_and_returns_the_frames_whole(tmp_path):
    import os
    root, lst, names = make_files(tmp_path)
    np.random.seed(5)
    want_in, want_gt = data.NLDriveDataset(root, lst, num_points=512)[0]
    np.random.seed(5)
    got_in, got_gt = data.NLDriveDataset(root, lst, num_points=512, raw_gt=True)[0]
    assert len(got_in) == 4 and len(got_gt) == 3
    for a, b in zip(want_in, got_in):
        assert torch.equal(a, b)
    for j, t in enumerate(got_gt):
        raw = data.read_frame(os.path.join(root, names[4 + j]))
        assert t.dtype == torch.float32 and torch.equal(t, torch.from_numpy(raw))
    assert [t.shape[0] for t in got_gt] == [300, 257, 900] and all(t.shape == (512, 3) for t in want_gt)
    # and a batch of them collates
    inp, gt, lens = data.collate_padded([(got_in, got_gt), (want_in, [t[:100] for t in got_gt])])
    assert [tuple(t.shape) for t in gt] == [(2, 300, 3), (2, 257, 3), (2, 900, 3)] and [l.tolist() for l in lens] == [[300, 100], [257, 100], [900, 100]]
