"""The Chamfer distance over the valid prefixes of a padded batch (HipBackend.chamfer(x_lengths=, y_lengths=)): value against the
CPU oracle on each element's prefixes, gradients against the length-free chamfer run per element on the sliced clouds, exact
zeros beyond a length, bitwise independence of the padding's contents, the drop-in chamfer_distance and evaluate(raw_gt=True)."""
import os

import numpy as np
import pytest
import torch

from mocopci_amd import compat, data, ops, training
from oracle import pointset as orc
from tests.test_knn_lengths_gpu import cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

B, N, M = 3, 300, 257
XLEN, YLEN = (300, 17, 1), (257, 257, 2)


def padded_clouds(filling=0):
    """x (B,N,3), y (B,M,3); rows beyond XLEN[b] / YLEN[b] are padding: 1e30 in x and copies of live x points in y (an unmasked
    search finds them at distance 0), or NaN / -5e29 with filling=1."""
    x, y = cloud(80, B, N), cloud(81, B, M)
    for b in range(B):
        xl, yl = XLEN[b], YLEN[b]
        y[b, yl:] = x[b, torch.arange(M - yl) % xl] if filling == 0 else -5e29
        x[b, xl:] = 1e30 if filling == 0 else float("nan")
    return x, y


@pytest.fixture(scope="module")
def clouds():
    return padded_clouds()


@pytest.fixture(scope="module")
def oracle_values(clouds):
    x, y = clouds
    return [orc.chamfer(x[b:b + 1, :XLEN[b]], y[b:b + 1, :YLEN[b]]) for b in range(B)]


@pytest.fixture(scope="module")
def grads(clouds):
    """Gradients of the mean value w.r.t. x and y through the length-aware path."""
    return run_grads(*clouds)


def run_grads(x, y, y_grad=True):
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(y_grad)
    v = ops.backend().chamfer(xd, yd, x_lengths=list(XLEN), y_lengths=list(YLEN))
    return torch.autograd.grad(v, [xd, yd] if y_grad else [xd])


def test_value_matches_oracle_on_the_prefixes(clouds, oracle_values):
    x, y = clouds
    want = float(np.mean(oracle_values))
    got = float(ops.backend().chamfer(x.to(DEV), y.to(DEV), x_lengths=list(XLEN), y_lengths=list(YLEN)))
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    # the differentiable path computes the same value
    got = float(ops.backend().chamfer(x.to(DEV).requires_grad_(True), y.to(DEV), x_lengths=list(XLEN), y_lengths=list(YLEN)).detach())
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)


@pytest.mark.parametrize("with_grad", [False, True])
def test_per_sample_values(clouds, oracle_values, with_grad):
    x, y = clouds
    got = ops.backend().chamfer(x.to(DEV).requires_grad_(with_grad), y.to(DEV), per_sample=True, x_lengths=torch.tensor(XLEN),
                                y_lengths=torch.tensor(YLEN, device=DEV))
    assert got.shape == (B,)
    for b in range(B):
        assert abs(float(got[b].detach()) - oracle_values[b]) <= 1e-6 * abs(oracle_values[b]), (b, float(got[b].detach()), oracle_values[b])


def test_gradients_match_the_length_free_chamfer_on_the_slices(clouds, grads):
    x, y = clouds
    gx, gy = (g.cpu() for g in grads)
    for b in range(B):
        xl, yl = XLEN[b], YLEN[b]
        xs, ys = x[b:b + 1, :xl].to(DEV).requires_grad_(True), y[b:b + 1, :yl].to(DEV).requires_grad_(True)
        wx, wy = (g.cpu() / B for g in torch.autograd.grad(ops.backend().chamfer(xs, ys), [xs, ys]))
        for name, got, want in (("x", gx[b, :xl], wx[0]), ("y", gy[b, :yl], wy[0])):
            torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-6 * float(want.abs().max()) + 1e-9, msg=lambda m: f"d{name}[{b}]: {m}")
        assert not gx[b, xl:].any() and not gy[b, yl:].any(), f"gradient rows beyond the lengths of element {b} are not exact zeros"


def test_gradients_are_deterministic_and_blind_to_the_padding(grads):
    again = run_grads(*padded_clouds())
    other = run_grads(*padded_clouds(filling=1))
    for g, a, o in zip(grads, again, other):
        assert torch.equal(g, a), "two calls differ"
        assert torch.equal(g, o), "the padding's contents reached a gradient"


def test_ground_truth_without_requires_grad(clouds, grads):
    (gx,) = run_grads(*clouds, y_grad=False)
    assert torch.equal(gx, grads[0])
    x, y = clouds
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV)
    ops.backend().chamfer(xd, yd, x_lengths=list(XLEN), y_lengths=list(YLEN)).backward()
    assert yd.grad is None and torch.equal(xd.grad, gx)
    # training.chamfer_loss passes the ground truth's lengths through (gt in train.py's (B,3,n) layout)
    xd2 = cloud(83, B, 50).to(DEV).requires_grad_(True)
    v = training.chamfer_loss(xd2, yd.transpose(1, 2), gt_lengths=list(YLEN))
    w = ops.backend().chamfer(xd2, yd, y_lengths=list(YLEN))
    assert torch.equal(v, w)


def test_lengths_none_is_todays_chamfer():
    x, y = cloud(80, B, N).to(DEV), cloud(81, B, M).to(DEV)
    be = ops.backend()
    assert torch.equal(be.chamfer(x, y, x_lengths=None, y_lengths=None), be.chamfer(x, y))
    assert torch.equal(be.chamfer(x, y, per_sample=True, x_lengths=None, y_lengths=None), be.chamfer(x, y, per_sample=True))
    xg = x.clone().requires_grad_(True)
    a = torch.autograd.grad(be.chamfer(xg, y, x_lengths=None, y_lengths=None), xg)[0]
    assert torch.equal(a, torch.autograd.grad(be.chamfer(xg, y), xg)[0])
    # full lengths: the same neighbours, so the same distances; only the order of the row sums may differ
    full = be.chamfer(x, y, per_sample=True, x_lengths=[N] * B, y_lengths=[M] * B)
    torch.testing.assert_close(full, be.chamfer(x, y, per_sample=True), rtol=1e-6, atol=0)


def test_compat_chamfer_distance(clouds):
    x, y = (t.to(DEV) for t in clouds)
    loss, normals = compat.chamfer_distance(x, y, x_lengths=torch.tensor(XLEN), y_lengths=torch.tensor(YLEN))
    assert normals is None and torch.equal(loss, ops.backend().chamfer(x, y, x_lengths=list(XLEN), y_lengths=list(YLEN)))
    a, b = cloud(80, B, N).to(DEV), cloud(81, B, M).to(DEV)
    loss, normals = compat.chamfer_distance(a, b)
    assert normals is None and torch.equal(loss, ops.backend().chamfer(a, b))


def test_evaluate_against_whole_ground_truth_frames(tmp_path):
    """evaluate(raw_gt=True) on two sequences whose ground-truth frames hold 300 / 257 / 900 points (in two orders, so the batch is
    padded), at the point count of tests/test_data.py's evaluate test: finite Chamfer values that equal the unpadded per-sequence
    Chamfer distance of the same predictions, and no EMD."""
    from torch.utils.data import DataLoader
    from tests import harness_checks as hc
    rng = np.random.default_rng(0)
    lines, gt_sizes = [], [(300, 257, 900), (900, 300, 257)]
    for s, gts in enumerate(gt_sizes):
        names = []
        for i, n in enumerate((2500, 2048, 2048, 2100) + gts):
            names.append(f"scene00_seq{s:04d}_frame{i:02d}.bin")
            data.write_frame(tmp_path / names[-1], rng.normal(size=(n, 3)).astype(np.float32) * 20)
        lines.append(" ".join(names))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    ds = data.NLDriveDataset(str(tmp_path), str(tmp_path / "list.txt"), num_points=2048, raw_gt=True)
    net, outs = hc.build_model(DEV), []

    def recording(a, b):
        outs.append(net(a, b))
        return outs[-1]

    np.random.seed(0)
    res = data.evaluate(recording, DataLoader(ds, batch_size=2, collate_fn=data.collate_padded), device=DEV, raw_gt=True)
    assert res["sequences"] == 2 and res["emd"] is None and res["seconds_per_forward"] > 0 and len(outs) == 1
    assert all(np.isfinite(res["chamfer"]))
    for j in range(3):
        per_seq = []
        for s in range(2):
            raw = torch.from_numpy(data.read_frame(os.path.join(str(tmp_path), lines[s].split(" ")[4 + j]))).to(DEV)
            assert raw.shape[0] == gt_sizes[s][j]
            per_seq.append(float(ops.backend().chamfer(outs[0][j][s:s + 1].contiguous(), raw[None].contiguous())))
        want = float(np.mean(per_seq))
        assert abs(res["chamfer"][j] - want) <= 1e-6 * abs(want), (j, res["chamfer"][j], want)
