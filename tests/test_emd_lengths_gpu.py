"""The EMD metric over the valid prefixes of a padded batch (emd.earth_mover_distance / approxmatch_forward / EMD with lengths1 /
lengths2, mcp_emd_lengths / mcp_emd_keep_lengths / mcp_emd_grad_lengths): cost against the CPU oracle on each element's prefixes,
cost / match / gradients bit for bit against the length-free kernels on the sliced clouds, exact zeros beyond a length, bitwise
independence of the padding's contents, the unchanged length-free path, the wrappers and evaluate(raw_gt=True, raw_emd=True).

One padded batch serves every test.  emd.hip streams tiles of 1024 with 256-lane workgroups, emd_grad.hip tiles of 512 in 64-entry
wave slices; the lengths sit on and beside those boundaries, with the mass ratio (integer division of the two counts,
emd_kernel.cu:32-38) at 1, multiL = 2 (element 2) and 3 (elements 3, 4), a one-point cloud, an empty cloud on either side and
equal lengths.  1025 / 513 is 1 in integer division, so a second, smaller batch (RATIO_*) adds multiR = 2 and 4."""
import os

import numpy as np
import pytest
import torch

from mocopci_amd import data, emd, ops, training
from oracle import pointset as orc
# the float64 gradient yardstick is the one of tests/test_emd_grad.py, imported so that both files measure with the same code
from tests.test_emd_grad import assert_within, grads_from_match

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

B, N, M = 8, 1300, 2100
LEN1 = [1300, 1025, 1024, 257, 1, 600, 0, 700]
LEN2 = [2100, 513, 2049, 1023, 3, 0, 900, 700]
GRAD_COST = [1.7, -0.6, 2.5, 1.3, 0.9, -1.1, 0.4, 0.0]   # non-uniform, one zero entry
LIVE = [b for b in range(B) if LEN1[b] and LEN2[b]]

RATIO_N, RATIO_M, RATIO_LEN1, RATIO_LEN2 = 1100, 600, [1026, 1100], [513, 275]   # multiR = 2 and 4


def padded_clouds(filling=0):
    """x (B,N,3), y (B,M,3) in [0,4)^3; rows beyond LEN1[b] / LEN2[b] are padding: zeros, NaN (filling=1), or 1e30 in x and copies
    of live x points in y (filling=2; -5e29 where x has no live point)."""
    gen = torch.Generator().manual_seed(20)
    x, y = torch.rand(B, N, 3, generator=gen) * 4, torch.rand(B, M, 3, generator=gen) * 4
    for b in range(B):
        xl, yl = LEN1[b], LEN2[b]
        if filling == 0:
            x[b, xl:], y[b, yl:] = 0.0, 0.0
        elif filling == 1:
            x[b, xl:], y[b, yl:] = float("nan"), float("nan")
        else:
            y[b, yl:] = x[b, torch.arange(M - yl) % xl] if xl else -5e29
            x[b, xl:] = 1e30
    return x, y


def run_lengths(x, y, len1=LEN1, len2=LEN2, grad_cost=GRAD_COST):
    """Everything the length-aware path computes: cost (no gradient), cost of the level-keeping forward, match, both gradients."""
    xd, yd = x.to(DEV), y.to(DEV)
    cost = emd.earth_mover_distance(xd, yd, transpose=False, lengths1=len1, lengths2=len2)
    match = emd.approxmatch_forward(xd, yd, lengths1=len1, lengths2=len2)
    xg, yg = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    kept = emd.earth_mover_distance(xg, yg, transpose=False, lengths1=len1, lengths2=len2)
    assert "Lengths" in type(kept.grad_fn).__name__
    g1, g2 = torch.autograd.grad(kept, (xg, yg), torch.tensor(grad_cost, device=DEV))
    return {"cost": cost, "kept": kept.detach(), "match": match, "g1": g1, "g2": g2}


def run_slice(xs, ys, g):
    """The length-free kernels on one element's contiguous prefixes (1,xl,3), (1,yl,3)."""
    xs, ys = xs.contiguous().to(DEV), ys.contiguous().to(DEV)
    cost = emd.earth_mover_distance(xs, ys, transpose=False)
    match = emd.approxmatch_forward(xs, ys)
    xg, yg = xs.clone().requires_grad_(True), ys.clone().requires_grad_(True)
    kept = emd.EarthMoverDistanceFunction.apply(xg, yg)
    g1, g2 = torch.autograd.grad(kept, (xg, yg), torch.tensor([g], device=DEV))
    return {"cost": cost, "kept": kept.detach(), "match": match, "g1": g1, "g2": g2}


@pytest.fixture(scope="module")
def clouds():
    return padded_clouds()


@pytest.fixture(scope="module")
def got(clouds):
    return run_lengths(*clouds)


@pytest.fixture(scope="module")
def slices(clouds):
    x, y = clouds
    return {b: run_slice(x[b:b + 1, :LEN1[b]], y[b:b + 1, :LEN2[b]], GRAD_COST[b]) for b in LIVE}


def test_cost_matches_the_oracle_on_the_prefixes(clouds, got):
    x, y = clouds
    cost = got["cost"].cpu()
    for b in range(B):
        if b not in LIVE:
            assert float(cost[b]) == 0.0, (b, float(cost[b]))
            continue
        want = orc.earth_mover_distance(x[b:b + 1, :LEN1[b]].contiguous(), y[b:b + 1, :LEN2[b]].contiguous())
        print(f"\nelement {b} ({LEN1[b]}, {LEN2[b]}): cost {float(cost[b]):.6f}, oracle {float(want):.6f}")
        torch.testing.assert_close(cost[b:b + 1], want, rtol=1e-5, atol=1e-6)   # tests/test_emd.py's north_star tolerance


def test_cost_equals_the_length_free_kernel_on_the_slices(got, slices):
    for b in LIVE:
        assert torch.equal(got["cost"][b:b + 1], slices[b]["cost"]), (b, float(got["cost"][b]), float(slices[b]["cost"]))
        assert torch.equal(slices[b]["kept"], slices[b]["cost"])
    assert torch.equal(got["kept"], got["cost"]), "the level-keeping forward gives other bits"


def test_match_block_equals_the_slice_and_the_rest_is_zero(got, slices):
    match = got["match"]
    assert match.shape == (B, M, N)
    outside = match.clone()
    for b in LIVE:
        xl, yl = LEN1[b], LEN2[b]
        assert torch.equal(match[b, :yl, :xl], slices[b]["match"][0]), b
        outside[b, :yl, :xl] = 0
    assert int(torch.count_nonzero(outside)) == 0, "a match entry outside the [:len2, :len1] blocks is not zero"


def test_gradients_equal_the_length_free_function_on_the_slices(got, slices):
    g1, g2 = got["g1"], got["g2"]
    assert g1.shape == (B, N, 3) and g2.shape == (B, M, 3)
    for b in range(B):
        if b not in LIVE:
            assert int(torch.count_nonzero(g1[b])) == 0 and int(torch.count_nonzero(g2[b])) == 0, f"element {b} has an empty side"
            continue
        xl, yl = LEN1[b], LEN2[b]
        assert torch.equal(g1[b, :xl], slices[b]["g1"][0]), f"grad1 of element {b}"
        assert torch.equal(g2[b, :yl], slices[b]["g2"][0]), f"grad2 of element {b}"
        assert int(torch.count_nonzero(g1[b, xl:])) == 0 and int(torch.count_nonzero(g2[b, yl:])) == 0, f"padded rows of element {b}"
        if GRAD_COST[b] != 0.0:
            assert float(g1[b].abs().max()) > 0 and float(g2[b].abs().max()) > 0
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all())


def test_gradients_match_float64_on_the_device_match(clouds, got):
    """tests/test_emd_grad.py's yardstick: float64 gradients at the fixed (zero-padded) match of the length-aware forward."""
    x, y = clouds
    w1, w2 = grads_from_match(torch.tensor(GRAD_COST, device=DEV), x.to(DEV), y.to(DEV), got["match"])
    assert_within(got["g1"], w1, 1e-5)
    assert_within(got["g2"], w2, 1e-5)


def test_single_input_gradient_and_determinism(clouds, got):
    x, y = clouds
    again = run_lengths(x, y)
    for key in ("cost", "kept", "g1", "g2"):
        assert torch.equal(again[key], got[key]), f"two runs differ in {key}"
    g = torch.tensor(GRAD_COST, device=DEV)
    xg, yd = x.to(DEV).requires_grad_(True), y.to(DEV)
    emd.earth_mover_distance(xg, yd, transpose=False, lengths1=LEN1, lengths2=LEN2).backward(g)
    assert yd.grad is None and torch.equal(xg.grad, got["g1"])
    xd, yg = x.to(DEV), y.to(DEV).requires_grad_(True)
    len1, len2 = ops.lengths_tensor(LEN1, B, N, DEV), ops.lengths_tensor(LEN2, B, M, DEV)
    c = emd.EarthMoverDistanceLengthsFunction.apply(xd, yg, len1, len2)
    outs = c.grad_fn.apply(g)                                      # the function's own backward outputs
    assert outs[0] is None and torch.equal(outs[1], got["g2"]) and outs[2] is None and outs[3] is None


@pytest.mark.parametrize("filling", [1, 2])
def test_padding_is_never_read(got, filling):
    other = run_lengths(*padded_clouds(filling))
    for key in ("cost", "kept", "match", "g1", "g2"):
        assert torch.equal(other[key], got[key]), f"the padding's contents reached {key}"


def test_lengths_none_and_full_lengths_are_todays_path(clouds):
    x, y = (t.to(DEV) for t in clouds)
    g = torch.tensor(GRAD_COST, device=DEV)
    plain = emd.earth_mover_distance(x, y, transpose=False)
    assert torch.equal(emd.earth_mover_distance(x, y, transpose=False, lengths1=None, lengths2=None), plain)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    c = emd.earth_mover_distance(xg, yg, transpose=False, lengths1=None, lengths2=None)
    assert type(c.grad_fn).__name__.startswith("EarthMoverDistanceFunction")
    p1, p2 = torch.autograd.grad(c, (xg, yg), g)
    assert torch.equal(c.detach(), plain)
    # full lengths, and a device int64 tensor whose entries exceed N / M (clamped in the kernel), and one side only
    for len1, len2 in (([N] * B, [M] * B), (torch.full((B,), N + 7, device=DEV), torch.full((B,), 1 << 20, device=DEV)),
                       (None, [M] * B), (torch.tensor([N] * B, dtype=torch.int32), None)):
        assert torch.equal(emd.earth_mover_distance(x, y, transpose=False, lengths1=len1, lengths2=len2), plain)
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        c = emd.earth_mover_distance(xg, yg, transpose=False, lengths1=len1, lengths2=len2)
        f1, f2 = torch.autograd.grad(c, (xg, yg), g)
        assert torch.equal(c.detach(), plain) and torch.equal(f1, p1) and torch.equal(f2, p2)


def test_mass_ratio_on_the_right_side():
    """multiR = 2 (1026 / 513) and 4 (1100 / 275): cost and gradients bit for bit the length-free ones on the slices."""
    gen = torch.Generator().manual_seed(21)
    x, y = torch.rand(2, RATIO_N, 3, generator=gen) * 4, torch.rand(2, RATIO_M, 3, generator=gen) * 4
    for b in range(2):
        x[b, RATIO_LEN1[b]:], y[b, RATIO_LEN2[b]:] = float("nan"), float("nan")
    g = [0.8, -1.4]
    res = run_lengths(x, y, RATIO_LEN1, RATIO_LEN2, g)
    for b in range(2):
        xl, yl = RATIO_LEN1[b], RATIO_LEN2[b]
        want = run_slice(x[b:b + 1, :xl], y[b:b + 1, :yl], g[b])
        assert torch.equal(res["cost"][b:b + 1], want["cost"]) and torch.equal(res["kept"][b:b + 1], want["cost"])
        assert torch.equal(res["match"][b, :yl, :xl], want["match"][0])
        assert torch.equal(res["g1"][b, :xl], want["g1"][0]) and torch.equal(res["g2"][b, :yl], want["g2"][0])
        assert int(torch.count_nonzero(res["g1"][b, xl:])) == 0 and int(torch.count_nonzero(res["g2"][b, yl:])) == 0
        ocost = orc.earth_mover_distance(x[b:b + 1, :xl].contiguous(), y[b:b + 1, :yl].contiguous())
        torch.testing.assert_close(res["cost"][b:b + 1].cpu(), ocost, rtol=1e-5, atol=1e-6)


def test_wrappers(clouds, got):
    x, y = (t.to(DEV) for t in clouds)
    pc1, pc2 = x.transpose(1, 2).contiguous(), y.transpose(1, 2).contiguous()   # (B,3,N), (B,3,M)
    # transpose=True layout
    assert torch.equal(emd.earth_mover_distance(pc1, pc2, transpose=True, lengths1=LEN1, lengths2=LEN2), got["cost"])
    a = pc1.clone().requires_grad_(True)
    emd.earth_mover_distance(a, pc2, lengths1=LEN1, lengths2=LEN2).backward(torch.tensor(GRAD_COST, device=DEV))
    assert a.grad.shape == pc1.shape and torch.equal(a.grad, got["g1"].transpose(1, 2))
    # EMD(): mean_b(cost_b / max(len1_b, 1))
    want = torch.mean(got["cost"] / torch.tensor([max(v, 1) for v in LEN1], device=DEV, dtype=torch.float32))
    torch.testing.assert_close(emd.EMD(pc1, pc2, lengths1=LEN1, lengths2=LEN2), want, rtol=1e-6, atol=0)
    # lengths2 only: every point of pc1 counts
    c2 = emd.earth_mover_distance(x, y, transpose=False, lengths2=LEN2)
    torch.testing.assert_close(emd.EMD(pc1, pc2, lengths2=LEN2), torch.mean(c2 / N), rtol=1e-6, atol=0)
    # training.emd_loss passes the ground truth's lengths through (pred (B,n,3), gt (B,3,n)) and is differentiable
    pred = x.clone().requires_grad_(True)
    loss = training.emd_loss(pred, pc2, gt_lengths=LEN2)
    assert torch.equal(loss.detach(), emd.EMD(pc1, pc2, lengths2=LEN2))
    loss.backward()
    assert pred.grad.shape == x.shape and bool(torch.isfinite(pred.grad).all())
    # without lengths EMD is the reference's mean(cost) / N
    full = emd.EMD(pc1, pc1)
    assert torch.equal(full, torch.mean(emd.earth_mover_distance(x, x, transpose=False)) / N)


def test_evaluate_reports_emd_against_whole_ground_truth_frames(tmp_path):
    """evaluate(raw_gt=True, raw_emd=True) on the two-sequence setup of tests/test_chamfer_lengths_gpu.py (ground-truth frames of
    300 / 257 / 900 points in two orders, so the batch is padded): "emd" is finite and equals the unpadded per-sequence EMD of
    the same predictions; with raw_emd left out it is still None."""
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
    loader = DataLoader(ds, batch_size=2, collate_fn=data.collate_padded)
    res = data.evaluate(recording, loader, device=DEV, raw_gt=True, raw_emd=True)
    assert res["sequences"] == 2 and len(outs) == 1 and len(res["emd"]) == 3
    assert all(np.isfinite(res["emd"])) and all(np.isfinite(res["chamfer"]))
    for j in range(3):
        per_seq = []
        for s in range(2):
            raw = torch.from_numpy(data.read_frame(os.path.join(str(tmp_path), lines[s].split(" ")[4 + j]))).to(DEV)
            assert raw.shape[0] == gt_sizes[s][j]
            per_seq.append(float(emd.EMD(outs[0][j][s:s + 1].permute(0, 2, 1).contiguous(), raw[None].permute(0, 2, 1).contiguous())))
        want = float(np.mean(per_seq))
        assert abs(res["emd"][j] - want) <= 1e-6 * abs(want), (j, res["emd"][j], want)
    assert data.evaluate(lambda a, b: outs[0], loader, device=DEV, raw_gt=True)["emd"] is None   # the recorded frames again
