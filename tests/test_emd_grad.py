"""EMD backward (emd_cuda.matchcost_backward, models/EMD/emd.py:15-21) and the explicit-match emd_cuda API.

Float64 references are formed here from a match array (the HIP approxmatch_forward or the oracle's), with the match held
constant as the reference's matchcostgrad1 / matchcostgrad2 do:
    grad1[k] = 2 g sum_l match[l][k] (x1_k - x2_l),   grad2[l] = 2 g sum_k match[l][k] (x2_l - x1_k)."""
import sys

import pytest
import torch

from mocopci_amd import _lib

P1 = [[1.7, -0.1, 0.1], [0.1, 1.2, 0.3]]   # models/EMD/test_emd_loss.py:7-10
P2 = [[0.3, 1.8, 0.2], [1.2, -0.2, 0.3]]
SHAPES = ((2, 512, 512), (2, 1000, 500), (2, 300, 900), (1, 777, 1025), (2, 2048, 2048), (1, 4096, 4096))
DEV = "cuda:0"


def grads_from_match(g, x1, x2, match):
    """float64 gradients of cost = sum match * |x2 - x1|^2 at a fixed match (B,M,N)."""
    g, x1, x2, match = g.double(), x1.double(), x2.double(), match.double()
    g1 = x1 * match.sum(1).unsqueeze(-1) - match.transpose(1, 2) @ x2
    g2 = x2 * match.sum(2).unsqueeze(-1) - match @ x1
    return 2 * g.view(-1, 1, 1) * g1, 2 * g.view(-1, 1, 1) * g2


def clouds(b, n, m, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 3, generator=gen) * 4, torch.rand(b, m, 3, generator=gen) * 4


def grad_cost_for(b):
    return torch.tensor([0.0, 1.7, -0.6, 2.5][:b] if b > 1 else [1.3])  # non-uniform, a zero entry when b > 1


def lean_grads(x, y, g):
    from mocopci_amd import emd
    x = x.to(DEV).requires_grad_(True)
    y = y.to(DEV).requires_grad_(True)
    cost = emd.earth_mover_distance(x, y, transpose=False)
    cost.backward(g.to(DEV))
    return cost.detach(), x.grad, y.grad


def assert_within(got, want, rel):
    got, want = got.double().cpu(), want.double().cpu()
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    assert err <= rel * scale, f"max error {err:.3e} > {rel} x max |grad| {scale:.3e}"


# ---------------- CPU ----------------

NEW_SYMBOLS = ("mcp_emd_levels_floats", "mcp_emd_keep", "mcp_emd_grad", "mcp_matchcost", "mcp_matchcost_grad")


def test_emd_backward_symbols_are_exported():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_emd_backward_argument_validation_needs_no_gpu():
    lib = _lib.load()
    assert lib.mcp_emd_keep(0, 16, 16, None, None, None, None, None, None) == 10001
    assert lib.mcp_emd_keep(1, 16, 16, None, None, None, None, None, None) == 10001
    assert lib.mcp_emd_grad(1, 0, 16, None, None, None, None, None, None, None) == 10001
    assert lib.mcp_emd_grad(1, 16, 16, None, None, None, None, None, None, None) == 10001
    assert lib.mcp_matchcost(1, 16, -1, None, None, None, None, None) == 10001
    assert lib.mcp_matchcost(1, 16, 16, None, None, None, None, None) == 10001
    assert lib.mcp_matchcost_grad(1, 16, 16, None, None, None, None, None, None, None) == 10001


def test_emd_levels_floats_is_the_documented_size():
    lib = _lib.load()
    assert lib.mcp_emd_levels_floats(8, 8192, 8192) == 8 * 10 * (8192 + 8192)
    assert lib.mcp_emd_levels_floats(2, 1000, 500) == 2 * 10 * 1500
    assert lib.mcp_emd_levels_floats(1, 777, 1025) == 10 * (777 + 1025)
    assert lib.mcp_emd_levels_floats(0, 8, 8) == 0


def test_emd_cuda_module_has_the_reference_names():
    from mocopci_amd import emd, emd_cuda
    for name in ("approxmatch_forward", "matchcost_forward", "matchcost_backward"):   # models/EMD/cuda/emd.cpp:24-26
        assert getattr(emd_cuda, name) is getattr(emd, name)


def test_compat_install_registers_emd_cuda():
    from mocopci_amd import compat, emd_cuda
    saved = {k: sys.modules.get(k) for k in ("emd_cuda", "pointnet2_cuda", "pointnet2.pointnet2_utils",
                                             "models.pointnet2.pointnet2_utils", "models.common")}
    try:
        compat.install()
        assert sys.modules["emd_cuda"] is emd_cuda
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_emd_api_rejects_non_float32_or_host_tensors():
    from mocopci_amd import emd
    x, y = clouds(1, 8, 8, 0)
    with pytest.raises(RuntimeError, match="float32 CUDA"):
        emd.matchcost_forward(x, y, torch.zeros(1, 8, 8))
    with pytest.raises(RuntimeError, match="float32 CUDA"):
        emd.matchcost_backward(torch.ones(1), x.double(), y.double(), torch.zeros(1, 8, 8))
    with pytest.raises(RuntimeError, match="float32 CUDA"):
        emd.EarthMoverDistanceFunction.apply(x.requires_grad_(True), y)


# ---------------- GPU ----------------

@pytest.mark.gpu
def test_reference_known_answer_gradients():
    """models/EMD/test_emd_loss.py: loss d0/2 + 2 d1 + d2/3 on the 2-point clouds; p1.grad / p2.grad equal float64 autograd of
    the closed-form gt_dist (the optimal matching p1[0]<->p2[1], p1[1]<->p2[0])."""
    from mocopci_amd import emd
    q1 = torch.tensor([P1], dtype=torch.float64).repeat(3, 1, 1).requires_grad_(True)
    q2 = torch.tensor([P2], dtype=torch.float64).repeat(3, 1, 1).requires_grad_(True)
    pair = [((q1[i, 0] - q2[i, 1]) ** 2).sum() + ((q1[i, 1] - q2[i, 0]) ** 2).sum() for i in range(3)]
    (pair[0] / 2 + pair[1] * 2 + pair[2] / 3).backward()
    p1 = torch.tensor([P1]).repeat(3, 1, 1).to(DEV).requires_grad_(True)
    p2 = torch.tensor([P2]).repeat(3, 1, 1).to(DEV).requires_grad_(True)
    d = emd.earth_mover_distance(p1, p2, transpose=False)
    assert d.grad_fn is not None
    loss = d[0] / 2 + d[1] * 2 + d[2] / 3
    loss.backward()
    torch.testing.assert_close(p1.grad.cpu().double(), q1.grad, rtol=0, atol=1e-5)
    torch.testing.assert_close(p2.grad.cpu().double(), q2.grad, rtol=0, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("b,n,m", SHAPES)
def test_lean_backward_matches_float64_on_the_device_match(b, n, m):
    from mocopci_amd import emd
    x, y = clouds(b, n, m, 11 + n + m)
    g = grad_cost_for(b)
    _, g1, g2 = lean_grads(x, y, g)
    match = emd.approxmatch_forward(x.to(DEV), y.to(DEV)).cpu()
    w1, w2 = grads_from_match(g, x, y, match)
    assert_within(g1, w1, 1e-5)
    assert_within(g2, w2, 1e-5)
    if b > 1:
        assert float(g1[0].abs().max()) == 0.0 and float(g2[0].abs().max()) == 0.0   # grad_cost[0] = 0


@pytest.mark.gpu
@pytest.mark.parametrize("b,n,m", ((2, 512, 512), (2, 1000, 500), (2, 300, 900), (1, 2048, 2048)))
def test_lean_backward_against_the_oracle_match(b, n, m):
    """The oracle's match and the device's differ by up to 2e-3 per entry (test_emd.py), so the gradients agree only to that
    order: relative L2 error of each gradient below 2e-3."""
    from oracle import pointset as orc
    x, y = clouds(b, n, m, 5 + n)
    g = torch.tensor([1.0, 0.5][:b])
    _, g1, g2 = lean_grads(x, y, g)
    _, omatch = orc.earth_mover_distance(x, y, return_match=True)
    w1, w2 = grads_from_match(g, x, y, omatch)
    e1 = float((g1.cpu().double() - w1).norm() / w1.norm())
    e2 = float((g2.cpu().double() - w2).norm() / w2.norm())
    print(f"\nEMD gradient vs the oracle's match, {(b, n, m)}: relative L2 error grad1 {e1:.2e}, grad2 {e2:.2e}")
    assert e1 < 2e-3 and e2 < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("b,n,m", SHAPES + ((1, 8192, 8192),))
def test_explicit_match_path_agrees_with_the_lean_path(b, n, m):
    from mocopci_amd import emd_cuda, emd
    x, y = clouds(b, n, m, 23 + n)
    g = grad_cost_for(b)
    cost, g1, g2 = lean_grads(x, y, g)
    xd, yd = x.to(DEV), y.to(DEV)
    match = emd_cuda.approxmatch_forward(xd, yd)
    c = emd_cuda.matchcost_forward(xd, yd, match)
    d2 = ((yd.double().unsqueeze(2) - xd.double().unsqueeze(1)) ** 2).sum(-1)            # (B,M,N)
    exact = (match.double() * d2).sum((1, 2))
    del d2
    torch.testing.assert_close(c.double(), exact, rtol=1e-6, atol=0)
    # the fused forward sums its n*m products per level in float32: within the metric's 1e-5 of the same total
    fused = emd.earth_mover_distance(xd, yd, transpose=False)
    torch.testing.assert_close(fused, c, rtol=1e-5, atol=0)
    assert torch.equal(cost, fused)                                                     # level-keeping forward: same bits
    print(f"\nEMD cost {(b, n, m)}: matchcost vs float64 {float(((c.double() - exact) / exact).abs().max()):.1e}, "
          f"fused forward vs float64 {float(((fused.double() - exact) / exact).abs().max()):.1e} relative")
    e1, e2 = emd_cuda.matchcost_backward(g.to(DEV), xd, yd, match)
    assert e1.shape == (b, n, 3) and e2.shape == (b, m, 3)
    assert_within(e1, g1, 1e-5)
    assert_within(e2, g2, 1e-5)


@pytest.mark.gpu
def test_memory_determinism_and_no_grad_path_at_baseline_size():
    """B = 8, N = M = 8192: forward + backward need the kept levels (5.2 MB), not a (B,M,N) match (2 GiB)."""
    from mocopci_amd import emd
    B, N = 8, 8192
    gen = torch.Generator().manual_seed(31)
    x = (torch.rand(B, N, 3, generator=gen) * torch.tensor([80.0, 80.0, 6.0])).to(DEV)
    y = (x + 0.3 * torch.randn(B, N, 3, generator=gen).to(DEV)).contiguous()
    g = torch.linspace(0.5, 2.0, B, device=DEV)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        plain = emd.earth_mover_distance(x, y, transpose=False)
    torch.cuda.synchronize()
    levels_bytes = 4 * _lib.load().mcp_emd_levels_floats(B, N, N)
    assert torch.cuda.max_memory_allocated() - base < levels_bytes          # no level buffer without a gradient
    del plain
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    base = torch.cuda.memory_allocated()
    cost = emd.earth_mover_distance(xr, yr, transpose=False)
    ga = torch.autograd.grad(cost, (xr, yr), g, retain_graph=True)
    gb = torch.autograd.grad(cost, (xr, yr), g)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 * 2 ** 20
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])         # fixed summation order
    with torch.no_grad():
        plain = emd.earth_mover_distance(x, y, transpose=False)
    assert torch.equal(plain, cost.detach())                                # the level-keeping forward: same cost bits
    assert bool(torch.isfinite(ga[0]).all()) and float(ga[0].abs().max()) > 0


@pytest.mark.gpu
def test_wrappers_layout_scale_and_single_input_gradient():
    from mocopci_amd import emd
    gen = torch.Generator().manual_seed(41)
    pc1 = (torch.rand(2, 3, 700, generator=gen) * 4).to(DEV)
    pc2 = (torch.rand(2, 3, 700, generator=gen) * 4).to(DEV)
    g = torch.tensor([0.7, 1.9], device=DEV)
    # transpose=True: (B,3,N) in, gradient in the same layout
    a, b = pc1.clone().requires_grad_(True), pc2.clone().requires_grad_(True)
    emd.earth_mover_distance(a, b, transpose=True).backward(g)
    _, w1, w2 = lean_grads(pc1.transpose(1, 2).contiguous().cpu(), pc2.transpose(1, 2).contiguous().cpu(), g.cpu())
    assert a.grad.shape == pc1.shape
    assert torch.equal(a.grad, w1.transpose(1, 2)) and torch.equal(b.grad, w2.transpose(1, 2))
    # EMD(): mean over the batch / N
    a, b = pc1.clone().requires_grad_(True), pc2.clone().requires_grad_(True)
    emd.EMD(a, b).backward()
    _, w1, w2 = lean_grads(pc1.transpose(1, 2).contiguous().cpu(), pc2.transpose(1, 2).contiguous().cpu(), torch.ones(2))
    torch.testing.assert_close(a.grad, w1.transpose(1, 2) / (2 * 700), rtol=1e-6, atol=1e-12)
    torch.testing.assert_close(b.grad, w2.transpose(1, 2) / (2 * 700), rtol=1e-6, atol=1e-12)
    # a gradient on one input only: None for the other
    x = pc1.transpose(1, 2).contiguous().requires_grad_(True)
    y = pc2.transpose(1, 2).contiguous()
    cost = emd.earth_mover_distance(x, y, transpose=False)
    cost.backward(g)
    assert y.grad is None and x.grad is not None
    torch.testing.assert_close(x.grad, lean_grads(x.detach().cpu(), y.cpu(), g.cpu())[1], rtol=0, atol=0)
    y2 = pc2.transpose(1, 2).contiguous().requires_grad_(True)
    c2 = emd.EarthMoverDistanceFunction.apply(x.detach(), y2)
    gx, gy = c2.grad_fn.apply(g)                                      # the function's own backward outputs (c2 kept alive)
    assert gx is None and gy is not None and gy.shape == y2.shape
