"""-m "not gpu": the float64 statement of the feature-propagation layer (tests/fp_mlp_reference.py) against the layer in fp32 torch
within C * 2^-24 * bound, C being the constant the GPU test holds the kernel to, and, on the same inputs, the two-term mutant of the
bf16 split outside that bound.  Also the Python mirrors of the kernel's shape rules, the route predicate, and the parameter names of
PointnetFPModule against the names recorded from the reference class.  (The module's composition under lengths needs three_nn, which
runs on the GPU only: those checks are in test_fp_mlp_gpu.py.)"""
import json
import os

import pytest
import torch

from mocopci_amd import ops
from tests import fp_mlp_reference as fpr
from tests import fused_reference as fr

C_FP_MLP = 2.0   # as tests/test_fp_mlp_gpu.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    dict(b=2, n=45, m=21, c2=4, c1=0, widths=[32]),
    dict(b=2, n=45, m=21, c2=20, c1=3, widths=[64, 32]),
    dict(b=2, n=45, m=21, c2=128, c1=4, widths=[128, 128, 128]),
    dict(b=2, n=45, m=21, c2=256, c1=64, widths=[256, 128]),
]


def ratios(case, rule, short=False):
    from tests.test_kernel_variants_gpu import two_term
    d = fpr.fp_mlp_inputs(case)
    dist = d["dist"]
    if short:   # what three_nn gives over two, and over no, known points
        dist = dist.clone()
        dist[0, :, 2] = float("inf")
        dist[1] = float("inf")
    args = (d["known_feats"], d["skip"], d["idx"], dist, d["weights"])
    exact, bound = fpr.fp_mlp_reference(*args, rule=rule, w3=d["w3"])
    assert exact.dtype == bound.dtype == torch.float64 and torch.isfinite(exact).all() and torch.isfinite(bound).all()
    assert 0.1 < (exact > 0).double().mean().item(), "the last ReLU cuts nearly everything"
    tol = (C_FP_MLP * fr.U * bound).clamp_min(1e-300)
    comp = fpr.composition(*args, rule=rule, w3=d["w3"]).reshape(exact.shape).double()
    assert torch.isfinite(comp).all()
    mutant = fpr.fp_mlp_reference(*args, rule=rule, w3=d["w3"], cut=two_term)[0]
    assert (fr.U * bound).max().item() <= 2.0 ** -10 * max(1.0, exact.abs().max().item())   # a bound, not a licence
    return ((comp - exact).abs() / tol).max().item(), ((mutant - exact).abs() / tol).max().item()


@pytest.mark.parametrize("rule", ["pointnet2", "flownet3d", "given"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"c{c['c2']}+{c['c1']}-{'x'.join(map(str, c['widths']))}")
def test_composition_inside_and_two_term_mutant_outside_the_bound(case, rule):
    comp, mutant = ratios(case, rule)
    print(f"RATIO composition={comp:.3f} two_term={mutant:.2f}")
    assert comp <= 1.0, f"fp32 composition and float64 statement differ by {comp:.2f} x the bound"
    assert mutant > 1.0, f"the bound does not tell a two-term split from three terms ({mutant:.2f})"


@pytest.mark.parametrize("rule", ["pointnet2", "flownet3d"])
def test_infinite_distances_weigh_nothing(rule):
    """A slot at +inf has weight exactly 0; three of them give the MLP of [0 | skip]; nothing is NaN."""
    case = CASES[1]
    comp, _ = ratios(case, rule, short=True)
    assert comp <= 1.0
    d = fpr.fp_mlp_inputs(case)
    dist = torch.full_like(d["dist"], float("inf"))
    w, used = fpr.blend_weights(dist, rule)
    assert (w == 0).all() and not used.any()
    poisoned = torch.full_like(d["known_feats"], float("nan"))
    exact, bound = fpr.fp_mlp_reference(poisoned, d["skip"], d["idx"], dist, d["weights"], rule=rule)
    x = torch.cat([torch.zeros(*d["skip"].shape[:2], case["c2"]), d["skip"]], -1).double().reshape(-1, case["c2"] + case["c1"])
    for wl, bias in d["weights"]:
        x = torch.relu(x @ wl.double().T + bias.double())
    assert torch.allclose(exact, x, rtol=1e-12, atol=1e-12) and torch.isfinite(bound).all()
    two = d["dist"].clone()
    two[..., 2] = float("inf")
    w, used = fpr.blend_weights(two, rule)
    assert (w[..., 2] == 0).all() and not used[..., 2].any() and torch.allclose(w.sum(-1), torch.ones(()))


def test_coincident_point_reaches_the_floors():
    d = fpr.fp_mlp_inputs(CASES[0])
    assert (d["dist"][:, fpr.COINCIDENT, 0] == 0).all()
    for rule in ("pointnet2", "flownet3d"):
        w, _ = fpr.blend_weights(d["dist"], rule)
        assert torch.isfinite(w).all() and (w[:, fpr.COINCIDENT, 0] > 0.999).all()


def test_shape_rules_mirror_the_kernel():
    inside = [(4, 0, [32]), (512, 256, [256, 256]), (256, 3, [256, 256]), (128, 4, [128, 128, 128]), (64, 64, [32, 256]), (256, 512, [64]),
              (20, 1, [256, 32, 64])]
    outside = [(6, 0, [32]), (0, 4, [32]), (516, 0, [32]), (4, 513, [32]), (512, 260, [32]), (4, 0, [48]), (4, 0, [512]), (4, 0, []),
               (4, 0, [32, 32, 32, 32]), (4, -1, [32])]
    for c2, c1, widths in inside:
        assert ops.fp_mlp_supported(c2, c1, widths), (c2, c1, widths)
    for c2, c1, widths in outside:
        assert not ops.fp_mlp_supported(c2, c1, widths), (c2, c1, widths)
    # weight pieces: 32-channel tiles x k-steps x 3 KB per layer; the interpolated and the skip part round up on their own
    assert ops.fp_mlp_image_bytes(4, 0, [32]) == 3072
    assert ops.fp_mlp_image_bytes(20, 3, [64, 32]) == (2 * 3 + 1 * 4) * 3072
    assert ops.fp_mlp_image_bytes(512, 256, [256, 256]) == (8 * 48 + 8 * 16) * 3072
    assert ops.fp_mlp_weights_in_lds(64, 3, [64, 64]) and ops.fp_mlp_weights_in_lds(4, 0, [256])
    assert not ops.fp_mlp_weights_in_lds(64, 64, [32, 256]) and not ops.fp_mlp_weights_in_lds(256, 3, [256, 256])
    assert [ops.fp_mlp_tmax(w) for w in ([32], [64, 32], [32, 128], [256, 64])] == [2, 2, 4, 8]


def test_route_predicate_is_a_pure_function_of_shapes(monkeypatch):
    assert ops.fp_mlp_class(256, 3, [256, 256]) == (256, 3, (256, 256))
    assert not ops.fp_mlp_routes_fused(252, 3, [256, 256], 1 << 20), "a class without a measured row keeps the composition"
    monkeypatch.setattr(ops, "FP_MLP_FUSED_CLASSES", {(256, 3, (256, 256)): 4096})
    assert ops.fp_mlp_routes_fused(256, 3, [256, 256], 4096) and ops.fp_mlp_routes_fused(256, 3, (256, 256), 1 << 20)
    assert not ops.fp_mlp_routes_fused(256, 3, [256, 256], 4095) and not ops.fp_mlp_routes_fused(256, 4, [256, 256], 1 << 20)
    from mocopci_amd.pointnet2_modules import PointnetFPModule
    m = PointnetFPModule(mlp=[259, 256, 256]).eval()
    assert m.route == "measured" and m.weighting == "pointnet2"
    assert m.fused(256, 3, 4096) and not m.fused(256, 3, 100) and not m.fused(255, 4, 4096)
    m.route = "never"
    assert not m.fused(256, 3, 4096)
    m.route = "always"
    assert m.fused(256, 3, 1) and not m.train().fused(256, 3, 1)
    assert not PointnetFPModule(mlp=[259, 48]).eval().fused(256, 3, 1 << 20)


@pytest.mark.parametrize("bn", [True, False])
def test_module_parameter_names_are_the_recorded_list(bn):
    from mocopci_amd.pointnet2_modules import PointnetFPModule
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "pointnet2_fp_state_keys.json")))["bn" if bn else "plain"]
    mlp = [259, 256, 256]
    m = PointnetFPModule(mlp=mlp, bn=bn)
    assert mlp == [259, 256, 256], "the caller's list is left alone"
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == spec
    m.load_state_dict({k: torch.zeros(s) if "num_batches" not in k else torch.zeros(s, dtype=torch.long) for k, s in spec.items()}, strict=True)


def test_broadcast_of_a_global_feature_is_the_composition():
    """known=None: known_feats (B, C2, 1) is expanded over the unknown points; no search, no kernel, on any device."""
    from mocopci_amd.pointnet2_modules import PointnetFPModule
    g = torch.Generator().manual_seed(3)
    m = PointnetFPModule(mlp=[8 + 3, 32], bn=False).eval()
    m.route = "always"
    feats, skip = torch.randn(2, 8, 1, generator=g), torch.randn(2, 3, 10, generator=g)
    with torch.no_grad():
        out = m(torch.zeros(2, 10, 3), None, skip, feats)
    conv = m.mlp.layer0.conv
    want = torch.relu(torch.nn.functional.conv2d(torch.cat([feats.expand(2, 8, 10), skip], 1).unsqueeze(-1), conv.weight, conv.bias)).squeeze(-1)
    assert out.shape == (2, 32, 10) and torch.allclose(out, want, rtol=1e-5, atol=1e-6)
