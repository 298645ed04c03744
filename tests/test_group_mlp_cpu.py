"""-m "not gpu": the float64 statement of the set-abstraction layer (tests/group_mlp_reference.py) against the layer as the modules
compose it in fp32 torch -- neighbour lists from the oracle's ball query or from the clusters, grouped tensor, 1x1 convolutions, pool --
within C * 2^-24 * bound, C being the constant the GPU test holds the kernel to; and, on the same inputs, the two-term mutant of the
bf16 split outside that bound: the inputs make the bound discriminating before a GPU is involved.  Also the Python mirrors of the
kernel's shape rules and the parameter names of the modules against the committed list."""
import json
import os

import pytest
import torch

from mocopci_amd import ops
from tests import fused_reference as fr
from tests import group_mlp_reference as gr

C_GROUP_MLP = 2.0   # as tests/test_group_mlp_gpu.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    dict(b=2, n=200, m=19, c=4, nsample=16, widths=[32, 32, 64]),
    dict(b=2, n=200, m=19, c=0, nsample=12, widths=[32]),
    dict(b=2, n=200, m=19, c=64, nsample=24, widths=[64, 64, 128], pool="mean"),
    dict(b=2, n=200, m=19, c=64, nsample=8, widths=[128, 128, 256], use_xyz=False),
    dict(b=2, n=200, m=19, c=64, c2=64, nsample=16, widths=[64, 64], extent=True),
]


def ratios(case, idx=None):
    from tests.test_kernel_variants_gpu import two_term
    xyz, new_xyz, feats, cidx, centre, ws = gr.group_mlp_inputs(case)
    idx = cidx if idx is None else idx(xyz, new_xyz)
    kw = dict(use_xyz=case.get("use_xyz", True), pool=case.get("pool", "max"), centre=centre)
    exact, bound = gr.group_mlp_reference(xyz, new_xyz, feats, idx, ws, **kw)
    assert exact.dtype == bound.dtype == torch.float64 and torch.isfinite(exact).all() and torch.isfinite(bound).all()
    assert 0.1 < (exact > 0).double().mean().item(), "the last ReLU cuts nearly everything"
    tol = (C_GROUP_MLP * fr.U * bound).clamp_min(1e-300)
    comp = gr.composition(xyz, new_xyz, feats, idx, ws, **kw).reshape(exact.shape).double()
    mutant = gr.group_mlp_reference(xyz, new_xyz, feats, idx, ws, cut=two_term, **kw)[0]
    # the bound is a bound, not a licence: nowhere more than 2^-10 of the output's scale
    assert (fr.U * bound).max().item() <= 2.0 ** -10 * max(1.0, exact.abs().max().item())
    return ((comp - exact).abs() / tol).max().item(), ((mutant - exact).abs() / tol).max().item()


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"c{c['c']}-ns{c['nsample']}-{'x'.join(map(str, c['widths']))}")
def test_composition_inside_and_two_term_mutant_outside_the_bound(case):
    comp, mutant = ratios(case)
    print(f"RATIO composition={comp:.3f} two_term={mutant:.2f}")
    assert comp <= 1.0, f"fp32 composition and float64 statement differ by {comp:.2f} x the bound"
    assert mutant > 1.0, f"the bound does not tell a two-term split from three terms ({mutant:.2f})"


def test_ball_query_lists_of_the_oracle():
    """Neighbour lists as QueryAndGroup makes them (first hits in index order, padded with the first hit), on the oracle's ball query."""
    from oracle import pointset as orc
    case = dict(b=2, n=200, m=19, c=4, nsample=16, widths=[32, 32, 64])
    comp, mutant = ratios(case, idx=lambda xyz, new_xyz: orc.ball_query(0.7, 16, xyz, new_xyz))
    assert comp <= 1.0 and mutant > 1.0, (comp, mutant)


def test_shape_rules_mirror_the_kernel():
    assert ops.group_mlp_supported(4, [32, 32, 64], 16) and ops.group_mlp_supported(0, [32], 64) and ops.group_mlp_supported(128, [128, 128, 256], 1)
    for c, widths, ns, use_xyz in ((0, [32], 16, False), (6, [32], 16, True), (132, [32], 16, True), (4, [256, 64], 16, True), (4, [48], 16, True),
                                   (4, [32, 32, 32, 32], 16, True), (4, [32], 65, True), (4, [32], 0, True), (4, [512], 16, True)):
        assert not ops.group_mlp_supported(c, widths, ns, use_xyz), (c, widths, ns, use_xyz)
    # weight pieces: 32-channel tiles x k-steps x 3 KB per layer
    assert ops.group_mlp_image_bytes(4, [32, 32, 64]) == (1 * 1 + 1 * 2 + 2 * 2) * 3072
    assert ops.group_mlp_image_bytes(0, [32]) == 0 and ops.group_mlp_image_bytes(80, [32]) == 8 * 3072
    assert ops.group_mlp_weights_in_lds(4, [32, 32, 64]) and ops.group_mlp_weights_in_lds(0, [32])
    assert not ops.group_mlp_weights_in_lds(64, [64, 64, 128]) and not ops.group_mlp_weights_in_lds(128, [128, 128, 256])
    assert ops.group_mlp_class(4, [32, 32, 64], 12) == (16, 4, (32, 32, 64))


def test_fold_conv_bn_is_the_eval_batchnorm():
    g = torch.Generator().manual_seed(5)
    conv, bn = torch.nn.Conv2d(7, 32, 1, bias=False), torch.nn.BatchNorm2d(32, eps=1e-3)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(32, generator=g) + 0.5); bn.bias.copy_(torch.randn(32, generator=g))
        bn.running_mean.copy_(torch.randn(32, generator=g)); bn.running_var.copy_(torch.rand(32, generator=g) + 0.2)
    bn.eval()
    x = torch.randn(2, 7, 5, 3, generator=g)
    w, b = ops.fold_conv_bn(conv, bn)
    want = bn(conv(x))
    got = torch.nn.functional.conv2d(x, w[:, :, None, None], b)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)


def test_module_parameter_names_are_the_committed_list():
    from mocopci_amd.pointnet2_modules import PointnetSAModule, PointnetSAModuleMSG
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "pointnet2_sa_state_keys.json")))
    mlps = [[4, 32, 32, 64], [4, 64, 64, 128]]
    m = PointnetSAModuleMSG(npoint=128, radii=[0.7, 1.5], nsamples=[12, 24], mlps=mlps)
    assert mlps == [[4, 32, 32, 64], [4, 64, 64, 128]], "the caller's lists are left alone"
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == spec
    m.load_state_dict({k: torch.zeros(s) if "num_batches" not in k else torch.zeros(s, dtype=torch.long) for k, s in spec.items()}, strict=True)
    plain = PointnetSAModule(mlp=[4, 32], npoint=8, radius=1.0, nsample=8, bn=False)
    assert sorted(plain.state_dict()) == ["mlps.0.layer0.conv.bias", "mlps.0.layer0.conv.weight"]
    assert tuple(plain.state_dict()["mlps.0.layer0.conv.weight"].shape) == (32, 7, 1, 1)
