"""-m "not gpu": the float64 gradients of the feature-propagation layer (tests/fp_mlp_grad_reference.py) against torch autograd over
the layer's composition, the properties of its test data that the GPU test relies on (clear rows, half-active ReLU layers, three
mutants outside the bound), and the host side of the backward: supported shapes, image sizes, ABI table, the differentiable fold."""
import ctypes
import os
import re

import pytest
import torch

from mocopci_amd import _lib, ops
from tests import fp_mlp_grad_reference as fgr
from tests import fp_mlp_reference as fpr

C_CAP = 2.0 ** -13   # the loosest constant any backward of this project carries: test_fp_mlp_grad_gpu.py may not exceed it
B, N, M = 3, 70, 37


def case(c2, c1, widths, b=B, n=N):
    return dict(b=b, n=n, m=M, c2=c2, c1=c1, widths=widths)


def case_id(k):
    return f"c{k['c2']}+{k['c1']}-{'x'.join(map(str, k['widths']))}" + ("" if (k["b"], k["n"]) == (B, N) else f"-{k['b']}x{k['n']}")


# the forward tests' twelve shapes (tests/test_fp_mlp_gpu.py: CASES), restated so that this file needs no GPU module
CASES = [
    case(4, 0, [32]), case(20, 0, [64, 32]), case(64, 3, [64, 64]), case(128, 4, [128, 128, 128]), case(256, 3, [256, 256]),
    case(256, 64, [256, 128]), case(256, 128, [256, 256]), case(512, 256, [256, 256]), case(64, 64, [32, 256]),
    case(256, 128, [64]), case(4, 0, [128]), case(4, 0, [256]),
]
OTHER_RULES = [CASES[1], CASES[2], CASES[3], CASES[7], CASES[11]]
SMALL = [case(20, 0, [64, 32], b, n) for b, n in ((1, 5), (2, 64))] + [case(256, 3, [256, 256], b, n) for b, n in ((1, 5), (2, 64))]


@pytest.mark.parametrize("rule", fpr.RULES)
@pytest.mark.parametrize("case_", [CASES[1], CASES[2], CASES[3]], ids=case_id)
def test_reference_agrees_with_autograd_over_the_composition(case_, rule):
    prep = fgr.prepare(case_, rule)
    d = prep.data
    l64 = [t.double().clone().requires_grad_(True) for t in prep.leaves]
    skip = l64[1] if prep.has_skip else None
    wb = l64[prep.point_leaves():]
    dist = None if d["dist"] is None else d["dist"].double()
    out = fpr.composition(l64[0], skip, d["idx"], dist, list(zip(wb[0::2], wb[1::2])), rule=rule, w3=d["w3"].double())
    want = torch.autograd.grad(out.reshape(-1, out.shape[-1]), l64, prep.g)
    for name, a, b in zip(prep.names, fgr.gradients(prep), want):
        assert (a - b).abs().max().item() <= 1e-10 * max(1.0, b.abs().max().item()), name


@pytest.mark.parametrize("case_", CASES + SMALL, ids=case_id)
def test_cases_keep_their_rows_clear_and_their_relus_half_active(case_):
    for rule in fpr.RULES if case_ in OTHER_RULES else ("pointnet2",):
        prep = fgr.prepare(case_, rule)
        kept = prep.clear.double().mean().item()
        print(f"CLEAR {case_id(case_)}-{rule} kept={kept:.3f} active={' '.join(f'{a:.3f}' for a in prep.active)}")
        assert kept > 0.9
        assert all(0.25 < a < 0.75 for a in prep.active), prep.active


def test_cases_reach_every_instantiation():
    """(accumulator tiles per bank, both halves of the image whole in LDS): the six instantiations of fp_mlp_grad_kernel."""
    inst = lambda k: (ops.fp_mlp_tmax(k["widths"]), ops.fp_mlp_grad_weights_in_lds(k["c2"], k["c1"], k["widths"]))
    assert {inst(k) for k in CASES} == {(t, s) for t in (2, 4, 8) for s in (True, False)}
    assert {inst(k) for k in SMALL} == {(2, True), (8, False)}


@pytest.mark.parametrize("case_", CASES, ids=case_id)
def test_mutants_lie_outside_the_bound_at_its_cap(case_):
    """All masks set to 1, the last clear row dropped, the last clear row counted twice: each moves the layer's largest weight gradient
    by more than C_CAP x its largest entry; the first also moves grad_known_feats by more than that."""
    prep = fgr.prepare(case_, "pointnet2")
    exact = fgr.gradients(prep)
    last = prep.clear.nonzero().flatten()[-1:]
    one = fgr.gradients(prep, last)
    lw = prep.largest_weight()
    mutants = {"all-masks": fgr.gradients(prep, masks_one=True), "dropped": [a - b for a, b in zip(exact, one)],
               "twice": [a + b for a, b in zip(exact, one)]}
    for name, m in mutants.items():
        r = fgr.ratio(m[lw], exact[lw], C_CAP)
        print(f"MUTANT {case_id(case_)} {name} {prep.names[lw]} ratio={r:.1f}")
        assert r > 1.0, (name, r)
    r = fgr.ratio(mutants["all-masks"][0], exact[0], C_CAP)
    assert r > 1.0, ("all-masks on grad_known_feats", r)


def test_supported_shapes_image_sizes_and_abi():
    for c2, c1, widths in ((4, 0, [32]), (512, 256, [256, 256]), (256, 3, [256, 256]), (256, 128, [256, 256]), (128, 4, [128, 128, 128]), (20, 0, [64, 32])):
        assert ops.fp_mlp_grad_supported(c2, c1, widths), (c2, c1, widths)
    for c2, c1, widths in ((6, 0, [32]), (4, 0, [48]), (4, 0, [32, 32, 32, 32]), (512, 260, [32]), (0, 4, [32]), (516, 0, [32]), (4, 0, [512])):
        assert not ops.fp_mlp_grad_supported(c2, c1, widths), (c2, c1, widths)
    slab = 3 * 64 * 16
    assert ops.fp_mlp_grad_image_bytes(4, 0, [32]) == 2 * 1 * 1 * slab
    assert ops.fp_mlp_grad_image_bytes(20, 3, [64, 32]) == (2 * 1 * 2 + 2 * 2 * 1) * slab
    assert ops.fp_mlp_grad_image_bytes(256, 3, [256, 256]) == (2 * 8 * 8 + 2 * 8 * 9) * slab
    assert ops.fp_mlp_grad_packed_floats(20, 3, [64, 32]) == (2 * 3 + 1 * 4) * 768 + 96 + 8 * 768
    assert ops.fp_mlp_grad_weights_in_lds(20, 3, [64, 32]) and not ops.fp_mlp_grad_weights_in_lds(256, 3, [256, 256])
    assert all(isinstance(v, int) and ops.fp_mlp_grad_supported(*k) for k, v in ops.FP_MLP_GRAD_FUSED_CLASSES.items())
    assert not ops.fp_mlp_grad_routes_fused(252, 3, [256, 256], 1 << 30), "a class without a measured row keeps the composition"
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mocopci_hip.h")).read()
    for name, nargs in (("mcp_fp_mlp_grad_packed_floats", 4), ("mcp_fp_mlp_grad_pack", 8), ("mcp_fp_mlp_grad_workspace_bytes", 6), ("mcp_fp_mlp_grad", 26)):
        assert re.search(r"\b" + name + r"\(", header), name
        assert len(_lib.SIGNATURES[name]) == nargs
    assert _lib._RESTYPES["mcp_fp_mlp_grad_workspace_bytes"] is ctypes.c_size_t
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    assert lib.mcp_fp_mlp_grad_packed_floats(20, 3, 2, w(64, 32)) == ops.fp_mlp_grad_packed_floats(20, 3, [64, 32])
    assert lib.mcp_fp_mlp_grad_packed_floats(512, 256, 2, w(256, 256)) == ops.fp_mlp_grad_packed_floats(512, 256, [256, 256])
    assert lib.mcp_fp_mlp_grad_packed_floats(6, 0, 1, w(32)) == 0 and lib.mcp_fp_mlp_grad_workspace_bytes(3, 70, 6, 0, 1, w(32)) == 0
    assert lib.mcp_fp_mlp_grad_workspace_bytes(3, 70, 20, 3, 2, w(64, 32)) >= 4 * 210 * (23 + 64 + 64 + 32 + 20 + 3)
    assert lib.mcp_fp_mlp_grad_workspace_bytes(0, 70, 20, 3, 2, w(64, 32)) == 0


def test_differentiable_fold_has_the_bits_of_the_fold_and_reaches_the_parameters():
    g = torch.Generator().manual_seed(3)
    conv, bn = torch.nn.Conv2d(7, 5, 1), torch.nn.BatchNorm2d(5)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(5, generator=g))
        bn.running_var.copy_(torch.rand(5, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(5, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(5, generator=g))
    for norm in (bn, None):
        w, b = ops.fold_conv_bn_grad(conv, norm)
        w0, b0 = ops.fold_conv_bn(conv, norm)
        assert torch.equal(w.detach(), w0) and torch.equal(b.detach(), b0) and w.requires_grad and b.requires_grad
        gw, gb = torch.randn(5, 7, generator=g), torch.randn(5, generator=g)
        params = [conv.weight, conv.bias] + ([bn.weight, bn.bias] if norm is not None else [])
        got = torch.autograd.grad((w * gw).sum() + (b * gb).sum(), params, retain_graph=True)
        x = torch.randn(4, 7, 3, 1, generator=g)            # the same parameters through the modules themselves, in eval mode
        bn.eval()
        y = conv(x) if norm is None else bn(conv(x))
        wx = torch.einsum("oc,bcnk->bonk", w.detach(), x) + b.detach().view(1, -1, 1, 1)
        assert torch.allclose(y, wx, rtol=1e-5, atol=1e-5)
        gy = torch.randn(y.shape, generator=g)
        want = torch.autograd.grad(y, params, gy)
        # d<y, gy>/dparam through the fold: gw = sum gy x^T, gb = sum gy
        via = torch.autograd.grad((w * torch.einsum("bonk,bcnk->oc", gy, x)).sum() + (b * gy.sum((0, 2, 3))).sum(), params)
        for a, c in zip(via, want):
            assert torch.allclose(a, c, rtol=1e-4, atol=1e-5)
        assert all(t is not None and torch.isfinite(t).all() for t in got)
        bn.train()
