"""-m "not gpu": the float64 gradients of the set-abstraction layer (tests/group_mlp_grad_reference.py) against torch autograd over the
layer's composition, the properties of its test data that the GPU test relies on (clear channels, half-active ReLU layers, five
mutants outside the bound), and the host side of the backward: supported shapes, image and workspace sizes, ABI table, the
differentiable fold."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from mocopci_amd import _lib, ops
from tests import group_mlp_grad_reference as ggr
from tests import group_mlp_reference as gr

C_CAP = 2.0 ** -13   # the loosest constant any backward of this project carries: test_group_mlp_grad_gpu.py may not exceed it
B, M, N = 3, 37, 500


def case(c, nsample, widths, b=B, m=M, **kw):
    return dict(b=b, n=N, m=m, c=c, nsample=nsample, widths=widths, **kw)


def case_id(k):
    extra = "".join(f"-{n}={k[n]}" for n in ("pool", "c2", "use_xyz") if n in k)
    return f"c{k['c']}-ns{k['nsample']}-{'x'.join(map(str, k['widths']))}{extra}" + ("" if (k["b"], k["m"]) == (B, M) else f"-{k['b']}x{k['m']}")


CASES = [
    *[case(4, ns, [32, 32, 64]) for ns in (8, 12, 16, 32, 64)],              # group widths 8, 16, 32; a partial group; two tiles
    case(0, 16, [32]),                                                      # coordinates only, one layer
    case(64, 16, [64, 64, 128]), case(64, 16, [64, 64, 128], use_xyz=False),
    case(128, 8, [128, 128, 256]), case(128, 64, [128, 128, 256]),
    case(4, 16, [256]), case(80, 24, [32, 128]),
    case(4, 12, [32, 32, 64], pool="mean"), case(64, 64, [64, 64, 128], pool="mean"), case(128, 32, [128, 128, 256], pool="mean"),
    case(64, 16, [64, 64], c2=64), case(64, 64, [32, 32, 64], c2=64, pool="mean"),   # FlowEmbedding form: row_bias
]
TWO_SLOTS = [k for k in CASES if k["nsample"] == 64 and k.get("pool", "max") == "max"]        # every point sits in two slots
PARTIAL = [k for k in CASES if k["nsample"] == 12]                                            # 12 slots in a group of 16
# (B, M) = (1, 3): one tile with dead groups; whole tiles that fill the eight waves of one workgroup exactly
SMALL = [case(4, 8, [32, 32, 64], 1, 3), case(4, 8, [32, 32, 64], 2, 16), case(128, 32, [128, 128, 256], 1, 3, pool="mean"),
         case(128, 32, [128, 128, 256], 1, 8, pool="mean", seed=6)]   # seed 5 leaves one of the eight centres with a hidden unit on the kink


# the smallest B * M above the persistent grid's 256 workgroups x 8 waves (one centre per unit at nsample = 32): a partial second trip
PERSISTENT = [case(4, 32, [32, 32, 64], 3, 700)]


def ux(k):
    return k.get("use_xyz", True)


@pytest.mark.parametrize("case_", [CASES[2], CASES[7], CASES[15]], ids=case_id)
def test_reference_agrees_with_autograd_over_the_composition(case_):
    """F.max_pool2d's semantics: in these three cases slots tie only where they repeat a point (asserted), and there the lowest slot
    takes the gradient on both sides.  row_bias enters the composition as the centre's part of the first layer's input."""
    prep = ggr.prepare(case_)
    d = prep.data
    l64 = [t.double().clone().requires_grad_(True) for t in prep.leaves]
    t = dict(zip(prep.names, l64))
    weights = [(t[f"w{l + 1}"], t[f"b{l + 1}"]) for l in range(len(d["weights"]))]
    bi = torch.arange(B)[:, None, None]
    j = d["idx"].long()
    parts = ([t["xyz"][bi, j] - t["new_xyz"][:, :, None]] if d["use_xyz"] else []) + ([t["features"][bi, j]] if "features" in t else [])
    h = torch.cat(parts, -1).permute(0, 3, 1, 2)
    for l, (w, bias) in enumerate(weights):
        h = F.conv2d(h, w[:, :, None, None], bias)
        if l == 0 and "row_bias" in t:
            h = h + t["row_bias"].permute(0, 2, 1)[..., None]
        h = torch.relu(h)
    assert d["pool"] == "max"
    out = F.max_pool2d(h, kernel_size=[1, h.size(3)]).squeeze(-1).transpose(1, 2)
    want = torch.autograd.grad(out.reshape(-1, out.shape[-1]), l64, prep.g)
    for name, a, b in zip(prep.names, ggr.gradients(prep, torch.arange(B * M)), want):
        assert (a - b).abs().max().item() <= 1e-10 * max(1.0, b.abs().max().item()), name
    # the composition of group_mlp_reference (amax) gives the same value
    if "row_bias" not in t:
        with torch.no_grad():
            comp = gr.composition(d["xyz"].double(), d["new_xyz"].double(), None if d["features"] is None else d["features"].double(), d["idx"],
                                  [(w.double(), b.double()) for w, b in d["weights"]], use_xyz=d["use_xyz"], pool="max")
        assert (comp - out).abs().max().item() <= 1e-10


@pytest.mark.parametrize("case_", CASES + SMALL + PERSISTENT, ids=case_id)
def test_cases_keep_their_channels_clear_and_their_relus_half_active(case_):
    prep = ggr.prepare(case_)
    kept = prep.clear.double().mean().item()
    print(f"CLEAR {case_id(case_)} kept={kept:.3f} active={' '.join(f'{a:.3f}' for a in prep.active)} pooled<=0 {prep.dead:.3f}")
    assert kept > 0.9
    assert all(0.25 < a < 0.75 for a in prep.active), prep.active


def test_masked_winners_and_repeated_points_are_exercised():
    dead = [ggr.prepare(k).dead for k in CASES if k.get("pool", "max") == "max"]
    assert min(dead) > 0.0, "every max-pool case has pooled entries whose winner the ReLU mask removes"
    for k in TWO_SLOTS:
        idx = ggr.grad_inputs(k)["idx"]
        assert all(len(set(r.tolist())) <= 32 for r in idx.view(-1, 64)), "every point of a two-tile group sits in two slots"


def test_cases_reach_every_instantiation():
    """group_mlp_grad_kernel has one register class; its two instantiations are the two sides of the staging predicate."""
    inst = lambda k: ops.group_mlp_grad_weights_in_lds(k["c"], k["widths"], ux(k))
    assert {inst(k) for k in CASES} == {True, False}
    assert {inst(k) for k in SMALL} == {True, False}


@pytest.mark.parametrize("case_", CASES, ids=case_id)
def test_mutants_lie_outside_the_bound_at_its_cap(case_):
    """(a) all masks 1, (d) the last clear centre dropped, (e) the last clear centre counted twice -- on every case; (b) the maximum's
    gradient sent to every slot that attains it -- where every point sits in two slots; (c) the padding columns of a partial group
    counted -- nsample = 12 in a group of 16.  Each moves the layer's largest weight gradient by more than C_CAP x its largest entry;
    (a) also moves the first per-point gradient (grad_features, or grad_xyz without features) by more than that."""
    prep = ggr.prepare(case_)
    exact = ggr.gradients(prep)
    last = ggr.clear_centres(prep)[-1:]
    one = ggr.gradients(prep, last)
    lw = prep.largest_weight()
    mutants = {"all-masks": ggr.gradients(prep, masks_one=True), "dropped": [a - b for a, b in zip(exact, one)],
               "twice": [a + b for a, b in zip(exact, one)]}
    if case_ in TWO_SLOTS:
        mutants["every-tied-slot"] = ggr.gradients(prep, ties="all")
    if case_ in PARTIAL:
        mutants["padding-counted"] = ggr.gradients(prep, pad=4)
    for name, m in mutants.items():
        r = ggr.ratio(m[lw], exact[lw], C_CAP)
        print(f"MUTANT {case_id(case_)} {name} {prep.names[lw]} ratio={r:.1f}")
        assert r > 1.0, (name, r)
    r = ggr.ratio(mutants["all-masks"][0], exact[0], C_CAP)
    assert r > 1.0, (f"all-masks on grad_{prep.names[0]}", r)


def test_partial_and_two_slot_cases_exist():
    assert len(TWO_SLOTS) >= 2 and {k.get("pool", "max") for k in PARTIAL} == {"max", "mean"}


def test_supported_shapes_image_sizes_and_abi():
    shapes = [(c, w, ns, u) for c in (0, 4, 6, 64, 80, 128, 132) for w in ([32], [256], [48], [32, 128], [256, 32], [128, 128, 256], [32, 32, 32, 32])
              for ns in (0, 1, 12, 64, 65) for u in (True, False)]
    for c, w, ns, u in shapes:   # the supported set is the forward's: nothing was narrowed
        assert ops.group_mlp_grad_supported(c, w, ns, u) == ops.group_mlp_supported(c, w, ns, u), (c, w, ns, u)
    piece = 3 * 64 * 16
    assert ops.group_mlp_grad_image_bytes(4, [32]) == 2 * 1 * 1 * piece
    assert ops.group_mlp_grad_image_bytes(64, [64, 32]) == (2 * 1 * 2 + 2 * 2 * 3) * piece
    assert ops.group_mlp_grad_image_bytes(64, [64, 32], use_xyz=False) == (2 * 1 * 2 + 2 * 2 * 2) * piece
    assert ops.group_mlp_grad_weights_in_lds(4, [32, 32, 64]) and not ops.group_mlp_grad_weights_in_lds(128, [128, 128, 256])
    assert all(isinstance(v, int) and ops.group_mlp_grad_supported(k[1], k[2], k[0]) for k, v in ops.GROUP_MLP_GRAD_FUSED_CLASSES.items())
    assert not ops.group_mlp_grad_routes_fused(8, [32, 48], 16, 1 << 30), "a class without a measured row keeps the composition"
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mocopci_hip.h")).read()
    for name, nargs in (("mcp_group_mlp_grad_packed_floats", 4), ("mcp_group_mlp_grad_pack", 8), ("mcp_group_mlp_grad_workspace_bytes", 7),
                        ("mcp_group_mlp_grad", 29)):
        assert re.search(r"\b" + name + r"\(", header), name
        assert len(_lib.SIGNATURES[name]) == nargs
    assert _lib._RESTYPES["mcp_group_mlp_grad_workspace_bytes"] is ctypes.c_size_t
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    for k in CASES:
        wd = k["widths"]
        got = lib.mcp_group_mlp_grad_packed_floats(k["c"], int(ux(k)), len(wd), w(*wd))
        assert got == ops.group_mlp_grad_packed_floats(k["c"], wd, ux(k)) > 0, case_id(k)
        assert got == lib.mcp_group_mlp_packed_floats(k["c"], len(wd), w(*wd)) + ops.group_mlp_grad_image_bytes(k["c"], wd, ux(k)) // 4
    # unsupported shapes: size 0 from both queries
    assert lib.mcp_group_mlp_grad_packed_floats(6, 1, 1, w(32)) == 0 and lib.mcp_group_mlp_grad_packed_floats(0, 0, 1, w(32)) == 0
    assert lib.mcp_group_mlp_grad_packed_floats(4, 1, 2, w(256, 32)) == 0
    assert lib.mcp_group_mlp_grad_workspace_bytes(3, 37, 6, 16, 1, 1, w(32)) == 0 and lib.mcp_group_mlp_grad_workspace_bytes(3, 37, 4, 65, 1, 1, w(32)) == 0
    assert lib.mcp_group_mlp_grad_workspace_bytes(0, 37, 4, 16, 1, 1, w(32)) == 0
    # per pair: x (c + 3 in whole quads), h1, h2, gz1, gz2, gz3, dx (c + 3)
    pairs = 3 * 37 * 12
    assert lib.mcp_group_mlp_grad_workspace_bytes(3, 37, 4, 12, 1, 3, w(32, 32, 64)) >= 4 * pairs * (8 + 32 + 32 + 32 + 32 + 64 + 4 + 3)
    assert lib.mcp_group_mlp_grad_workspace_bytes(3, 37, 4, 12, 1, 3, w(32, 32, 64)) < 4 * pairs * (8 + 32 + 32 + 32 + 32 + 64 + 4 + 3) + (1 << 20)


def test_differentiable_fold_carries_the_gradient_to_the_module_parameters():
    from mocopci_amd.pointnet2_modules import PointnetSAModuleMSG
    m = PointnetSAModuleMSG(npoint=4, radii=[0.5], nsamples=[8], mlps=[[4, 32, 32]], bn=True).eval()
    assert m.grad_route == "measured" and m.route == "measured"
    convs, bns = m._layers(0)
    folded = [ops.fold_conv_bn_grad(c, b) for c, b in zip(convs, bns)]
    assert [tuple(w.shape) for w, _ in folded] == [(32, 7), (32, 32)]
    loss = sum((w * w).sum() + b.sum() for w, b in folded)
    grads = torch.autograd.grad(loss, list(m.parameters()))
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)
    for (w, b), c, bn in zip(folded, convs, bns):
        w0, b0 = ops.fold_conv_bn(c, bn)
        assert torch.equal(w.detach(), w0) and torch.equal(b.detach(), b0)
    # the route predicate: measured table empty -> composition; "always" -> fused in eval(), never under a training-mode BatchNorm
    assert not m.fused_scale_grad(0, 4, 1 << 20)
    m.grad_route = "always"
    assert m.fused_scale_grad(0, 4, 8) and not m.train().fused_scale_grad(0, 4, 8)
    nobn = PointnetSAModuleMSG(npoint=4, radii=[0.5], nsamples=[8], mlps=[[4, 32, 32]], bn=False).train()
    nobn.grad_route = "always"
    assert nobn.fused_scale_grad(0, 4, 8) and not nobn.fused_scale_grad(0, 6, 8), "bn=False is eligible in train(); an unsupported shape is not"
