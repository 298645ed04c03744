"""-m gpu: the hand-written backward kernels of the fused point layers (csrc/fusion_grad.hip, cross_grad.hip, cross256_grad.hip,
pointconv_grad.hip, ptblock_grad.hip) against the float64 gradients of tests/fused_grad_reference.py, at the edges of their persistent
loops: launches with fewer points than a workgroup has waves, workgroups that receive nothing and must still write a zero partial
vector, the first total above the grid cap, ragged per-XCD eighths, the three roles of cross_grad_kernel<128> with their different
round counts, odd tails of the pair kernels, the three deals of the D = 256 plan.  tests/kernel_variants.py names the cases
(GRAD_CASES) and mirrors the launches; test_kernel_variants_cpu.py checks that the cases reach every emitted kernel and every such
edge, test_fused_grad_reference_cpu.py that the reference agrees with the unfused twins in float64 and that the clear rules keep the
upstream gradient.  The grid caps are the device's CU count; the mirror is checked at 256, so the tests skip on any other device.

Every case runs the public path (be.fusion_mlp, be.cross_layer, be.pointconv_agg, be.ptblock_layer) with requires_grad leaves:
gradients finite, with every buffer the backward allocates filled with NaN beforehand (poisoned_buffers: an unwritten partial vector or
output row cannot hide behind a fresh allocation's zeros); a second backward and the neighbour list in its other form (two halves / one list; fusion and cross) give identical
bits; rows of p2 / xyz2 / points2 / s_xyz / s_points / k / v that no list gathers get exactly zero; and for every gradient
    ratio = max|hip - exact| / (c * max|exact|) <= 1
with one constant c per kernel family and group -- per-point gradients (coordinates, features) and weight / bias gradients.
Gradients that are zero in exact arithmetic (fused_grad_reference.exact_zero says which and why) are held to the project's absolute
floor 2e-5 instead.  The bound matters: with contribution(p) the float64 weight gradient of the upstream gradient masked to point p,
the reference mutants exact - contribution(p) (a dropped point) and exact + contribution(p) (a point counted twice: what a dead wave
or an odd tail does when its zero upstream gradient is not zero) must both lie outside the bound (ratio > 1) on the layer's largest
weight matrix, for p the last clear point of the launch and, with more than one round, the last clear point of a last round.

c: the smallest power of two that is at least twice the worst max|hip - exact| / max|exact| measured on the MI355X over the family's
cases (in brackets, with the case and gradient that set it; profiles/fused_grad_accuracy.txt holds every RATIO line, beside the
same figure for the float32 unfused twin on the device, a yardstick that nothing is asserted on).  The bound in use before,
2e-4 max|grad| + 2e-5 (tests/test_grad_gpu.py), was never measured."""
import contextlib
import functools

import pytest
import torch

from mocopci_amd import grad, ops
from tests import fused_grad_reference as gr
from tests import kernel_variants as kv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2e-5
# family: (c of the per-point gradients, c of the weight / bias gradients)   [worst max|hip - exact| / max|exact|: case, gradient]
C = {
    "fusion": (2.0 ** -16, 2.0 ** -16),          # fusion_grad_kernel            [5.14e-6: grid-75, p1]  [6.83e-6: 5-points, w3]
    "cross": (2.0 ** -20, 2.0 ** -19),           # cross_grad_kernel<64 | 128>   [3.38e-7: <64> cap-4-rounds, points1]  [6.93e-7: <64> cap+1, bmlp]
    "cross256": (2.0 ** -19, 2.0 ** -18),        # cross256_grad_{z,w,dx}_kernel [5.71e-7: ragged-workgroup, points1]  [1.35e-6: cap+1, bmlp]
    "pointconv_agg": (2.0 ** -20, 2.0 ** -19),   # pointconv_agg_grad_kernel     [3.78e-7: 9-centres, s_xyz]  [6.41e-7: cap-3-rounds, b0]
    "ptblock": (2.0 ** -15, 2.0 ** -13),         # ptblock_grad_kernel           [9.75e-6: odd-B1, q]  [7.00e-5: odd-B1, wg2 -- see below]
}
# ptblock weights: the rule gives 2^-12 = 2.4e-4, above the 2e-4 in use before, so it is a finding and not adopted; the constant stays
# at 2^-13 = 1.2e-4, 1.74 x the worst figure.  The cause is the case's data, seen in float64 alone: odd-B1 has extent=True and 333 =
# 20 x 16 + 13 points, so the lists of the 13 points of the last, incomplete cluster wrap around into cluster 0, up to 43 units away
# where every other neighbour is within 5.  Their |attn| / 8 reaches 104 (10 in every other case) and |delta| 53 (5): a logit of 104
# carries an fp32 rounding of 8e-6, which exp() turns into a relative error of that size in the softmax weights and so in the gradients
# of fc_gamma, whose exact values (3.8) are no larger than elsewhere.  The float32 unfused twin is 1.5 x further from float64 on the same
# gradient (1.06e-4).  Without this case the worst ptblock weight figure is 1.31e-5 (xcd-ragged with logits of 80, wg2).
GATHERED = {"fusion": ["p2"], "cross": ["xyz2", "points2"], "pointconv_agg": ["s_xyz", "points"], "ptblock": ["k", "v"]}   # rows reached only through the list


def family(case):
    return "cross256" if case["op"] == "cross" and case["d"] == 256 else case["op"]


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(Prepared, float64 gradients) of a case, computed once."""
    case = next(c for c in kv.GRAD_CASES if kv.grad_case_id(c) == cid)
    prep = gr.prepare(case)
    return prep, gr.gradients(prep)


def forms(case, idx):
    """The neighbour list as the case's builder gives it, then in its other form where the entry point takes both."""
    if isinstance(idx, (tuple, list)):
        halves = tuple(t.to(DEV) for t in idx)
        return [halves, torch.cat(halves, -1).contiguous()]
    return [idx.to(DEV)]


def run(case, fn_of_be, leaves, idx, g):
    """Gradients w.r.t. fresh device leaves of <layer, g> through the public path (or the unfused twin)."""
    dl = [t.to(DEV).requires_grad_(True) for t in leaves]
    op = case["op"]
    if op == "fusion":
        out = fn_of_be["fusion"](dl[0], dl[1], idx, *dl[2:])
    elif op == "cross":
        out = fn_of_be["cross"](*dl[:4], idx, *dl[4:])
    elif op == "pointconv_agg":
        out = fn_of_be["pointconv_agg"](*dl[:3], idx, *dl[3:])
    elif case.get("packed"):   # q, k, v as slices of one (B, N, 192) leaf: dl = [xyz, qkv, weights...]
        out = fn_of_be["ptblock"](dl[0], dl[1][..., :64], dl[1][..., 64:128], dl[1][..., 128:], idx, dl[2:])
    else:
        out = fn_of_be["ptblock"](*dl[:4], idx, dl[4:])
    return list(torch.autograd.grad(out, dl, g.view(out.shape)))


@contextlib.contextmanager
def poisoned_buffers():
    """While active, torch.empty / torch.empty_like hand out device buffers of 0xFF bytes (NaN as float32): the backward's outputs and
    its workspace of per-workgroup partial vectors come from torch.empty, a fresh allocation usually reads as zeros, and so a partial
    row that an idle workgroup failed to write would otherwise go unnoticed in the sum over all rows."""
    real_empty, real_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_cuda and t.numel() and t.is_contiguous():
            t.view(torch.uint8).fill_(255)
        return t
    torch.empty, torch.empty_like = (lambda *a, **kw: poison(real_empty(*a, **kw))), (lambda *a, **kw: poison(real_like(*a, **kw)))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def hip_path(be):
    return {"fusion": be.fusion_mlp, "cross": be.cross_layer, "pointconv_agg": be.pointconv_agg, "ptblock": be.ptblock_layer}


def twin_path(be):
    G = be.group_rows
    return {"fusion": lambda *a: grad.fusion_twin(G, *a), "cross": lambda *a: grad.cross_twin(G, *a),
            "pointconv_agg": lambda *a: grad.pointconv_agg_twin(G, *a), "ptblock": lambda x, q, k, v, i, w: grad.ptblock_twin(G, x, q, k, v, i, *w)}


def last_round_points(case, total):
    """Points the mirror places in a last round of the role that sums the largest weight matrix, when it has more than one round."""
    role = kv.grad_launch_grid(cus=256, **case)[kv.grad_weight_role(case)]
    rounds = max(len(wg) for wg in role["dealt"])
    if rounds < 2:
        return []
    units = [u for wg in role["dealt"] if len(wg) == rounds for u in wg[-1]]
    pair = case["op"] in ("pointconv_agg", "ptblock")
    return sorted(p for u in units for p in ((2 * u, 2 * u + 1) if pair else (u,)) if p < total)


@pytest.mark.parametrize("case", kv.GRAD_CASES, ids=kv.grad_case_id)
def test_backward_variant_matches_float64(case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the backward grids are capped at the CU count and the cases are chosen for 256 CUs; this device has {cus}")
    cid = kv.grad_case_id(case)
    prep, exact = reference(cid)
    be = ops.backend()
    names, leaves, exact = list(prep.names), list(prep.leaves), list(exact)
    if case.get("packed"):
        names[1:4], leaves[1:4], exact[1:4] = ["qkv"], [torch.cat(leaves[1:4], -1)], [torch.cat(exact[1:4], -1)]
    g = prep.g.float().to(DEV)
    idx_forms = forms(case, prep.idx)

    with poisoned_buffers():
        hip = run(case, hip_path(be), leaves, idx_forms[0], g)
        again = run(case, hip_path(be), leaves, idx_forms[0], g)
    for name, a, a2 in zip(names, hip, again):
        assert torch.isfinite(a).all(), f"{name}: not finite"
        assert torch.equal(a, a2), f"{name}: a second backward gives other bits"
    for other in idx_forms[1:]:
        for name, a, a2 in zip(names, hip, run(case, hip_path(be), leaves, other, g)):
            assert torch.equal(a, a2), f"{name}: the list as two halves and as one list give other bits"
    twin = run(case, twin_path(be), leaves, idx_forms[0], g)

    # rows that no list gathers: exactly zero
    whole = gr.fr._whole(prep.idx).long()
    bi = torch.arange(whole.shape[0]).view(-1, 1, 1).expand_as(whole)
    for name in GATHERED[case["op"]]:
        src = hip[names.index("qkv")][..., 64 * (1 + ("k", "v").index(name)):][..., :64] if case.get("packed") else hip[names.index(name)]
        used = torch.zeros(src.shape[:2], dtype=torch.bool)
        used[bi, whole] = True
        assert not src.cpu()[~used].any(), f"{name}: a row that nothing gathers has a gradient"

    npoint = 2 if case.get("packed") else gr.POINT_LEAVES[case["op"]]
    failures = []
    for k, (name, a, t32, e) in enumerate(zip(names, hip, twin, exact)):
        a, t32 = a.double().cpu(), t32.double().cpu()
        group, c = ("point", C[family(case)][0]) if k < npoint else ("weight", C[family(case)][1])
        scale, err, err_twin = float(e.abs().max()), float((a - e).abs().max()), float((t32 - e).abs().max())
        if gr.exact_zero(case, name):
            print(f"RATIO {cid} {name} [{group}, zero in exact arithmetic] max|exact|={scale:.1e} max|hip|={float(a.abs().max()):.3e} max|twin|={float(t32.abs().max()):.3e}")
            assert scale <= 1e-12
            if not float(a.abs().max()) <= FLOOR:
                failures.append(f"{name}: {float(a.abs().max()):.2e} where exact arithmetic gives zero")
            continue
        print(f"RATIO {cid} {name} [{group}] max|exact|={scale:.3e} err/max={err / scale:.3e} kernel={err / (c * scale):.3f} twin={err_twin / (c * scale):.3f}")
        if not err <= c * scale:
            failures.append(f"{name}: max err {err:.2e} = {err / scale:.2e} of the gradient's scale {scale:.2e}, allowed {c:.2e}")

    # the mutants: a dropped and a doubled point must lie outside the bound on the largest weight matrix
    wname = gr.LARGEST_WEIGHT[case["op"]]
    wk = names.index(wname)
    if not gr.exact_zero(case, wname):
        clear = prep.clear_points()
        picks = {"last": int(clear[-1])}
        in_last = set(last_round_points(case, prep.total)) & set(clear.tolist())
        if in_last:
            picks["last-round"] = max(in_last)
        a, e = hip[wk].double().cpu(), exact[wk]
        bound = C[family(case)][1] * float(e.abs().max())
        for tag, p in picks.items():
            contrib = gr.gradients(prep, sel=[p])[prep.names.index(wname)]
            dropped, doubled = float((a - (e - contrib)).abs().max()) / bound, float((a - (e + contrib)).abs().max()) / bound
            print(f"RATIO {cid} {wname} mutant point {p} ({tag}): dropped={dropped:.2f} doubled={doubled:.2f}")
            if not (dropped > 1.0 and doubled > 1.0):
                failures.append(f"{wname}: the bound does not see point {p} ({tag}) dropped ({dropped:.2f}) or counted twice ({doubled:.2f})")
    assert not failures, "; ".join(failures)
