"""-m gpu: the fusion layer on batch statistics (csrc/fusion_bn.hip: three statistics passes, the layer, four backward passes; 13
kernels) against the float64 reference of tests/fusion_bn_reference.py at the edges of its persistent loops.  One call launches under
TWO grid caps -- the statistics passes, the layer, B1 and B4 on min(ceil(total / 4), 2 CUs) workgroups, B2 and B3 on
min(ceil(total / 4), CUs) -- and every pass deals points through mcp_units_by_xcd, so above a cap with a ragged eighth some workgroups
receive nothing and must still write a zero partial row, which fusion_bn_stats_kernel / sum_partials_kernel add over all workgroups.
tests/kernel_variants.py names the cases (BN_CASES) and mirrors the launches; test_kernel_variants_cpu.py checks that the cases reach
every emitted kernel and every such edge, test_fusion_bn_reference_cpu.py that the reference is right and that the cases have the dead
neighbours, zero variances and far channels they claim.  The caps are multiples of the CU count; the mirror is checked at 256, so the
tests skip on any other device.

Every case runs the public path (be.fusion_bn with requires_grad leaves) with every buffer that the forward and the backward allocate
filled with NaN beforehand (poisoned_buffers): out, the bn vector, the variances and all 14 gradients are finite; a second forward +
backward and the list as one (B, N, 64) tensor give identical bits; be.fusion_bn_forward without the kept scores gives the same out /
bn / var; mcp_fusion_bn_backward (which re-evaluates the layer) gives the same row_c, row_dy, row_a, d_p1, d_nb, d_w, d_aff as
mcp_fusion_bn_backward_saved, with poisoned scratch and workspace; every kept channel is in 0..127 and a dead neighbour (no positive
layer-3 channel: score floored at 0, gated by `score > 0`) has row_dy exactly 0; rows of p2 that no list gathers and the conv-bias
gradients (the unit's header promises a memset) are exactly zero.  Then, against float64,
    ratio = max|hip - exact| / (c * scale) <= 1
with one constant c per group: out (scale max|exact|), mean (per channel, |mean| + sigma), rstd (what the layer consumes, well
defined at zero variance: relative), the variance output (per channel, var + (mean - bias)^2 + eps: the size of the S2 / R the
kernel subtracts from, so the `far` case needs no looser constant), and the gradients in three groups -- per point (p1, p2), conv
weights, affine -- each on max|exact|.  Gradients that are zero in exact arithmetic (one point: all but p2's) are held to the
absolute floor 2e-5.  The `far` case checks statistics and out only.

The bound matters: with contribution(p) the float64 gradient of the upstream gradient masked to point p, the mutants
exact - contribution(p) (a dropped point) and exact + contribution(p) (a point counted twice) must both lie outside the bound on w3
for p the last clear point, and on w3 and w2 (w1) for the last clear point of a last round of the narrow (wide) role where it has
more than one round; and the layer-3 statistics recomputed in float64 without the last point's 64 rows must lie outside the bound on
the mean or on rstd.

c: the smallest power of two that is at least twice the worst max|hip - exact| / scale measured on the MI355X over the cases (in
brackets, with the case that set it; profiles/fusion_bn_variants_accuracy.txt holds every RATIO line, beside the same figure for the
float32 unfused composition on the device, a yardstick that nothing is asserted on)."""
import ctypes

import pytest
import torch

from mocopci_amd import _lib, ops
from tests import fused_reference as fr
from tests import fusion_bn_reference as br
from tests import kernel_variants as kv
from tests.test_fused_grad_variants_gpu import poisoned_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2e-5
# group: c   [worst max|hip - exact| / scale: case]
C = {
    "out": 2.0 ** -15,       # [8.45e-6: far]
    "mean": 2.0 ** -12,      # [6.49e-5: one-point -- see below]
    "rstd": 2.0 ** -15,      # [9.94e-6: far]
    "var": 2.0 ** -14,       # [1.55e-5: far]
    "point": 2.0 ** -18,     # [1.54e-6: grid-75, p1]
    "weight": 2.0 ** -14,    # [2.44e-5: cap-rounds, w3]
    "affine": 2.0 ** -13,    # [4.34e-5: cap-rounds, gamma2]
}
# mean: 2^-12 = 2.4e-4 is above the 1e-4 that tests/test_grad_gpu.py allows the statistics, so it is a finding; the cause is the case's
# data, seen in float64 alone, and the constant is adopted.  With one point every variance is zero, so the scale |mean| + sigma is
# |mean|, and layer 3's channel 34 has the mean 5.8e-4 = its conv bias -0.130 + W h 0.130: a few fp32 roundings of 0.13 (1.5e-8 each)
# are 6.5e-5 of that mean.  The float32 unfused composition is at 5.0e-5 on the same channel.  Without this case the worst mean figure
# is 2.09e-5 (far; the float32 composition: 2.3e-5).
# far: until the statistics passes took their shift from the data (fusion_bn.hip, fusion_bn_fwd_kernel) this case stood at out 7.5e-5,
# mean 1.5e-4, rstd 2.6e-4, var 2.1e-4 -- ten times the float32 composition, from the cancellation of S2 / R - (S1 / R)^2 around the conv
# bias in layer 2 -- which put rstd at 2^-10 and mean at 2^-11, and neither bound then saw the last point dropped from the layer-3
# statistics of 1025, 2049 or 3093 points (ratios 0.13 to 0.56).
OFF4 = (0, 256, 512)     # the bn vector: per layer mean | rstd | gamma | beta
OFFV = (0, 64, 128)      # the variance output


def statistics(bn, var):
    """(mean, rstd, var) per layer of the kernels' bn vector and variance output, float64 on the CPU."""
    bn, var = bn.double().cpu(), var.double().cpu()
    return ([bn[o:o + c] for o, c in zip(OFF4, br.WIDTHS)], [bn[o + c:o + 2 * c] for o, c in zip(OFF4, br.WIDTHS)],
            [var[o:o + c] for o, c in zip(OFFV, br.WIDTHS)])


def statistic_errors(mean, rstd, var, ev, biases):
    """Worst error over channels and layers, in units of each quantity's scale: (mean, rstd, var)."""
    em = er = evar = 0.0
    for i in range(3):
        m, v = ev.mean[i], ev.var[i]
        em = max(em, float(((mean[i] - m).abs() / (m.abs() + v.sqrt())).max()))
        exact_rstd = torch.rsqrt(v + br.EPS)
        er = max(er, float(((rstd[i] - exact_rstd).abs() / exact_rstd).max()))
        evar = max(evar, float(((var[i] - v).abs() / (v + (m - biases[i]).square() + br.EPS)).max()))
    return em, er, evar


def last_round_point(role, clear):
    """The last clear point that the mirror places in a last round of `role`, when the role has more than one round."""
    rounds = max(len(wg) for wg in role["dealt"])
    if rounds < 2:
        return None
    mine = {u for wg in role["dealt"] if len(wg) == rounds for u in wg[-1]} & set(clear.tolist())
    return max(mine) if mine else None


@pytest.mark.parametrize("case", kv.BN_CASES, ids=kv.bn_case_id)
def test_fusion_on_batch_statistics_matches_float64(case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the grids are capped at multiples of the CU count and the cases are chosen for 256 CUs; this device has {cus}")
    cid = kv.bn_case_id(case)
    prep = br.prepare(case)
    lib, be = _lib.load(), ops.backend()
    B, N, total, rows = case["b"], case["n"], prep.total, prep.total * 64
    backward = not case.get("forward_only")
    if case.get("far"):
        assert float(br.far_ratio(prep).min()) > 30      # the case is what it claims to be
    halves = tuple(t.to(DEV) for t in prep.idx)
    one_list = torch.cat(halves, -1).contiguous()
    g = prep.g.float().to(DEV).view(B, N, 3)
    names = prep.names

    def public(idx):
        leaves = [t.to(DEV).requires_grad_(True) for t in prep.leaves]
        out, bn, var = be.fusion_bn(leaves[0], leaves[1], idx, leaves[2:8], leaves[8:], br.EPS)
        return [out.detach(), bn, var] + (list(torch.autograd.grad(out, leaves, g)) if backward else [])
    labels = ["out", "bn", "var"] + (names if backward else [])
    with poisoned_buffers():
        hip, again, as_one_list = public(halves), public(halves), public(one_list)
    for name, a, a2, a3 in zip(labels, hip, again, as_one_list):
        assert torch.isfinite(a).all(), f"{name}: not finite"
        assert torch.equal(a, a2), f"{name}: a second forward + backward gives other bits"
        assert torch.equal(a, a3), f"{name}: the list as two halves and as one list give other bits"
    out, bn, var = hip[:3]
    grads = dict(zip(names, hip[3:]))

    # ---- every entry point agrees bit for bit ----
    dl = [t.to(DEV) for t in prep.leaves]
    with poisoned_buffers():
        saved = (torch.empty(rows, dtype=torch.int32, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV))
        plain = be.fusion_bn_forward(dl[0], dl[1], halves, dl[2:8], dl[8:], br.EPS)
        keeping = be.fusion_bn_forward(dl[0], dl[1], halves, dl[2:8], dl[8:], br.EPS, saved=saved)
    for name, a, b, c in zip(("out", "bn", "var"), plain, keeping, (out, bn, var)):
        assert torch.equal(a, c) and torch.equal(b, c), f"{name}: the forward without the kept scores gives other bits"
    assert int(saved[0].min()) >= 0 and int(saved[0].max()) < 128 and bool((saved[2] >= 0).all())
    if backward:
        st = torch.cuda.current_stream().cuda_stream
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        need = lib.mcp_fusion_bn_grad_workspace_bytes(B, N)

        def entry(name, extra):
            with poisoned_buffers():
                scr = dict(row_c=torch.empty(rows, dtype=torch.int32, device=DEV), row_dy=torch.empty(rows, device=DEV), row_a=torch.empty(rows, device=DEV),
                           dy2=torch.empty(rows, 64, device=DEV), dy1=torch.empty(rows, 64, device=DEV), d_p1=torch.empty_like(dl[0]),
                           d_nb=torch.empty(B, N, 64, 3, device=DEV), d_w=torch.empty(lib.mcp_fusion_grad_floats(), device=DEV),
                           d_aff=torch.empty(512, device=DEV), ws=torch.empty(need, dtype=torch.uint8, device=DEV))
            rc = getattr(lib, name)(B, N, 64, P(dl[0]), P(dl[1]), P(halves[0]), P(halves[1]), *[P(t) for t in dl[2:8]], P(bn), P(g), *extra,
                                    P(scr["row_c"]), P(scr["row_dy"]), P(scr["row_a"]), P(scr["dy2"]), P(scr["dy1"]), P(scr["d_p1"]), P(scr["d_nb"]),
                                    P(scr["d_w"]), P(scr["d_aff"]), P(scr["ws"]), need, st)
            assert rc == 0, name
            torch.cuda.synchronize()
            return scr
        fresh = entry("mcp_fusion_bn_backward", ())
        kept = entry("mcp_fusion_bn_backward_saved", tuple(P(t) for t in saved))
        for k in ("row_c", "row_dy", "row_a", "d_p1", "d_nb", "d_w", "d_aff"):
            assert torch.equal(fresh[k], kept[k]), f"{k}: the backward that re-evaluates the layer and the one that reads the kept scores give other bits"
        assert torch.equal(kept["d_p1"], grads["p1"]) and torch.equal(kept["d_aff"][:64], grads["gamma1"])
        # ---- kept rows ----
        assert int(fresh["row_c"].min()) >= 0 and int(fresh["row_c"].max()) < 128
        dead_dy = fresh["row_dy"].cpu().view(total, 64)[prep.dead]
        assert not dead_dy.any(), f"{int((dead_dy != 0).sum())} of {int(prep.dead.sum())} dead neighbours have a gradient"
        # ---- exact zeros ----
        whole = fr._whole(prep.idx).long()
        used = torch.zeros(B, N, dtype=torch.bool)
        used[torch.arange(B).view(-1, 1, 1).expand_as(whole), whole] = True
        assert not grads["p2"].cpu()[~used].any(), "p2: a row that nothing gathers has a gradient"
        for name in br.CONV_BIASES:
            assert not grads[name].any(), f"{name}: a conv bias in front of a batch-statistics BatchNorm has a gradient"

    # ---- the float32 unfused composition on the device: the yardstick ----
    tl = [t.to(DEV).requires_grad_(True) for t in prep.leaves]
    tev = br.layer(tl, one_list.long())
    twin = dict(zip(names, torch.autograd.grad(tev.out, tl, g.view(-1, 3)))) if backward else {}
    tev.pre, tev.z3 = None, None

    failures = []
    print()

    def held(label, group, err, err_twin, scale_text=""):
        print(f"RATIO {cid} {label} [{group}]{scale_text} err/scale={err:.3e} kernel={err / C[group]:.3f} twin={err_twin / C[group]:.3f}")
        if not err <= C[group]:
            failures.append(f"{label}: error {err:.2e} of its scale, allowed {C[group]:.2e}")

    # ---- accuracy against float64 ----
    ev = prep.ev
    scale = float(ev.out.abs().max())
    held("out", "out", float((out.double().cpu().view(-1, 3) - ev.out).abs().max()) / scale,
         float((tev.out.detach().double().cpu() - ev.out).abs().max()) / scale, f" max|exact|={scale:.3e}")
    biases = [prep.leaves[k].double() for k in (3, 5, 7)]
    mean, rstd, hvar = statistics(bn, var)
    errs = statistic_errors(mean, rstd, hvar, ev, biases)
    tmean, tvar = [m.detach().double().cpu() for m in tev.mean], [v.detach().double().cpu() for v in tev.var]
    terrs = statistic_errors(tmean, [torch.rsqrt(v + br.EPS) for v in tvar], tvar, ev, biases)
    for label, e, t in zip(("mean", "rstd", "var"), errs, terrs):
        held(label, label, e, t)
    if backward:
        exact = dict(zip(names, br.gradients(prep)))
        for name in names:
            if name in br.CONV_BIASES:
                continue
            a, t32, e = grads[name].double().cpu(), twin[name].double().cpu(), exact[name]
            scale = float(e.abs().max())
            if br.exact_zero(case, name):
                print(f"RATIO {cid} {name} [{br.group(name)}, zero in exact arithmetic] max|exact|={scale:.1e} max|hip|={float(a.abs().max()):.3e} max|twin|={float(t32.abs().max()):.3e}")
                assert scale <= 1e-12
                if not float(a.abs().max()) <= FLOOR:
                    failures.append(f"{name}: {float(a.abs().max()):.2e} where exact arithmetic gives zero")
                continue
            held(name, br.group(name), float((a - e).abs().max()) / scale, float((t32 - e).abs().max()) / scale, f" max|exact|={scale:.3e}")

        # ---- the mutants: a dropped and a doubled point must lie outside the bound ----
        if not br.exact_zero(case, "w3"):
            clear, grid = prep.clear_points(), kv.bn_launch_grid(cus=256, **case)
            picks = {int(clear[-1]): [("last", "w3")]}
            for role, mats in (("narrow", ("w3", "w2")), ("wide", ("w1",))):
                p = last_round_point(grid[role], clear)
                if p is not None:
                    picks.setdefault(p, []).extend((f"last round of {role}", m) for m in mats)
            for p, wanted in picks.items():
                contrib = dict(zip(names, br.gradients(prep, sel=[p])))
                for tag, wname in wanted:
                    a, e = grads[wname].double().cpu(), exact[wname]
                    bound = C["weight"] * float(e.abs().max())
                    dropped, doubled = float((a - (e - contrib[wname])).abs().max()) / bound, float((a - (e + contrib[wname])).abs().max()) / bound
                    print(f"RATIO {cid} {wname} mutant point {p} ({tag}): dropped={dropped:.2f} doubled={doubled:.2f}")
                    if not (dropped > 1.0 and doubled > 1.0):
                        failures.append(f"{wname}: the bound does not see point {p} ({tag}) dropped ({dropped:.2f}) or counted twice ({doubled:.2f})")
    if total > 1:   # the layer-3 statistics without the last point's 64 rows
        m, v = br.stats3_without(prep, total - 1)
        mut_rstd = torch.rsqrt(v + br.EPS)
        on_mean = float(((mean[2] - m).abs() / (m.abs() + v.sqrt())).max()) / C["mean"]
        on_rstd = float(((rstd[2] - mut_rstd).abs() / mut_rstd).max()) / C["rstd"]
        print(f"RATIO {cid} layer-3 statistics mutant without point {total - 1}: mean={on_mean:.2f} rstd={on_rstd:.2f}")
        if not (on_mean > 1.0 or on_rstd > 1.0):
            failures.append(f"the bounds do not see the last point dropped from the layer-3 statistics (mean {on_mean:.2f}, rstd {on_rstd:.2f})")
    prep.release()
    assert not failures, "; ".join(failures)
