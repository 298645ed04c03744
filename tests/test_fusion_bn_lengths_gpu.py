"""-m gpu: the train-mode fusion layer with per-cloud lengths (csrc/fusion_bn_lengths.hip; mcp_fusion_bn_forward_lengths /
mcp_fusion_bn_backward_lengths, ops.HipBackend.fusion_bn(lengths=)) against the float64 reference of
tests/fusion_bn_lengths_reference.py, whose CASES name the edge each case reaches: one live point (m = 64), an empty element between
two live ones, no live point at all (m = 0), a padded tail inside a workgroup's deal, a padded FIRST point (the statistics' shift must
come from a live row), a padded total above the narrow grid cap (1024 points at 256 CUs, kernel_variants.bn_launch_grid) with the live
total below it, and padded and live totals above both caps (2048) with one nearly empty element.  The caps are multiples of the CU
count, so the two large cases skip on a device without 256 CUs, as test_fusion_bn_variants_gpu.py does.

Every case: padded rows of p1, p2 and of the upstream gradient are NaN, padded rows of the lists are out of range (-1 in the first half,
2^30 in the second), every buffer the calls allocate is NaN-filled beforehand (poisoned_buffers).  out, bn, var, count and the 14
gradients are finite; out and the gradients of p1 and p2 are exactly zero on padded rows; a second forward + backward gives identical
bits; other values in the padded rows change no bit; on the unpadded batch len = NULL (the C entry points) and len = (N, ..., N) give
the dense entry points' bits; count is the number of live points.  Against float64, ratio = max|hip - exact| / (c * scale) <= 1 with
the groups and scales of test_fusion_bn_variants_gpu.py.  The bound must bite: the layer-3 statistics in float64 without the last live
point's 64 rows, and with one padded point's rows counted in (finite garbage coordinates), lie outside the mean or the rstd bound, and
w3's gradient without the last clear live point's contribution lies outside the weight bound.

c: the smallest power of two that is at least twice the worst ratio measured on the MI355X over the cases (in brackets, with the case
that set it; profiles/fusion_bn_lengths_accuracy.txt holds every RATIO line beside the float32 torch formulation on the device, a
yardstick that nothing is asserted on).  No constant is larger than the dense test's for the same group."""
import ctypes

import pytest
import torch

from mocopci_amd import _lib, grad, ops
from tests import fused_reference as fr
from tests import fusion_bn_lengths_reference as lr
from tests import fusion_bn_reference as br
from tests.fusion_bn_lengths_reference import CASES, case_id
from tests.test_fused_grad_variants_gpu import poisoned_buffers
from tests.test_fusion_bn_variants_gpu import statistic_errors, statistics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2e-5
# group: c   [worst max|hip - exact| / scale: case]
C = {
    "out": 2.0 ** -20,       # [3.57e-7: over-both-caps]
    "mean": 2.0 ** -12,      # [7.45e-5: one-point -- the dense test's one-point case and its cause: every variance is zero, the scale is |mean| alone]
    "rstd": 2.0 ** -21,      # [1.58e-7: first-point-padded]
    "var": 2.0 ** -21,       # [2.06e-7: first-point-padded]
    "point": 2.0 ** -18,     # [1.31e-6: over-both-caps, p1]
    "weight": 2.0 ** -15,    # [1.34e-5: over-both-caps, w3]
    "affine": 2.0 ** -14,    # [1.83e-5: first-point-padded, beta3]
}
# out, rstd and var are far below the dense test's constants because that test's worst case for them is `far` (a layer-2 channel 77
# sigma from its bias), which has no counterpart here.  At the dense constant for rstd (2^-15) the bounds did not see the last of the
# 2103 live points of over-both-caps dropped from the layer-3 statistics (mean 0.11, rstd 0.60); at 2^-21 they do.
BIG = 1 << 30


def poisoned(prep, value=float("nan"), ia_pad=-1, ib_pad=BIG, g_pad=float("nan")):
    """(leaves, halves, g) on the device with the padded rows of p1, p2, the lists and the upstream gradient replaced."""
    leaves = [t.clone() for t in prep.leaves]
    for t in leaves[:2]:
        t[~prep.live] = value
    ia, ib = prep.idx[0].clone(), prep.idx[1].clone()
    ia[~prep.live], ib[~prep.live] = ia_pad, ib_pad
    g = prep.g.float().view(prep.case["b"], prep.case["n"], 3).clone()
    g[~prep.live] = g_pad
    return [t.to(DEV) for t in leaves], (ia.to(DEV), ib.to(DEV)), g.to(DEV)


def public(be, leaves, idx, g, lengths):
    """be.fusion_bn with requires_grad leaves -> [out, bn, var, (count,) 14 gradients]"""
    leaves = [t.clone().requires_grad_(True) for t in leaves]
    res = be.fusion_bn(leaves[0], leaves[1], idx, leaves[2:8], leaves[8:], br.EPS, **({} if lengths is None else dict(lengths=lengths)))
    return [t.detach() for t in res] + list(torch.autograd.grad(res[0], leaves, g))


def skip_unless_256(case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if case["b"] * case["n"] > 1024 and cus != 256:
        pytest.skip(f"the grid caps are multiples of the CU count and the case is chosen for 256 CUs; this device has {cus}")


def test_the_entry_points_exist():
    lib = _lib.load()
    assert lib.mcp_fusion_bn_forward_lengths and lib.mcp_fusion_bn_backward_lengths


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fusion_on_batch_statistics_with_lengths_matches_float64(case):
    skip_unless_256(case)
    cid = case_id(case)
    prep = lr.prepare(case)
    lib, be = _lib.load(), ops.backend()
    B, N, names = case["b"], case["n"], prep.names
    lens = torch.tensor(case["lens"], dtype=torch.int32, device=DEV)
    live_d = prep.live.to(DEV)
    labels = ["out", "bn", "var", "count"] + names

    # ---- poisoning, repeatability, padding invariance ----
    leaves, halves, g = poisoned(prep)
    with poisoned_buffers():
        hip, again = public(be, leaves, halves, g, lens), public(be, leaves, halves, g, lens)
        other = public(be, *poisoned(prep, value=7.5, ia_pad=3 % N, ib_pad=BIG + 1, g_pad=1.0), lens)
    for name, a, a2, a3 in zip(labels, hip, again, other):
        assert torch.isfinite(a).all(), f"{name}: not finite"
        assert torch.equal(a, a2), f"{name}: a second forward + backward gives other bits"
        assert torch.equal(a, a3), f"{name}: other values in the padded rows change the result"
    out, bn, var, count = hip[:4]
    grads = dict(zip(names, hip[4:]))
    assert int(count) == prep.live_points, f"count {int(count)}, live points {prep.live_points}"
    assert not out[~live_d].any(), "out: a padded row is not zero"
    assert not grads["p1"][~live_d].any() and not grads["p2"][~live_d].any(), "a padded point has a gradient"
    for name in br.CONV_BIASES:
        assert not grads[name].any(), f"{name}: a conv bias in front of a batch-statistics BatchNorm has a gradient"

    # ---- on the unpadded batch: len = NULL and full lengths are the dense entry points, bit for bit ----
    clean = [t.to(DEV) for t in prep.leaves]
    chalves = tuple(t.to(DEV) for t in prep.idx)
    cg = torch.where(live_d.unsqueeze(-1), g, torch.zeros((), device=DEV))
    with poisoned_buffers():
        dense = public(be, clean, chalves, cg, None)
        full = public(be, clean, chalves, cg, torch.full((B,), N, dtype=torch.int32, device=DEV))
    assert int(full[3]) == B * N
    for name, a, b in zip(["out", "bn", "var"] + names, dense, full[:3] + full[4:]):
        assert torch.equal(a, b), f"{name}: every length n gives other bits than the dense entry point"
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rows = B * N * 64

    def forward_null():
        with poisoned_buffers():
            r = dict(bn=dense[1].clone(), var=torch.empty(256, device=DEV), out=torch.empty(B, N, 3, device=DEV), count=torch.empty(1, dtype=torch.int32, device=DEV),
                     ws=torch.empty(lib.mcp_fusion_bn_workspace_bytes(B, N), dtype=torch.uint8, device=DEV))
        rc = lib.mcp_fusion_bn_forward_lengths(B, N, 64, P(clean[0]), P(clean[1]), P(chalves[0]), P(chalves[1]), None, *[P(t) for t in clean[2:8]], br.EPS,
                                               P(r["bn"]), P(r["var"]), P(r["out"]), P(r["count"]), P(r["ws"]), r["ws"].numel(), st)
        assert rc == 0
        return r

    def backward(name, with_len):
        need = lib.mcp_fusion_bn_grad_workspace_bytes(B, N)
        with poisoned_buffers():
            scr = dict(row_c=torch.empty(rows, dtype=torch.int32, device=DEV), row_dy=torch.empty(rows, device=DEV), row_a=torch.empty(rows, device=DEV),
                       dy2=torch.empty(rows, 64, device=DEV), dy1=torch.empty(rows, 64, device=DEV), d_p1=torch.empty_like(clean[0]),
                       d_nb=torch.empty(B, N, 64, 3, device=DEV), d_w=torch.empty(lib.mcp_fusion_grad_floats(), device=DEV),
                       d_aff=torch.empty(512, device=DEV), ws=torch.empty(need, dtype=torch.uint8, device=DEV))
        rc = getattr(lib, name)(B, N, 64, P(clean[0]), P(clean[1]), P(chalves[0]), P(chalves[1]), *((None,) if with_len else ()), *[P(t) for t in clean[2:8]],
                                P(dense[1]), P(cg), P(scr["row_c"]), P(scr["row_dy"]), P(scr["row_a"]), P(scr["dy2"]), P(scr["dy1"]), P(scr["d_p1"]),
                                P(scr["d_nb"]), P(scr["d_w"]), P(scr["d_aff"]), P(scr["ws"]), need, st)
        assert rc == 0, name
        torch.cuda.synchronize()
        return scr
    null = forward_null()
    torch.cuda.synchronize()
    assert torch.equal(null["out"], dense[0]) and torch.equal(null["bn"], dense[1]) and torch.equal(null["var"], dense[2]) and int(null["count"]) == B * N
    a, b = backward("mcp_fusion_bn_backward", False), backward("mcp_fusion_bn_backward_lengths", True)
    for k in ("row_c", "row_dy", "row_a", "dy2", "dy1", "d_p1", "d_nb", "d_w", "d_aff"):
        assert torch.equal(a[k], b[k]), f"{k}: len = NULL gives other bits than the dense backward"

    if prep.live_points == 0:   # m = 0: nothing is NaN or Inf (above), every gradient is zero, the statistics mean nothing
        for name in names:
            assert not grads[name].any(), f"{name}: a gradient without a live point"
        return

    # ---- the float32 torch formulation on the device: the yardstick ----
    tl = [t.clone().requires_grad_(True) for t in leaves]
    tout, tbn, tvar, _ = grad.fusion_bn_lengths_twin(None, tl[0], tl[1], torch.cat(halves, -1), tl[2:8], tl[8:], br.EPS, lens)
    twin = dict(zip(names, torch.autograd.grad(tout, tl, torch.where(live_d.unsqueeze(-1), g, torch.zeros((), device=DEV)))))

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
         float((tout.detach().double().cpu().view(-1, 3) - ev.out).abs().max()) / scale, f" max|exact|={scale:.3e}")
    biases = [prep.leaves[k].double() for k in (3, 5, 7)]
    mean, rstd, hvar = statistics(bn, var)
    tmean, trstd, tv = statistics(tbn, tvar)
    for label, e, t in zip(("mean", "rstd", "var"), statistic_errors(mean, rstd, hvar, ev, biases), statistic_errors(tmean, trstd, tv, ev, biases)):
        held(label, label, e, t)
    exact = dict(zip(names, lr.gradients(prep)))
    for name in names:
        if name in br.CONV_BIASES:
            continue
        a, t32, e = grads[name].double().cpu(), twin[name].double().cpu(), exact[name]
        scale = float(e.abs().max())
        if lr.exact_zero(prep, name):
            print(f"RATIO {cid} {name} [{br.group(name)}, zero in exact arithmetic] max|exact|={scale:.1e} max|hip|={float(a.abs().max()):.3e} max|twin|={float(t32.abs().max()):.3e}")
            assert scale <= 1e-12
            if not float(a.abs().max()) <= FLOOR:
                failures.append(f"{name}: {float(a.abs().max()):.2e} where exact arithmetic gives zero")
            continue
        held(name, br.group(name), float((a - e).abs().max()) / scale, float((t32 - e).abs().max()) / scale, f" max|exact|={scale:.3e}")

    # ---- the mutants ----
    def statistics_mutant(tag, m, v):
        mut_rstd = torch.rsqrt(v + br.EPS)
        on_mean = float(((mean[2] - m).abs() / (m.abs() + v.sqrt())).max()) / C["mean"]
        on_rstd = float(((rstd[2] - mut_rstd).abs() / mut_rstd).max()) / C["rstd"]
        print(f"RATIO {cid} layer-3 statistics mutant {tag}: mean={on_mean:.2f} rstd={on_rstd:.2f}")
        if not (on_mean > 1.0 or on_rstd > 1.0):
            failures.append(f"the bounds do not see the layer-3 statistics {tag} (mean {on_mean:.2f}, rstd {on_rstd:.2f})")
    if prep.live_points > 1:
        statistics_mutant("without the last live point", *lr.stats3_without_last(prep))
        if prep.live_points < B * N:
            gen = torch.Generator().manual_seed(5)
            statistics_mutant("with one padded point counted in", *lr.stats3_with_padded(prep, torch.tensor([5.0, -3.0, 2.0]), 3.0 * torch.randn(64, 3, generator=gen)))
        if not lr.exact_zero(prep, "w3"):
            p = int(prep.clear_points()[-1])
            contrib = dict(zip(names, lr.gradients(prep, sel=[p])))["w3"]
            a, e = grads["w3"].double().cpu(), exact["w3"]
            dropped = float((a - (e - contrib)).abs().max()) / (C["weight"] * float(e.abs().max()))
            print(f"RATIO {cid} w3 mutant without the last clear live point {p}: dropped={dropped:.2f}")
            if not dropped > 1.0:
                failures.append(f"w3: the bound does not see point {p} dropped ({dropped:.2f})")
    prep.release()
    assert not failures, "; ".join(failures)


def test_the_dense_entry_point_on_a_padded_batch_is_outside_the_bound():
    """What the length form is for: len = (40, 0, 17) run WITHOUT lengths (zeros in the padded rows, their 64 rows each counted in)
    puts the layer-1 mean far outside the bound that the length form is held to."""
    case = next(c for c in CASES if c["tag"] == "empty-middle")
    prep = lr.prepare(case)
    be = ops.backend()
    dl = [t.to(DEV) for t in prep.leaves]
    _, bn, var = be.fusion_bn_forward(dl[0], dl[1], tuple(t.to(DEV) for t in prep.idx), dl[2:8], dl[8:], br.EPS)
    errs = statistic_errors(*statistics(bn, var), prep.ev, [prep.leaves[k].double() for k in (3, 5, 7)])
    assert errs[0] > 100 * C["mean"], errs


def test_fusion_mlp_with_lengths_is_the_dense_kernel_plus_masking():
    case = next(c for c in CASES if c["tag"] == "empty-middle")
    prep = lr.prepare(case)
    be = ops.backend()
    live = prep.live.to(DEV).unsqueeze(-1)
    lens = torch.tensor(case["lens"], dtype=torch.int32, device=DEV)
    g = torch.randn(case["b"], case["n"], 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    leaves, halves, _ = poisoned(prep)

    def run(lv, idx, up, **kw):
        lv = [t.clone().requires_grad_(True) for t in lv[:8]]
        out = be.fusion_mlp(lv[0], lv[1], idx, *lv[2:], **kw)
        return [out.detach()] + list(torch.autograd.grad(out, lv, up))
    with poisoned_buffers():
        masked = run(leaves, halves, g, lengths=lens)
        dense = run([t.to(DEV) for t in prep.leaves], tuple(t.to(DEV) for t in prep.idx), torch.where(live, g, torch.zeros((), device=DEV)))
        plain = be.fusion_mlp(leaves[0], leaves[1], halves, *leaves[2:8], lengths=lens)     # without autograd: the forward kernel alone
    assert torch.equal(plain, masked[0])
    assert not masked[0][~live.squeeze(-1)].any() and torch.equal(masked[0][live.squeeze(-1)], dense[0][live.squeeze(-1)])
    for name, a, b in zip(prep.names[:8], masked[1:], dense[1:]):
        assert torch.isfinite(a).all() and torch.equal(a, b), f"{name}: the gradient differs from the dense call on the batch zeroed by hand"
    assert not masked[1][~live.squeeze(-1)].any()


def test_the_model_updates_its_running_estimates_with_the_live_rows():
    """fusion_batch_stats(lengths=): running_var moves by m / (m - 1) of the live rows (m = 64 * 57 here, not 64 * 120),
    running_mean by the batch mean, num_batches_tracked by the calls -- as the dense path does."""
    from tests import harness_checks as hc
    case = next(c for c in CASES if c["tag"] == "empty-middle")
    prep = lr.prepare(case)
    net = hc.build_model(DEV)
    m = "multi_frame_inference.conv."
    leaves, halves, _ = poisoned(prep)
    lens = torch.tensor(case["lens"], dtype=torch.int32, device=DEV)
    sd = dict(net.named_buffers())
    before = {k: sd[m + k].clone() for k in ("1.running_mean", "1.running_var", "7.running_var", "7.num_batches_tracked")}
    P = net._params()
    conv = [t for ci in (0, 3, 6) for t in (net.W(m + str(ci)), net.Bv(m + str(ci)))]
    aff = [t for bi in (1, 4, 7) for t in (P[m + f"{bi}.weight"], P[m + f"{bi}.bias"])]
    _, bn, var, count = ops.backend().fusion_bn_forward(leaves[0], leaves[1], halves, conv, aff, 1e-3, lengths=lens)
    out = net.fusion_batch_stats(leaves[0], leaves[1], halves, 1, lengths=lens)
    assert torch.isfinite(out).all() and int(count) == 57
    mom, rows = net.BN_MOMENTUM, 64.0 * 57
    after = dict(net.named_buffers())
    assert torch.allclose(after[m + "1.running_mean"], (1 - mom) * before["1.running_mean"] + mom * bn[0:64], rtol=1e-6, atol=1e-7)
    assert torch.allclose(after[m + "1.running_var"], (1 - mom) * before["1.running_var"] + mom * var[0:64] * (rows / (rows - 1)), rtol=1e-6, atol=1e-8)
    assert torch.allclose(after[m + "7.running_var"], (1 - mom) * before["7.running_var"] + mom * var[128:256] * (rows / (rows - 1)), rtol=1e-6, atol=1e-8)
    assert int(after[m + "7.num_batches_tracked"]) == int(before["7.num_batches_tracked"]) + 1


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_the_models_fusion_hands_lengths_to_the_searches_and_the_layer(mode):
    """MoCoPCI.fusion(lengths=): the two neighbour searches see live rows only and the layer runs on live points.  eval (folded
    BatchNorm, per-point kernel): a cloud's live rows have the bits of the same call on that cloud alone, cut to its length, and
    padded rows are zero.  train: out is finite, zero on padded rows, and the running estimates are finite."""
    from tests import harness_checks as hc
    net = hc.build_model(DEV)
    n, lens = 48, (48, 33)
    gen = torch.Generator().manual_seed(11)
    p1 = torch.randn(2, n, 3, generator=gen).to(DEV)
    p2 = (p1.cpu() + 0.1 * torch.randn(2, n, 3, generator=gen)).to(DEV)
    live = torch.arange(n, device=DEV).view(1, n) < torch.tensor(lens, device=DEV).view(2, 1)
    p1n, p2n = p1.clone(), p2.clone()
    p1n[~live] = p2n[~live] = float("nan")
    if mode == "train":
        net._mode = (0.0, 0.0, 0.0)
    try:
        out = net.fusion(p1n, p2n, lengths=lens)
        assert torch.isfinite(out).all() and not out[~live].any()
        if mode == "eval":
            for e, ln in enumerate(lens):
                alone = net.fusion(p1[e:e + 1, :ln].contiguous(), p2[e:e + 1, :ln].contiguous())
                assert torch.equal(out[e, :ln], alone[0]), f"element {e}: other bits than the cloud alone"
        else:
            assert all(torch.isfinite(b).all() for k, b in net.named_buffers() if k.startswith("multi_frame_inference.conv."))
    finally:
        net._mode = None
