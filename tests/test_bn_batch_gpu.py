"""-m gpu: BatchNorm on batch statistics with per-group lengths (csrc/bn_batch.hip; mcp_bn_batch_forward / mcp_bn_batch_backward,
ops.HipBackend.bn_batch) against the float64 reference of tests/bn_batch_reference.py, whose CASES name the edge each case reaches:
one live row (m = 1, var 0), no live row at all, an empty group between two live ones, live rows that are not contiguous across frames,
C = 256 with a one-point group, a length that ends inside the second of three parts (the third is all padding), lengths exactly on
part boundaries, and channels 3000 sigma from zero (`far`: a variance from unshifted float32 sums fails there).

Every case: padded rows of x and of the upstream gradient are NaN, every buffer the calls allocate is NaN-filled beforehand
(poisoned_buffers).  y, mean, var, count, dx, dgamma and dbeta are finite; y and dx are exactly zero on padded rows; count = F * len;
a second forward + backward gives identical bits; other values in the padded rows change no bit; on the unpadded batch full lengths
give the bits of len = NULL.  Against float64, ratio = max|hip - exact| / (c * scale) <= 1 per group of outputs:
  out, dx   scale = max|exact| of the tensor;          mean   scale = |mean| + sqrt(var), per group and channel;
  var       scale = var + eps;                         rstd   scale = rstd (rstd = rsqrt(var + eps) of the returned variance);
  affine    dgamma and dbeta, scale = max|exact| of each.
The bound must bite: for every group with m >= 2 the float64 statistics without its last live row, and with one padded row (finite
garbage) counted in, lie outside the mean or the rstd bound, and dgamma without that group's last live row's term lies outside the
affine bound.

c: the smallest power of two that is at least twice the worst ratio measured on the MI355X over the cases, the C = 48 one included (in
brackets, with the case that set it; profiles/bn_batch_accuracy.txt holds every RATIO line beside the float32 torch formulation on the
device, a yardstick that nothing is asserted on)."""
import pytest
import torch

from mocopci_amd import _lib, grad, ops
from tests import bn_batch_reference as ref
from tests.bn_batch_reference import CASES, EPS, case_id
from tests.test_fused_grad_variants_gpu import poisoned_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# group: c   [worst max|hip - exact| / scale: case]
C = {
    "out": 2.0 ** -13,       # [3.91e-5: far -- the float32 mean of a channel at 300 with sigma 0.1 is 1.5e-4 sigma off; the torch formulation 7.0e-5]
    "mean": 2.0 ** -22,      # [6.98e-8: fallback-c48 (the torch formulation); the kernels 5.17e-8: wide]
    "var": 2.0 ** -21,       # [1.51e-7: fallback-c48; the kernels 5.74e-8: empty-middle]
    "rstd": 2.0 ** -22,      # [7.56e-8: fallback-c48; the kernels 2.87e-8: empty-middle]
    "dx": 2.0 ** -14,        # [2.05e-5: far]
    "affine": 2.0 ** -12,    # [7.89e-5: far, dgamma -- xhat of the channels at 300 carries the rounded mean]
}
FALLBACK = dict(tag="fallback-c48", g=2, f=2, n=37, c=48, lens=(37, 11))


def padded(prep, value, g_value):
    """(x, dy) on the device with the padded rows replaced."""
    pad = ~prep.live.view(prep.case["g"], 1, prep.case["n"], 1).expand_as(prep.x)
    x, dy = prep.x.clone(), prep.dy.clone()
    x[pad], dy[pad] = value, g_value
    return x.to(DEV), dy.to(DEV)


def public(fn, x, dy, gamma, beta, lengths):
    """fn = be.bn_batch or the torch formulation -> [y, mean, var, count, dx, dgamma, dbeta]"""
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    res = fn(*leaves, EPS, lengths)
    return [t.detach() for t in res] + list(torch.autograd.grad(res[0], leaves, dy))


LABELS = ["y", "mean", "var", "count", "dx", "dgamma", "dbeta"]


def errors(res, ev):
    """{group: max|res - exact| / scale}; None where exact arithmetic gives zero everywhere (the caller asserts zeros)."""
    y, mean, var, _, dx, dgamma, dbeta = [t.double().cpu() for t in res]
    live = ev.count > 0
    out = {}

    def rel(a, e):
        s = float(e.abs().max())
        return None if s <= 1e-12 else float((a - e).abs().max()) / s
    out["out"], out["dx"] = rel(y, ev.y), rel(dx, ev.dx)
    aff = [r for r in (rel(dgamma, ev.dgamma), rel(dbeta, ev.dbeta)) if r is not None]
    out["affine"] = max(aff) if aff else None
    if not live.any():
        out["mean"] = out["var"] = out["rstd"] = None
        return out
    out["mean"] = float(((mean - ev.mean).abs() / (ev.mean.abs() + ev.var.sqrt()))[live].max())
    out["var"] = float(((var - ev.var).abs() / (ev.var + EPS))[live].max())
    rstd, exact = torch.rsqrt(var + EPS), torch.rsqrt(ev.var + EPS)
    out["rstd"] = float(((rstd - exact).abs() / exact)[live].max())
    return out


def check_case(case, fn, kernel):
    cid = case_id(case)
    prep = ref.prepare(case)
    ev = prep.ev
    G, Fr, N = case["g"], case["f"], case["n"]
    lens = torch.tensor(case["lens"], dtype=torch.int32, device=DEV)
    gamma, beta = prep.gamma.to(DEV), prep.beta.to(DEV)
    pad_d = ~prep.live.to(DEV).view(G, 1, N, 1).expand(G, Fr, N, case["c"])

    # ---- poisoning, repeatability, padding invariance ----
    x, dy = padded(prep, float("nan"), float("nan"))
    with poisoned_buffers():
        hip, again = public(fn, x, dy, gamma, beta, lens), public(fn, x, dy, gamma, beta, lens)
        other = public(fn, *padded(prep, 7.5, 1.0), gamma, beta, lens)
    for name, a, a2, a3 in zip(LABELS, hip, again, other):
        assert torch.isfinite(a).all(), f"{name}: not finite"
        assert torch.equal(a, a2), f"{name}: a second forward + backward gives other bits"
        assert torch.equal(a, a3), f"{name}: other values in the padded rows change the result"
    assert hip[3].dtype == torch.int32 and hip[3].tolist() == [Fr * ln for ln in case["lens"]], f"count {hip[3].tolist()}"
    assert not hip[0][pad_d].any(), "y: a padded row is not zero"
    assert not hip[4][pad_d].any(), "dx: a padded row is not zero"

    # ---- on the unpadded batch: full lengths are len = NULL, bit for bit ----
    cx, cdy = prep.x.to(DEV), prep.dy.to(DEV)
    with poisoned_buffers():
        dense = public(fn, cx, cdy, gamma, beta, None)
        full = public(fn, cx, cdy, gamma, beta, torch.full((G,), N, dtype=torch.int32, device=DEV))
    assert full[3].tolist() == [Fr * N] * G
    for name, a, b in zip(LABELS, dense, full):
        assert torch.equal(a, b), f"{name}: every length n gives other bits than len = NULL"

    # ---- accuracy against float64, beside the float32 torch formulation (the yardstick) ----
    twin = public(grad.bn_batch_lengths_twin, x, dy, gamma, beta, lens)
    mine, yard = errors(hip, ev), errors(twin, ev)
    failures = []
    print()
    for group in C:
        if mine[group] is None:     # exact arithmetic gives zero: so do the kernels (x - mean is exact with one live row)
            which = {"out": [0], "dx": [4], "affine": [5, 6], "mean": [1], "var": [2], "rstd": [2]}[group]
            print(f"RATIO {cid} [{group}, zero in exact arithmetic] max|hip|={max(float(hip[k].abs().max()) for k in which):.3e}")
            if kernel and any(hip[k].any() for k in which):
                failures.append(f"{group}: not zero where exact arithmetic gives zero")
            continue
        print(f"RATIO {cid} [{group}] err/scale={mine[group]:.3e} kernel={mine[group] / C[group]:.3f} twin={yard[group] / C[group]:.3f}")
        if not mine[group] <= C[group]:
            failures.append(f"{group}: error {mine[group]:.2e} of its scale, allowed {C[group]:.2e}")

    # ---- the mutants ----
    mean, var = hip[1].double().cpu(), hip[2].double().cpu()
    rstd = torch.rsqrt(var + EPS)
    x64 = prep.x.double()
    gen = torch.Generator().manual_seed(5)
    for g, ln in enumerate(case["lens"]):
        m = Fr * ln
        if m < 2:
            continue

        def statistics_mutant(tag, mu, v):
            mut = torch.rsqrt(v + EPS)
            on_mean = float(((mean[g] - mu).abs() / (mu.abs() + v.sqrt())).max()) / C["mean"]
            on_rstd = float(((rstd[g] - mut).abs() / mut).max()) / C["rstd"]
            print(f"RATIO {cid} group {g} statistics mutant {tag}: mean={on_mean:.2f} rstd={on_rstd:.2f}")
            if not (on_mean > 1.0 or on_rstd > 1.0):
                failures.append(f"the bounds do not see group {g}'s statistics {tag} (mean {on_mean:.2f}, rstd {on_rstd:.2f})")
        _, mu, v, _ = ref.forward(x64, prep.lens, prep.gamma.double(), prep.beta.double(), skip=(g, m - 1))
        statistics_mutant("without the last live row", mu[g], v[g])
        if ln < N:
            rows = torch.cat([x64[g, :, :ln].reshape(m, -1), (7.5 + 3.0 * torch.randn(1, case["c"], generator=gen)).double()])
            statistics_mutant("with one padded row counted in", rows.mean(0), rows.var(0, unbiased=False))
        _, dgamma, _ = ref.backward(x64, prep.lens, prep.gamma.double(), ev.mean, ev.var, prep.dy.double(), skip=(g, m - 1))
        dropped = float((hip[5].double().cpu() - dgamma).abs().max()) / (C["affine"] * float(ev.dgamma.abs().max()))
        print(f"RATIO {cid} group {g} dgamma mutant without the last live row's term: dropped={dropped:.2f}")
        if not dropped > 1.0:
            failures.append(f"dgamma: the bound does not see group {g}'s last live row dropped ({dropped:.2f})")
    assert not failures, "; ".join(failures)


def test_the_entry_points_exist():
    lib = _lib.load()
    assert lib.mcp_bn_batch_forward and lib.mcp_bn_batch_backward and hasattr(ops.backend(), "bn_batch")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bn_batch_with_lengths_matches_float64(case):
    check_case(case, ops.backend().bn_batch, kernel=True)


def test_an_unsupported_width_takes_the_torch_formulation_and_meets_the_same_bounds():
    """C = 48: no kernel (mcp_bn_batch_forward returns MCP_ERR_UNSUPPORTED); ops.bn_batch raises nothing and returns the masked torch
    formulation, held to the constants of the kernels."""
    assert _lib.load().mcp_bn_batch_parts(2, 2, 37, 48) == 10002
    check_case(FALLBACK, ops.backend().bn_batch, kernel=False)


def test_the_dense_call_on_a_padded_batch_is_outside_the_bound():
    """What the length form is for: lens (37, 0, 11) run WITHOUT lengths (zeros in the padded rows, counted in) puts the mean far
    outside the bound that the length form is held to."""
    prep = ref.prepare(next(c for c in CASES if c["tag"] == "empty-middle"))
    x, dy = padded(prep, 0.0, 0.0)
    res = public(ops.backend().bn_batch, x, dy, prep.gamma.to(DEV), prep.beta.to(DEV), None)
    assert errors(res, prep.ev)["mean"] > 100 * C["mean"]
