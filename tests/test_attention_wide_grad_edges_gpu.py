"""-m gpu: the wide-head attention in a training graph (csrc/attention_wide_grad.hip: the training forward with its kept log-sum-exp,
attention_wide_dsum_kernel, attention_wide_dq_kernel, attention_wide_dkv_kernel at head widths 32 / 64 / 256) at query / key counts on
and next to the kernels' own boundaries -- a wave's tile of 32 rows, a workgroup block of 128 rows (widths 32 / 64) or 32 rows shared
by four channel slices (width 256), a streamed stage of 32 rows fetched one stage ahead, the key-split forward's four waves -- against
float64 autograd over the dense (masked) formulation of tests/attention_lengths_reference.py.  tests/test_attention_lengths_gpu.py
walks such edges through the lengths inside a fixed launch; here the bounds are the launch's own nq / nk (the plain kernels' dead
lanes are different code), and dropout meets the lengths at every width.  kernel_variants.WIDE_GRAD_COUNTS is the grid,
WIDE_GUARD_CASES / WIDE_TRAIN_CASES the explicit cases; test_kernel_variants_cpu.py checks that together they launch every kernel the
unit emits and reach every boundary class.

Bounds, all the project's own for these kernels: output rtol 1e-4, atol 1e-5; log-sum-exp rtol = atol = 1e-5
(test_attention_wide_grad_gpu.py); gradients max |hip - f64| <= 1e-4 max |f64| + 1e-6 per tensor (test_grad_gpu.py).  Lines starting
with ERR carry each error as a fraction of its bound (profiles/attention_wide_grad_edges_accuracy.txt).

One key (nk = 1): the softmax is 1 whatever q and k hold, so dQ and dK are exactly zero and the gradient bound is its floor of 1e-6,
while ds = p (dP - D) subtracts two fp32 sums of the same hd products dO_c V_c taken in different orders (an MFMA chain, a lane
butterfly): with unit normals that difference is a few ulp of a sum of hd products, and dQ came to 0.99e-6 and 1.33e-6 at head width
32 (nq = 1 and 32, measured on the MI355X) -- the reference is ill-conditioned there, not the kernel wrong
(test_attention_wide_grad_gpu.py allows 1e-5 for its one-token case for the same reason).  In that column of the grid v and grad_out
are therefore rounded to multiples of 1 / 4: every product is a multiple of 1 / 16 and every partial sum stays below 2^12 (checked on
the CPU over 200 seeds per head width: the fp32 sum equals the float64 one in any order), so dP, D and their difference are exact in
fp32 and the kernels must give dQ = dK = 0 to the last bit -- which the same bound then asserts."""
import ctypes

import pytest
import torch

from mocopci_amd import _lib, ops
from tests import attention_lengths_reference as ref
from tests import kernel_variants as kv
from tests.test_attention_lengths_gpu import assert_zero_beyond, padded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, HEADS = 2, 2
CANARY = 1234.5
P_DROP = 0.25


def rnd(seed, *shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


def inputs(seed, bf, heads, hd, nq, nk, factor=1.0):
    """(q, kv, grad_out) on the device: unit normals from seeded CPU generators, q times `factor`.  With a single key, v and grad_out are
    rounded to multiples of 1 / 4 (see the module's docstring)."""
    C = heads * hd
    q, kv_, g = rnd(seed, bf, nq, C) * factor, rnd(seed + 1, bf, nk, 2 * C), rnd(seed + 2, bf, nq, C)
    if nk == 1:
        kv_[..., C:], g = torch.round(kv_[..., C:] * 4) / 4, torch.round(g * 4) / 4
    return q.to(DEV), kv_.to(DEV), g.to(DEV)


def lens_of(c):
    """(qlen, klen) of a case as (BF,) int32 device tensors or None."""
    return (ops.lengths_tensor(None if c["qlen"] is None else list(c["qlen"]), c["bf"], c["nq"], DEV),
            ops.lengths_tensor(None if c["klen"] is None else list(c["klen"]), c["bf"], c["nk"], DEV))


def train(q, kv_, g, heads, p=0.0, seed=0, qlen=None, klen=None):
    """(out, lse, grad_q, grad_kv) of the layer's autograd function -- what be.attention runs in a training graph."""
    be = ops.backend()
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, kv_)]
    out = ops._AttentionWideFn.apply(be, *leaves, heads, (q.shape[2] // heads) ** -0.5, p, seed, qlen, klen)
    lse = out.grad_fn.saved_tensors[3]
    gq, gkv = torch.autograd.grad(out, leaves, g)
    return out.detach(), lse, gq, gkv


def same_bits(a, b, label):
    for name, x, y in zip(("out", "lse", "grad_q", "grad_kv"), a, b):
        assert torch.equal(x, y), f"{label}: {name} differs"


def close_ratio(got, want, rtol, atol):
    return float(((got.double() - want).abs() / (atol + rtol * want.abs())).max())


def check(got, want, label):
    """out, lse, grad_q, grad_kv against float64 at the module's bounds; the four errors as fractions of their bounds."""
    out, lse, gq, gkv = got
    w_out, w_lse, wq, wkv = want
    for name, t in zip(("out", "lse", "grad_q", "grad_kv"), got):
        assert bool(torch.isfinite(t).all()), f"{label}: {name} is not finite"
    ratios = [close_ratio(out, w_out, 1e-4, 1e-5), close_ratio(lse, w_lse, 1e-5, 1e-5)]
    for a, w in ((gq, wq), (gkv, wkv)):
        ratios.append(float((a.double() - w).abs().max()) / ref.grad_bound(w))
    print(f"ERR attention_wide_grad[{label}] out={ratios[0]:.3f} lse={ratios[1]:.3f} dq={ratios[2]:.3f} dkv={ratios[3]:.3f} of the bound")
    torch.testing.assert_close(out.double(), w_out, rtol=1e-4, atol=1e-5, msg=lambda m: f"{label}: out: {m}")
    torch.testing.assert_close(lse.double(), w_lse, rtol=1e-5, atol=1e-5, msg=lambda m: f"{label}: lse: {m}")
    for name, a, w in (("q", gq, wq), ("kv", gkv, wkv)):
        err, bound = float((a.double() - w).abs().max()), ref.grad_bound(w)
        assert err <= bound, f"{label}: grad {name}: max err {err:.2e} > bound {bound:.2e}"
    return ratios


def form(bf, heads, hd, nq, nk):
    return "ksplit" if hd == 256 and kv.wide_keys_split(bf, nq, nk, heads) else "qs"


# ---- (a) the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", kv.WIDE_GRAD_COUNTS)
@pytest.mark.parametrize("hd", kv.WIDE_HEAD_WIDTHS)
def test_wide_attention_training_at_the_tile_boundaries(hd, nq):
    """One query count against every key count of the grid, through be.attention in a training graph."""
    be = ops.backend()
    for nk in kv.WIDE_GRAD_COUNTS:
        label = f"hd={hd},nq={nq},nk={nk},{form(BF, HEADS, hd, nq, nk)}"
        q, kv_, g = inputs(1000 * nq + 10 * nk + hd, BF, HEADS, hd, nq, nk)
        leaves = [t.clone().requires_grad_(True) for t in (q, kv_)]
        out = be.attention(*leaves, HEADS)
        assert type(out.grad_fn).__name__ == "_AttentionWideFnBackward"
        got = (out.detach(), out.grad_fn.saved_tensors[3]) + torch.autograd.grad(out, leaves, g)
        same_bits(got, train(q, kv_, g, HEADS), label + ": two runs")
        check(got, ref.reference(q, kv_, HEADS, None, None, g), label)
        if nk == 1:   # exactly summable v and grad_out (the module's docstring): dP - D is an exact zero
            assert not bool(got[2].any()) and not bool(got[3][..., :HEADS * hd].any()), f"{label}: dQ and dK of a single key are not exact zeros"


# ---- (b) guard rows --------------------------------------------------------------------------------------------------------------------
def guarded(rows, width):
    """A (rows, width) view with one canary row in front and one behind, and the buffer that holds all three parts."""
    buf = torch.full((rows + 2, width), CANARY, device=DEV)
    return buf[1:-1], buf


def untouched(buf, label):
    assert bool((buf[0] == CANARY).all()), f"{label}: the row in front was written"
    assert bool((buf[-1] == CANARY).all()), f"{label}: the row behind was written"


def c_entries(c, q, qs, k, ks, v, vs, g, p, seed, qlen, klen, guard=False):
    """mcp_attention_wide_lse[_lengths] then mcp_attention_wide_grad_lse[_lengths] on raw pointers -> (out, lse, grad_q, grad_kv); with
    guard every output and the workspace is a view between two canary rows, checked after the calls."""
    lib = _lib.load()
    bf, heads, hd, nq, nk = c["bf"], c["heads"], c["hd"], c["nq"], c["nk"]
    C, scale = heads * hd, hd ** -0.5
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    need = lib.mcp_attention_wide_grad_workspace_bytes(bf, nq, nk, heads, hd)
    assert need == 4 * bf * heads * nq
    (out, b_out), (lse, b_lse), (gq, b_gq), (gkv, b_gkv), (ws, b_ws) = (guarded(bf * nq, C), guarded(bf * heads, nq), guarded(bf * nq, C),
                                                                      guarded(bf * nk, 2 * C), guarded(bf * heads, nq))
    lens = qlen is not None or klen is not None
    tail = (None if qlen is None else P(qlen), None if klen is None else P(klen)) if lens else ()
    fwd = lib.mcp_attention_wide_lse_lengths if lens else lib.mcp_attention_wide_lse
    bwd = lib.mcp_attention_wide_grad_lse_lengths if lens else lib.mcp_attention_wide_grad_lse
    assert fwd(bf, nq, nk, heads, hd, P(q), qs, P(k), ks, P(v), vs, scale, p, seed, P(out), P(lse), *tail, st) == 0
    assert bwd(bf, nq, nk, heads, hd, P(q), qs, P(k), ks, P(v), vs, scale, p, seed, P(out), P(g), P(lse), P(gq), P(gkv), P(ws), need, *tail, st) == 0
    torch.cuda.synchronize()
    if guard:
        for name, buf in (("out", b_out), ("lse", b_lse), ("grad_q", b_gq), ("grad_kv", b_gkv), ("workspace", b_ws)):
            untouched(buf, f"{kv.wide_case_id(c)}: {name}")
    return out.view(bf, nq, C), lse.view(bf, heads, nq), gq.view(bf, nq, C), gkv.view(bf, nk, 2 * C)


def kv_entries(c, q, kv_, g, p=0.0, seed=0, qlen=None, klen=None, guard=False):
    C = c["heads"] * c["hd"]
    return c_entries(c, q, C, kv_[..., :C], 2 * C, kv_[..., C:], 2 * C, g, p, seed, qlen, klen, guard)


@pytest.mark.parametrize("c", kv.WIDE_GUARD_CASES, ids=kv.wide_case_id)
def test_partial_tiles_store_only_their_own_rows(c):
    """The C entries with out, lse, grad_q, grad_kv and the workspace between canary rows: the canaries are untouched, the live part is
    the public call's bit for bit, and with lengths the rows between a length and the launch bound are exact zeros."""
    label = kv.wide_case_id(c)
    assert ("ksplit" in label) == (c["heads"] == 1)
    q, kv_, g = inputs(4000 + c["hd"] + c["nk"], c["bf"], c["heads"], c["hd"], c["nq"], c["nk"])
    qlen, klen = lens_of(c)
    got = kv_entries(c, q, kv_, g, qlen=qlen, klen=klen, guard=True)
    same_bits(got, train(q, kv_, g, c["heads"], qlen=qlen, klen=klen), label + ": C entries against the public call")
    check(got, ref.reference(q, kv_, c["heads"], c["qlen"], c["klen"], g), label)
    if c["qlen"] is not None:
        out, lse, gq, gkv = got
        assert_zero_beyond(out, c["qlen"], "out")
        assert_zero_beyond(gq, c["qlen"], "grad_q")
        assert_zero_beyond(gkv, c["klen"], "grad_kv")
        for b, n in enumerate(c["qlen"]):
            assert bool((lse[b, :, n:] == 0).all()), f"lse: element {b} is not zero at rows >= {n}"


# ---- (c) dropout at the edges ----------------------------------------------------------------------------------------------------------
def keep_of(c, seed):
    return ref.keep_mask(seed, c["bf"], c["heads"], c["nq"], c["nk"], P_DROP, DEV).double() / (1.0 - P_DROP)


@pytest.mark.parametrize("c", kv.wide_cases("dropout"), ids=kv.wide_case_id)
def test_wide_dropout_at_the_tile_boundaries(c):
    """p = 0.25 under the rebuilt hash mask: output and gradients against float64 autograd over dropout(softmax) v, and no gradient
    leaks through dropped entries -- a key that every query of a head drops has dV = 0 exactly in that head."""
    bf, heads, hd, nq, nk = c["bf"], c["heads"], c["hd"], c["nq"], c["nk"]
    label, seed, C = kv.wide_case_id(c), 123457 + nq + nk, heads * hd
    q, kv_, g = inputs(nq * 7 + nk + hd, bf, heads, hd, nq, nk)
    keep = keep_of(c, seed)
    got = train(q, kv_, g, heads, P_DROP, seed)
    same_bits(got, train(q, kv_, g, heads, P_DROP, seed), label + ": two runs")
    check(got, ref.reference(q, kv_, heads, None, None, g, keep=keep), label)
    dead = (keep == 0).all(dim=2)                                          # (bf, heads, nk): no query of the head keeps this key
    dv = got[3][..., C:].reshape(bf, nk, heads, hd).permute(0, 2, 1, 3)    # (bf, heads, nk, hd)
    assert not (dv[dead] != 0).any(), f"{label}: a gradient leaks through dropped entries"
    if nq == 1:
        assert int(dead.sum()) > 0.15 * dead.numel()                       # a quarter of the keys, less sampling noise


# ---- (d) dropout with lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", kv.wide_cases("dropout-lengths"), ids=kv.wide_case_id)
def test_wide_dropout_with_lengths_matches_float64_and_ignores_the_padding(c):
    """The length instantiations with DROP at every width and on both forward forms: the same bits under paddings A and B
    (test_attention_lengths_gpu.padded), the no-grad forward's bits, float64 under the hash mask of the PADDED shape, exact zeros
    beyond the lengths."""
    be = ops.backend()
    bf, heads, hd, nq, nk, qlen, klen = c["bf"], c["heads"], c["hd"], c["nq"], c["nk"], c["qlen"], c["klen"]
    label, seed = kv.wide_case_id(c), 424243
    ql_t, kl_t = lens_of(c)
    keep = keep_of(c, seed)
    got = {}
    for filling in ("A", "B"):
        q, kv_, g = padded(bf, heads, hd, nq, nk, qlen, klen, filling)
        got[filling] = train(q, kv_, g, heads, P_DROP, seed, ql_t, kl_t)
        same_bits(got[filling], train(q, kv_, g, heads, P_DROP, seed, ql_t, kl_t), f"{label} {filling}: two runs")
        with torch.no_grad():
            assert torch.equal(be._attention_lengths(q, kv_, heads, hd ** -0.5, P_DROP, seed, ql_t, kl_t), got[filling][0]), "the no-grad forward differs"
    same_bits(got["A"], got["B"], label + ": the padding's content moved a result")
    out, lse, gq, gkv = got["A"]
    check(got["A"], ref.reference(q, kv_, heads, qlen, klen, g, keep=keep), label)
    assert_zero_beyond(out, qlen, "out")
    assert_zero_beyond(gq, qlen, "grad_q")
    assert_zero_beyond(gkv, klen, "grad_kv")
    for b in range(bf):
        assert bool((lse[b, :, qlen[b]:] == 0).all()), f"lse: element {b} is not zero at rows >= {qlen[b]}"
        if klen[b] == 0:
            assert bool((out[b] == 0).all()) and bool((lse[b] == 0).all()) and bool((gq[b] == 0).all()), f"element {b} has no keys"
        if qlen[b] == 0:
            assert bool((gkv[b] == 0).all()), f"element {b} has no queries"


# ---- (e) strides -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", kv.wide_cases("strides"), ids=kv.wide_case_id)
def test_q_k_v_as_slices_of_one_projection_output(c):
    """q, k, v as the column blocks of one (BF, n, 3C) tensor (all three row strides 3C): the contiguous call's bits."""
    bf, heads, hd, n = c["bf"], c["heads"], c["hd"], c["nq"]
    assert c["nq"] == c["nk"]
    label, C = kv.wide_case_id(c), heads * hd
    qkv, g = rnd(5000 + hd, bf, n, 3 * C).to(DEV), rnd(5001 + hd, bf, n, C).to(DEV)
    q, kv_ = qkv[..., :C].contiguous(), qkv[..., C:].contiguous()
    qlen, klen = lens_of(c)
    p, seed = (P_DROP, 777) if c["drop"] else (0.0, 0)
    packed = c_entries(c, qkv[..., :C], 3 * C, qkv[..., C:2 * C], 3 * C, qkv[..., 2 * C:], 3 * C, g, p, seed, qlen, klen)
    same_bits(packed, kv_entries(c, q, kv_, g, p, seed, qlen, klen), label + ": strided against contiguous")
    keep = keep_of(c, seed) if c["drop"] else None
    check(packed, ref.reference(q, kv_, heads, c["qlen"], c["klen"], g, keep=keep), label)


# ---- (f) large logits at an edge -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", kv.wide_cases("logits"), ids=kv.wide_case_id)
def test_wide_backward_with_large_logits_on_partial_tiles(c):
    """q scaled by 6: logits beyond 12, where exp2(s - L) without the row's statistic would overflow or lose the small terms."""
    bf, heads, hd, nq, nk = c["bf"], c["heads"], c["hd"], c["nq"], c["nk"]
    q, kv_, g = inputs(77 + hd, bf, heads, hd, nq, nk, factor=c["factor"])
    qh = q.double().reshape(bf, nq, heads, hd).permute(0, 2, 1, 3)
    kh = kv_.double().reshape(bf, nk, 2, heads, hd)[:, :, 0].permute(0, 2, 1, 3)
    top = float((qh @ kh.transpose(-2, -1) * hd ** -0.5).max())
    assert top > 12, top
    label = f"{kv.wide_case_id(c)},logits<={top:.1f}"
    got = train(q, kv_, g, heads)
    same_bits(got, train(q, kv_, g, heads), label + ": two runs")
    check(got, ref.reference(q, kv_, heads, None, None, g), label)
