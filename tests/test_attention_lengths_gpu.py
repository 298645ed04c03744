"""-m gpu: attention over a padded batch with per-element query and key lengths (HipBackend.attention / attention_rot with
query_lengths / key_lengths; mcp_attention_lengths, mcp_attention_{small,wide}_lse_lengths, mcp_attention_{small,wide}_grad_lse_lengths).

Every padded tensor is built twice with the same live part and two paddings -- A: padded k rows are copies of live q rows of the same
head times 50 (an unmasked key wins every softmax), padded v is 1e30; B: padded k is -5e29, padded v is inf; padded q and grad_out are
NaN in both -- and every result must be the same bits under both.

Criteria.  Forward, live rows: the float64 masked dense formulation (tests/attention_lengths_reference.py) within the project's bound
for the attention kernels with the element's own key count, C_ATTN 2^-24 (sqrt(kl) + S) (P @ |V|), i.e. ratio <= 1.  Head widths 8 - 64:
live rows are also the plain call on the element's sliced, contiguous prefixes bit for bit (the key loop order does not depend on the
batch).  Head width 256: whether the keys are split over the waves is decided from the PADDED batch (wide_keys_split), so a short
element may run the key-split form where its own slice alone would not (or the other way round) and the merge order differs: there the
float64 bound is the criterion.  Padded rows and elements without keys are exact zeros.  lse: rtol = atol = 1e-5 against float64 (the
figures of tests/test_attention_wide_grad_gpu.py).  Gradients: 1e-4 max|f64| + 1e-6 per tensor, exact zeros beyond the lengths.
Lines starting with MEASURED carry the largest error ratios per family (profiles/attention_lengths_accuracy.txt)."""
import ctypes

import pytest
import torch

from mocopci_amd import _lib, ops
from tests import attention_lengths_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WAVES = 4


def wide_keys_split(bf, nq, nk, heads):
    """csrc/attention_wide_fwd.h: wide_keys_split, restated."""
    return -(-nq // (32 * WAVES)) * heads * bf * WAVES < 1024 and nk >= 32 * WAVES


def rnd(seed, *shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


_CASES = {}


def padded(bf, heads, hd, nq, nk, qlen, klen, filling):
    """(q, kv, grad_out) on the device: the same live part for both fillings, the padding as the module's docstring says."""
    key = (bf, heads, hd, nq, nk, tuple(qlen), tuple(klen), filling)
    if key not in _CASES:
        C = heads * hd
        q, kv, g = rnd(11, bf, nq, C), rnd(12, bf, nk, 2 * C), rnd(13, bf, nq, C)
        for b in range(bf):
            a, c = qlen[b], klen[b]
            if c < nk:
                if filling == "A":
                    src = q[b, :a] if a > 0 else rnd(14, 1, C)
                    kv[b, c:, :C] = 50.0 * src[torch.arange(nk - c) % src.shape[0]]
                    kv[b, c:, C:] = 1e30
                else:
                    kv[b, c:, :C] = -5e29
                    kv[b, c:, C:] = float("inf")
            q[b, a:] = float("nan")
            g[b, a:] = float("nan")
        _CASES[key] = tuple(t.to(DEV) for t in (q, kv, g))
    return _CASES[key]


def assert_zero_beyond(t, lens, what):
    for b, n in enumerate(lens):
        assert bool((t[b, n:] == 0).all()), f"{what}: element {b} is not zero at rows >= {n}"


# ---- forward -------------------------------------------------------------------------------------------------------------------------
NARROW = [(4, 2, hd, 200, 130, ql, kl) for hd in (8, 16) for kl in ((0, 1, 31, 130), (32, 33, 63, 64), (65, 127, 128, 129))
          for ql in ((0, 1, 200, 33), (32, 127, 128, 129))]
WIDE = [(3, 2, hd, 130, 100, ql, kl) for hd in (32, 64) for kl in ((0, 1, 100), (31, 32, 33), (64, 65, 96)) for ql in ((0, 1, 130), (32, 33, 129))]
WIDE256_QS = [(2, 3, 256, 130, 100, (130, 5), (0, 37))]
# key split: kl <= 32 leaves three waves without a stage, kl = 0 all four, 129 / 333 / 96 / 33 give the waves unequal stage counts
WIDE256_SPLIT = [(2, 1, 256, 37, 130, (37, 1), (0, 129)), (2, 1, 256, 37, 130, (0, 33), (31, 130)),
                 (2, 3, 256, 100, 333, (33, 100), (1, 333)), (2, 3, 256, 100, 333, (100, 1), (127, 96)),
                 (2, 3, 256, 256, 160, (256, 33), (33, 128)), (2, 3, 256, 256, 160, (1, 0), (160, 0))]
FORWARD = NARROW + WIDE + WIDE256_QS + WIDE256_SPLIT
case_id = lambda c: f"hd{c[2]}-{c[0]}x{c[1]}-{c[3]}q{c[4]}k-ql{'_'.join(map(str, c[5]))}-kl{'_'.join(map(str, c[6]))}"


@pytest.mark.parametrize("case", FORWARD, ids=case_id)
def test_forward_live_rows_match_float64_and_the_sliced_call_padding_is_zero(case):
    bf, heads, hd, nq, nk, qlen, klen = case
    if case in WIDE256_SPLIT:
        assert wide_keys_split(bf, nq, nk, heads), "the padded shape must take the key-split kernel"
    elif hd == 256:
        assert not wide_keys_split(bf, nq, nk, heads)
    be = ops.backend()
    C = heads * hd
    results = {}
    for filling in ("A", "B"):
        q, kv, _ = padded(bf, heads, hd, nq, nk, qlen, klen, filling)
        with torch.no_grad():
            inf = be.attention(q, kv, heads, query_lengths=list(qlen), key_lengths=list(klen))     # the inference entry
            inf2 = be.attention(q, kv, heads, query_lengths=list(qlen), key_lengths=list(klen))
        ql_, kvl_ = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        trn = be.attention(ql_, kvl_, heads, query_lengths=list(qlen), key_lengths=list(klen)).detach()   # the training forward
        results[filling] = (inf, trn)
        assert torch.equal(inf, inf2), "two runs differ"
        for name, out in (("inference", inf), ("training", trn)):
            assert bool(torch.isfinite(out).all()), f"{name} {filling}: not finite"
            assert_zero_beyond(out, qlen, f"{name} {filling}")
            for b in range(bf):
                if klen[b] == 0:
                    assert bool((out[b] == 0).all()), f"{name} {filling}: element {b} has no keys and is not zero"
            ratio = ref.forward_ratio(out, q, kv[..., :C], kv[..., C:], heads, qlen, klen)
            print(f"MEASURED forward {name} {case_id(case)} filling {filling}: ratio {ratio:.3f}")
            assert ratio <= 1.0, f"{name} {filling}: error {ratio:.2f} x the bound"
        if hd != 256:
            for b in range(bf):
                a, c = qlen[b], klen[b]
                if a == 0 or c == 0:
                    continue
                qs, kvs = q[b:b + 1, :a].contiguous(), kv[b:b + 1, :c].contiguous()
                with torch.no_grad():
                    assert torch.equal(inf[b, :a], be.attention(qs, kvs, heads)[0]), f"inference: element {b} differs from its sliced call"
                assert torch.equal(trn[b, :a], be.attention(qs.requires_grad_(True), kvs, heads).detach()[0]), f"training: element {b}"
    for x, y in zip(results["A"], results["B"]):
        assert torch.equal(x, y), "the padding's content moved the output"


@pytest.mark.parametrize("heads,hd,bf,nq,nk", [(2, 8, 4, 200, 130), (2, 16, 4, 200, 130), (2, 32, 3, 130, 100), (2, 64, 3, 130, 100),
                                               (3, 256, 2, 130, 100), (3, 256, 2, 100, 333)], ids=lambda v: str(v))
def test_full_lengths_and_none_are_the_plain_call(heads, hd, bf, nq, nk):
    be = ops.backend()
    C = heads * hd
    q, kv, g = rnd(21, bf, nq, C).to(DEV), rnd(22, bf, nk, 2 * C).to(DEV), rnd(23, bf, nq, C).to(DEV)
    full = dict(query_lengths=[nq] * bf, key_lengths=[nk] * bf)
    with torch.no_grad():
        plain = be.attention(q, kv, heads)
        assert torch.equal(be.attention(q, kv, heads, **full), plain)
        assert torch.equal(be.attention(q, kv, heads, query_lengths=None, key_lengths=None), plain)
        assert torch.equal(be.attention(q, kv, heads, key_lengths=[nk] * bf), plain)
        k, v = kv[..., :C], kv[..., C:]
        assert torch.equal(be.attention_rot(q, k, v, heads, 1, **full), be.attention_rot(q, k, v, heads, 1))

    def grads(**kw):
        leaves = [t.clone().requires_grad_(True) for t in (q, kv)]
        out = be.attention(*leaves, heads, **kw)
        return (out.detach(),) + torch.autograd.grad(out, leaves, g)
    for a, b in zip(grads(**full), grads()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("hd,heads", [(8, 2), (256, 1)])
@pytest.mark.parametrize("shift", [1, 2])
def test_rotation_reads_the_length_of_the_rotated_element(hd, heads, shift):
    be = ops.backend()
    bf, nq, nk, C = 3, 70, 130, heads * hd
    qlen, klen = (70, 33, 1), (130, 31, 65)
    for filling in ("A", "B"):
        q, kv, _ = padded(bf, heads, hd, nq, nk, qlen, klen, filling)
        k, v = kv[..., :C], kv[..., C:]
        out = be.attention_rot(q, k, v, heads, shift, query_lengths=list(qlen), key_lengths=list(klen))
        assert bool(torch.isfinite(out).all())
        assert_zero_beyond(out, qlen, "rotation")
        ratio = ref.forward_ratio(out, q, k, v, heads, qlen, klen, kv_shift=shift)
        print(f"MEASURED forward rotation hd{hd} shift {shift} filling {filling}: ratio {ratio:.3f}")
        assert ratio <= 1.0
        # the wrong element's length would not pass: the same check with the lengths left unrotated
        unrot = torch.roll(torch.tensor(klen), shift).tolist()
        assert not ref.forward_ratio(out, q, k, v, heads, qlen, unrot, kv_shift=shift) <= 1.0


@pytest.mark.parametrize("hd,heads", [(8, 2), (32, 2), (256, 1)])
def test_device_lengths_cause_no_synchronisation_and_are_clamped(hd, heads):
    be = ops.backend()
    bf, nq, nk, C = 2, 70, 130, heads * hd
    q, kv, g = padded(bf, heads, hd, nq, nk, (70, 33), (0, 130), "A")
    dq_len = torch.tensor([nq + 9, 33], dtype=torch.int32, device=DEV)
    dk_len = torch.tensor([-3, nk + 7], dtype=torch.int64, device=DEV)
    ql_, kvl_ = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            dev_out = be.attention(q, kv, heads, query_lengths=dq_len, key_lengths=dk_len)
            host_out = be.attention(q, kv, heads, query_lengths=[70, 33], key_lengths=[0, 130])
            rot = be.attention_rot(q, kv[..., :C], kv[..., C:], heads, 1, query_lengths=dq_len, key_lengths=dk_len)
        trn = be.attention(ql_, kvl_, heads, query_lengths=dq_len, key_lengths=dk_len)
        gq, gkv = torch.autograd.grad(trn, (ql_, kvl_), g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(dev_out, host_out) and torch.equal(trn.detach(), host_out)
    assert bool((host_out[0] == 0).all()) and bool(torch.isfinite(rot).all()) and bool(torch.isfinite(gq).all()) and bool(torch.isfinite(gkv).all())
    assert ref.forward_ratio(rot, q, kv[..., :C], kv[..., C:], heads, (70, 33), (0, 130), kv_shift=1) <= 1.0


# ---- lse through the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [NARROW[0], NARROW[5], WIDE[0], WIDE[3], WIDE256_QS[0], WIDE256_SPLIT[0], WIDE256_SPLIT[2]], ids=case_id)
def test_lse_live_rows_match_float64_and_padded_rows_are_zero(case):
    bf, heads, hd, nq, nk, qlen, klen = case
    lib = _lib.load()
    C, scale = heads * hd, hd ** -0.5
    q, kv, _ = padded(bf, heads, hd, nq, nk, qlen, klen, "B")
    ql_t, kl_t = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in (qlen, klen))
    out, lse = torch.full_like(q, float("nan")), torch.full((bf, heads, nq), float("nan"), device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    fn = lib.mcp_attention_small_lse_lengths if hd in (8, 16) else lib.mcp_attention_wide_lse_lengths
    st = torch.cuda.current_stream().cuda_stream
    assert fn(bf, nq, nk, heads, hd, P(q), C, P(kv), 2 * C, ctypes.c_void_p(kv.data_ptr() + 4 * C), 2 * C, scale, 0.0, 0, P(out), P(lse), P(ql_t), P(kl_t),
              st) == 0
    _, want, _, _ = ref.reference(q, kv, heads, qlen, klen)
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(out).all())
    for b in range(bf):
        assert bool((lse[b, :, qlen[b]:] == 0).all()), f"element {b}: lse of padded rows"
        if klen[b] == 0:
            assert bool((lse[b] == 0).all())
    print(f"\nlse: max|f64| {float(want.abs().max()):.3e}  |hip - f64| {float((lse.double() - want).abs().max()):.3e}")
    torch.testing.assert_close(lse.double(), want, rtol=1e-5, atol=1e-5)
    # lse may be NULL: the same output
    out2 = torch.full_like(q, float("nan"))
    assert fn(bf, nq, nk, heads, hd, P(q), C, P(kv), 2 * C, ctypes.c_void_p(kv.data_ptr() + 4 * C), 2 * C, scale, 0.0, 0, P(out2), None, P(ql_t), P(kl_t),
              st) == 0
    assert torch.equal(out, out2)


# ---- gradients ---------------------------------------------------------------------------------------------------------------------------
GRADS = [(4, 2, 8, 200, 130, (33, 0, 200, 1), (0, 1, 31, 130)), (4, 2, 16, 200, 130, (127, 129, 0, 64), (65, 0, 128, 63)),
         (3, 2, 32, 130, 100, (129, 0, 31), (0, 33, 100)), (3, 2, 64, 130, 100, (0, 33, 130), (31, 0, 65)),
         (2, 3, 256, 130, 100, (130, 5), (0, 37)), (2, 3, 256, 130, 100, (0, 129), (33, 100)),
         (2, 3, 256, 100, 333, (33, 100), (0, 129)), (2, 3, 256, 100, 333, (0, 1), (127, 333))]


@pytest.mark.parametrize("case", GRADS, ids=case_id)
def test_gradients_match_float64_are_zero_beyond_the_lengths_and_ignore_the_padding(case):
    bf, heads, hd, nq, nk, qlen, klen = case
    be = ops.backend()
    got = {}
    for filling in ("A", "B"):
        q, kv, g = padded(bf, heads, hd, nq, nk, qlen, klen, filling)

        def run():
            leaves = [t.clone().requires_grad_(True) for t in (q, kv)]
            out = be.attention(*leaves, heads, query_lengths=list(qlen), key_lengths=list(klen))
            return torch.autograd.grad(out, leaves, g)
        got[filling] = run()
        for a, b in zip(got[filling], run()):
            assert torch.equal(a, b), "two runs differ"
    for a, b in zip(got["A"], got["B"]):
        assert torch.equal(a, b), "the padding's content moved a gradient"
    gq, gkv = got["A"]
    _, _, wq, wkv = ref.reference(q, kv, heads, qlen, klen, g)
    assert bool(torch.isfinite(gq).all()) and bool(torch.isfinite(gkv).all()), "a gradient is not finite"
    assert_zero_beyond(gq, qlen, "grad_q")
    assert_zero_beyond(gkv, klen, "grad_kv")
    for b in range(bf):
        if klen[b] == 0:
            assert bool((gq[b] == 0).all()), f"grad_q of element {b} (no keys)"
        if qlen[b] == 0:
            assert bool((gkv[b] == 0).all()), f"grad_kv of element {b} (no queries)"
    failures = []
    for name, a, w in (("q", gq, wq), ("kv", gkv, wkv)):
        err, bound = float((a.double() - w).abs().max()), ref.grad_bound(w)
        print(f"MEASURED grad {name} {case_id(case)}: max|f64| {float(w.abs().max()):.3e} |hip - f64| {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        if not err <= bound:
            failures.append(f"grad {name}: {err:.2e} > {bound:.2e}")
    assert not failures, "; ".join(failures)


# ---- dropout -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(4, 2, 8, 200, 130, (33, 0, 200, 129), (65, 130, 31, 0)), (3, 2, 32, 130, 100, (129, 0, 33), (0, 33, 100))], ids=case_id)
def test_dropout_matches_the_dense_formulation_under_the_hash_mask_of_the_padded_shape(case):
    bf, heads, hd, nq, nk, qlen, klen = case
    be = ops.backend()
    p, seed = 0.3, 424243
    q, kv, g = padded(bf, heads, hd, nq, nk, qlen, klen, "A")
    keep = ref.keep_mask(seed, bf, heads, nq, nk, p, DEV).double() / (1.0 - p)
    want, _, wq, wkv = ref.reference(q, kv, heads, qlen, klen, g, keep=keep)
    fn = ops._AttentionSmallFn if hd in (8, 16) else ops._AttentionWideFn
    ql_t, kl_t = ops.lengths_tensor(list(qlen), bf, nq, DEV), ops.lengths_tensor(list(klen), bf, nk, DEV)
    leaves = [t.clone().requires_grad_(True) for t in (q, kv)]
    out = fn.apply(be, *leaves, heads, hd ** -0.5, p, seed, ql_t, kl_t)
    gq, gkv = torch.autograd.grad(out, leaves, g)
    assert torch.equal(out.detach(), be._attention_lengths(q, kv, heads, hd ** -0.5, p, seed, ql_t, kl_t)), "the no-grad dropout forward differs"
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gq).all()) and bool(torch.isfinite(gkv).all())
    assert_zero_beyond(out, qlen, "out")
    assert_zero_beyond(gq, qlen, "grad_q")
    assert_zero_beyond(gkv, klen, "grad_kv")
    print(f"\noutput: max|f64| {float(want.abs().max()):.3e}  |hip - f64| {float((out.detach().double() - want).abs().max()):.3e}")
    torch.testing.assert_close(out.detach().double(), want, rtol=1e-4, atol=1e-5)
    for name, a, w in (("q", gq, wq), ("kv", gkv, wkv)):
        err, bound = float((a.double() - w).abs().max()), ref.grad_bound(w)
        print(f"MEASURED dropout grad {name} {case_id(case)}: |hip - f64| {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert err <= bound, f"grad {name}: {err:.2e} > {bound:.2e}"
    # the public call draws its seed from torch's generator, with lengths as without
    torch.manual_seed(5); o1 = be.attention(q, kv, heads, dropout_p=p, query_lengths=list(qlen), key_lengths=list(klen))
    torch.manual_seed(5); o2 = be.attention(q, kv, heads, dropout_p=p, query_lengths=list(qlen), key_lengths=list(klen))
    assert torch.equal(o1, o2)


# ---- other head widths, ABI ------------------------------------------------------------------------------------------------------------
def test_head_widths_without_a_kernel_take_the_dense_masked_formulation():
    be = ops.backend()
    bf, heads, hd, nq, nk = 3, 2, 24, 50, 40
    qlen, klen = (50, 0, 17), (0, 40, 33)
    q, kv, g = padded(bf, heads, hd, nq, nk, qlen, klen, "B")
    leaves = [t.clone().requires_grad_(True) for t in (q, kv)]
    out = be.attention(*leaves, heads, query_lengths=list(qlen), key_lengths=list(klen))
    gq, gkv = torch.autograd.grad(out, leaves, g)
    want, _, wq, wkv = ref.reference(q, kv, heads, qlen, klen, g)
    torch.testing.assert_close(out.detach().double(), want, rtol=1e-4, atol=1e-5)
    assert_zero_beyond(out.detach(), qlen, "out")
    for a, w in ((gq, wq), (gkv, wkv)):
        assert bool(torch.isfinite(a).all()) and float((a.double() - w).abs().max()) <= ref.grad_bound(w)


def test_abi_rejects_what_the_plain_calls_reject_and_accepts_a_single_row():
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    for hd in (8, 32, 256):
        q, kv, g = rnd(31, 1, 1, hd).to(DEV), rnd(32, 1, 1, 2 * hd).to(DEV), rnd(33, 1, 1, hd).to(DEV)
        out, lse = torch.empty_like(q), torch.empty(1, 1, 1, device=DEV)
        args = (1, 1, 1, 1, hd, P(q), hd, P(kv), 2 * hd, P(kv, 4 * hd), 2 * hd)
        assert lib.mcp_attention_lengths(*args, 0, 1.0, P(one), P(one), P(out), hd, st) == 0     # bf * nq = 1
        assert torch.equal(out, kv[:, :, hd:])                                                     # one key: softmax = 1, out = v
        assert lib.mcp_attention_lengths(1, 1, 1, 1, 24, P(q), hd, P(kv), 2 * hd, P(kv, 4 * hd), 2 * hd, 0, 1.0, P(one), P(one), P(out), hd, st) == 10002
        assert lib.mcp_attention_lengths(1, 1, 1, 1, hd, P(q, 4), hd, P(kv), 2 * hd, P(kv, 4 * hd), 2 * hd, 0, 1.0, P(one), P(one), P(out), hd, st) == 10001
        assert lib.mcp_attention_lengths(*args, 1, 1.0, P(one), P(one), P(out), hd, st) == 10001   # rotation out of range
        fam = "small" if hd == 8 else "wide"
        fwd, bwd = getattr(lib, f"mcp_attention_{fam}_lse_lengths"), getattr(lib, f"mcp_attention_{fam}_grad_lse_lengths")
        out2 = torch.empty_like(q)
        assert fwd(*args, 1.0, 0.0, 0, P(out2), P(lse), P(one), None, st) == 0
        assert torch.equal(out2, out)
        need = lib.mcp_attention_small_grad_workspace_bytes(1, 1, 1) if hd == 8 else lib.mcp_attention_wide_grad_workspace_bytes(1, 1, 1, 1, hd)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
        gq, gkv = torch.empty_like(q), torch.empty_like(kv)
        assert bwd(*args, 1.0, 0.0, 0, P(out2), P(g), P(lse), P(gq), P(gkv), P(ws), need, None, P(one), st) == 0
        torch.cuda.synchronize()
        # one key: p = 1 up to the rounding of exp2(s - L), so dv = dO, dq = dk = 0 to that accuracy
        torch.testing.assert_close(gkv[:, :, hd:], g, rtol=1e-5, atol=1e-6)
        assert float(gq.abs().max()) <= 1e-5 and float(gkv[:, :, :hd].abs().max()) <= 1e-5
        assert bwd(*args, 1.0, 0.0, 0, P(out2), P(g), P(lse), P(gq), P(gkv), P(ws), 0, None, P(one), st) == 10001
        assert fwd(1, 1, 1, 1, 24, P(q), hd, P(kv), 2 * hd, P(kv, 4 * hd), 2 * hd, 1.0, 0.0, 0, P(out2), P(lse), P(one), None, st) == 10002
        assert fwd(1, 1, 1, 1, hd, P(q, 4), hd, P(kv), 2 * hd, P(kv, 4 * hd), 2 * hd, 1.0, 0.0, 0, P(out2), P(lse), P(one), None, st) == 10001
