"""-m gpu: the narrow-head attention backward (csrc/attention_grad.hip: attention_stats_kernel, attention_dq_kernel, attention_dkv_kernel,
head widths 8 and 16) without per-element lengths, at query / key counts on and next to the kernels' own boundaries -- a wave's tile of 32
rows, a workgroup block of 128 (query rows in dq, key rows in dkv), a streamed stage of 64 rows (keys in stats and dq, queries in dkv)
with its double buffer -- against float64 autograd over softmax(q k^T scale) v.  tests/test_attention_lengths_gpu.py walks such edges
through the length instantiations, whose bounds are the lengths inside a fixed launch; here the bounds are the launch's own nq / nk.
kernel_variants.ATTN_GRAD_COUNTS is the grid; test_kernel_variants_cpu.py checks that it holds every boundary class.

The bound is the project's for these kernels (test_grad_gpu.py): max |hip - f64| <= 1e-4 max |f64| + 1e-6 per gradient tensor."""
import ctypes

import pytest
import torch

from mocopci_amd import _lib, ops
from tests import kernel_variants as kv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, HEADS = 2, 2


def rnd(seed, *shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


def dense(q, kv_, hd, keep=None):
    """softmax(q k^T scale) [* keep] v per head on (BF, n, C) / (BF, n, 2C) tensors of any dtype."""
    bf, nq, C = q.shape
    nk, heads = kv_.shape[1], C // hd
    qh = q.reshape(bf, nq, heads, hd).permute(0, 2, 1, 3)
    kvh = kv_.reshape(bf, nk, 2, heads, hd).permute(2, 0, 3, 1, 4)
    p = torch.softmax(qh @ kvh[0].transpose(-2, -1) * hd ** -0.5, dim=-1)
    if keep is not None:
        p = p * keep
    return (p @ kvh[1]).permute(0, 2, 1, 3).reshape(bf, nq, C)


def grads(fn, tensors, g, dt):
    leaves = [t.detach().to(dt).clone().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    return out.detach(), torch.autograd.grad(out, leaves, g.to(dt))


def within_bound(got, want, label):
    for name, a, b in zip(("q", "kv"), got, want):
        assert torch.isfinite(a).all(), f"{label}: grad {name} is not finite"
        scale = float(b.abs().max())
        err = float((a.double() - b).abs().max())
        assert err <= 1e-4 * scale + 1e-6, f"{label}: grad {name}: max err {err:.2e}, gradient scale {scale:.2e}"
    return [float((a.double() - b).abs().max()) / (1e-4 * float(b.abs().max()) + 1e-6) for a, b in zip(got, want)]


def entry_points_agree(q, kv_, g, hd, label):
    """mcp_attention_small_grad (statistics recomputed) and mcp_attention_small_grad_lse (the forward's log-sum-exp): the same bits."""
    lib = _lib.load()
    bf, nq, C = q.shape
    nk, heads = kv_.shape[1], C // hd
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    Pk, Pv = ctypes.c_void_p(kv_.data_ptr()), ctypes.c_void_p(kv_.data_ptr() + 4 * C)
    scale = hd ** -0.5
    out, lse = torch.empty_like(q), torch.empty(bf, heads, nq, device=DEV)
    assert lib.mcp_attention_small_lse(bf, nq, nk, heads, hd, P(q), C, Pk, 2 * C, Pv, 2 * C, scale, 0.0, 0, P(out), P(lse), st) == 0
    need = lib.mcp_attention_small_grad_workspace_bytes(bf, nq, heads)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dq1, dkv1, dq2, dkv2 = torch.empty_like(q), torch.empty_like(kv_), torch.empty_like(q), torch.empty_like(kv_)
    assert lib.mcp_attention_small_grad(bf, nq, nk, heads, hd, P(q), C, Pk, 2 * C, Pv, 2 * C, scale, 0.0, 0, P(out), P(g), P(dq1), P(dkv1), P(ws), need, st) == 0
    assert lib.mcp_attention_small_grad_lse(bf, nq, nk, heads, hd, P(q), C, Pk, 2 * C, Pv, 2 * C, scale, 0.0, 0, P(out), P(g), P(lse), P(dq2), P(dkv2),
                                            P(ws), need, st) == 0
    assert torch.equal(dq1, dq2) and torch.equal(dkv1, dkv2), f"{label}: the two backward entry points differ"
    return dq2, dkv2


@pytest.mark.parametrize("nq", kv.ATTN_GRAD_COUNTS)
@pytest.mark.parametrize("hd", [8, 16])
def test_attention_small_backward_at_the_tile_boundaries(hd, nq):
    """One query count against every key count of the grid."""
    be = ops.backend()
    C = HEADS * hd
    for nk in kv.ATTN_GRAD_COUNTS:
        label = f"hd={hd},nq={nq},nk={nk}"
        seed = 1000 * nq + 10 * nk + hd
        q, kv_, g = rnd(seed, BF, nq, C).to(DEV), rnd(seed + 1, BF, nk, 2 * C).to(DEV), rnd(seed + 2, BF, nq, C).to(DEV)
        _, hip = grads(lambda a, b: be.attention(a, b, HEADS), (q, kv_), g, torch.float32)
        _, again = grads(lambda a, b: be.attention(a, b, HEADS), (q, kv_), g, torch.float32)
        assert torch.equal(hip[0], again[0]) and torch.equal(hip[1], again[1]), f"{label}: not bit-reproducible"
        _, want = grads(lambda a, b: dense(a, b, hd), (q, kv_), g, torch.float64)
        rq, rkv = within_bound(hip, want, label)
        direct = entry_points_agree(q, kv_, g, hd, label)
        within_bound(direct, want, label + " (entry points)")
        print(f"ERR attention_small_grad[{label}] dq={rq:.3f} dkv={rkv:.3f} of the bound")


def keep_mask(bf, heads, nq, nk, p, seed):
    """The kernels' dropout mask (attention_dropout.h: a counter-based hash of seed, row = (batch, head, query), key), as 0 or 1 / (1 - p)."""
    M = 0xFFFFFFFF
    row = torch.arange(bf * heads * nq, device=DEV, dtype=torch.int64).view(bf, heads, nq, 1)
    key = torch.arange(nk, device=DEV, dtype=torch.int64).view(1, 1, 1, nk)
    x = (seed ^ ((row * 0x9E3779B1) & M) ^ ((key * 0x85EBCA77) & M)) & M
    x = x ^ (x >> 16); x = (x * 0x7FEB352D) & M; x = x ^ (x >> 15); x = (x * 0x846CA68B) & M; x = x ^ (x >> 16)
    return (x >= int(p * 4294967296.0)).double() / (1.0 - p)


@pytest.mark.parametrize("nq,nk", [(33, 65), (129, 63), (1, 129), (128, 64)])
@pytest.mark.parametrize("hd", [8, 16])
def test_attention_small_dropout_backward_at_the_tile_boundaries(hd, nq, nk):
    """p = 0.25 under the rebuilt mask: output and gradients against float64 autograd over dropout(softmax) v, and no gradient leaks
    through dropped entries -- a key that every query of a head drops has dV = 0 exactly in that head (dK is not zero there: the
    softmax's normalisation couples the keys, ds = -p D for a dropped entry)."""
    be = ops.backend()
    C, p, seed = HEADS * hd, 0.25, 123457 + nq + nk
    label = f"hd={hd},nq={nq},nk={nk},p={p}"
    q, kv_, g = rnd(nq * 7 + nk, BF, nq, C).to(DEV), rnd(nq * 7 + nk + 1, BF, nk, 2 * C).to(DEV), rnd(nq * 7 + nk + 2, BF, nq, C).to(DEV)
    keep = keep_mask(BF, HEADS, nq, nk, p, seed)
    fn = lambda a, b: ops._AttentionSmallFn.apply(be, a, b, HEADS, hd ** -0.5, p, seed)
    out, hip = grads(fn, (q, kv_), g, torch.float32)
    _, again = grads(fn, (q, kv_), g, torch.float32)
    assert torch.equal(hip[0], again[0]) and torch.equal(hip[1], again[1]), f"{label}: not bit-reproducible"
    want_out, want = grads(lambda a, b: dense(a, b, hd, keep), (q, kv_), g, torch.float64)
    torch.testing.assert_close(out.double(), want_out, rtol=1e-4, atol=1e-5)
    rq, rkv = within_bound(hip, want, label)
    print(f"ERR attention_small_grad[{label}] dq={rq:.3f} dkv={rkv:.3f} of the bound")
    dead = (keep == 0).all(dim=2)                                        # (BF, HEADS, nk): no query of the head keeps this key
    dv = hip[1][..., C:].reshape(BF, nk, HEADS, hd).permute(0, 2, 1, 3)  # (BF, HEADS, nk, hd)
    assert not (dv[dead] != 0).any(), f"{label}: a gradient leaks through dropped entries"
    if nq == 1:
        assert int(dead.sum()) > 0.15 * dead.numel()                     # a quarter of the keys, less sampling noise


@pytest.mark.parametrize("hd", [8, 16])
def test_attention_small_backward_with_large_logits(hd):
    """q scaled by 6: logits beyond 12, where exp2(s - L) without the row's statistic would overflow or lose the small terms."""
    be = ops.backend()
    nq, nk, C = 130, 200, HEADS * hd
    q, kv_, g = (rnd(77 + hd, BF, nq, C) * 6).to(DEV), rnd(78 + hd, BF, nk, 2 * C).to(DEV), rnd(79 + hd, BF, nq, C).to(DEV)
    qh = q.double().reshape(BF, nq, HEADS, hd).permute(0, 2, 1, 3)
    kh = kv_.double().reshape(BF, nk, 2, HEADS, hd)[:, :, 0].permute(0, 2, 1, 3)
    top = float((qh @ kh.transpose(-2, -1) * hd ** -0.5).max())
    assert top > 12, top
    label = f"hd={hd},nq={nq},nk={nk},logits<={top:.1f}"
    _, hip = grads(lambda a, b: be.attention(a, b, HEADS), (q, kv_), g, torch.float32)
    _, again = grads(lambda a, b: be.attention(a, b, HEADS), (q, kv_), g, torch.float32)
    assert torch.equal(hip[0], again[0]) and torch.equal(hip[1], again[1]), f"{label}: not bit-reproducible"
    _, want = grads(lambda a, b: dense(a, b, hd), (q, kv_), g, torch.float64)
    rq, rkv = within_bound(hip, want, label)
    within_bound(entry_points_agree(q, kv_, g, hd, label), want, label + " (entry points)")
    print(f"ERR attention_small_grad[{label}] dq={rq:.3f} dkv={rkv:.3f} of the bound")
