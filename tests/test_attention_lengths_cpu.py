"""-m "not gpu": the host side of the length-aware attention -- the float64 helper the GPU tests compare against
(tests/attention_lengths_reference.py) is itself checked against torch.softmax on each element's sliced prefixes, host lengths are
rejected through HipBackend.attention before anything is launched, and the five new entry points are declared, bound and validate
their arguments without a device."""
import os
import re

import pytest
import torch

from mocopci_amd import _lib, grad, ops
from tests import attention_lengths_reference as ref
from tests import test_lengths_cpu as base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcp_attention_lengths", "mcp_attention_small_lse_lengths", "mcp_attention_wide_lse_lengths",
       "mcp_attention_small_grad_lse_lengths", "mcp_attention_wide_grad_lse_lengths")
# the bad host forms of tests/test_lengths_cpu.py (for a batch of 2 and a limit of 10), not a copy of them
BAD_HOST_LENGTHS = next(m for m in base.test_host_lengths_are_validated.pytestmark if m.name == "parametrize").args[1]


def rnd(seed, *shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def padded_case(fill):
    bf, heads, hd, nq, nk = 4, 2, 8, 9, 7
    C = heads * hd
    q, kv, g = rnd(1, bf, nq, C), rnd(2, bf, nk, 2 * C), rnd(3, bf, nq, C)
    qlen, klen = [9, 4, 0, 5], [7, 3, 5, 0]
    for b in range(bf):
        q[b, qlen[b]:] = fill
        g[b, qlen[b]:] = fill
        kv[b, klen[b]:] = fill
    return bf, heads, hd, nq, nk, q, kv, g, qlen, klen


@pytest.mark.parametrize("fill", [float("nan"), float("inf"), 1e30])
def test_helper_live_rows_are_softmax_on_the_sliced_prefixes_and_the_rest_is_zero(fill):
    bf, heads, hd, nq, nk, q, kv, g, qlen, klen = padded_case(fill)
    C = heads * hd
    out, lse, gq, gkv = ref.reference(q, kv, heads, qlen, klen, g)
    assert all(bool(torch.isfinite(t).all()) for t in (out, lse, gq, gkv))
    for b in range(bf):
        a, c = qlen[b], klen[b]
        assert bool((out[b, a:] == 0).all()) and bool((lse[b, :, a:] == 0).all()) and bool((gq[b, a:] == 0).all()) and bool((gkv[b, c:] == 0).all())
        if a == 0 or c == 0:
            assert bool((out[b] == 0).all()) and bool((lse[b] == 0).all()) and bool((gq[b] == 0).all()) and bool((gkv[b] == 0).all())
            continue
        qs = q[b, :a].clone().requires_grad_(True)
        kvs = kv[b, :c].clone().requires_grad_(True)
        qh = qs.reshape(a, heads, hd).permute(1, 0, 2)
        kh, vh = (kvs[:, i * C:(i + 1) * C].reshape(c, heads, hd).permute(1, 0, 2) for i in (0, 1))
        s = qh @ kh.transpose(-1, -2) * hd ** -0.5
        want = (torch.softmax(s, dim=-1) @ vh).permute(1, 0, 2).reshape(a, C)
        wq, wkv = torch.autograd.grad(want, (qs, kvs), g[b, :a])
        torch.testing.assert_close(out[b, :a], want.detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(lse[b, :, :a], torch.logsumexp(s, dim=-1).detach() / ref.LN2, rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(gq[b, :a], wq, rtol=1e-11, atol=1e-13)
        torch.testing.assert_close(gkv[b, :c], wkv, rtol=1e-11, atol=1e-13)


def test_helper_rotation_reads_the_rotated_elements_length_and_the_ratio_tells_a_wrong_key_count():
    bf, heads, hd, nq, nk, q, kv, g, qlen, klen = padded_case(float("nan"))
    k, v = ref.split_kv(kv)
    out, _ = ref.masked_attention(q, k, v, heads, qlen, klen, kv_shift=1)
    for b in range(bf):
        src = (b + 1) % bf
        one, _ = ref.masked_attention(q[b:b + 1], k[src:src + 1], v[src:src + 1], heads, qlen[b:b + 1], klen[src:src + 1])
        assert torch.equal(out[b], one[0])
    # the error ratio: 0 for the reference itself, far above 1 when one key too many is attended to
    exact, _ = ref.masked_attention(q, k, v, heads, qlen, klen)
    assert ref.forward_ratio(exact, q, k, v, heads, qlen, klen) == 0.0
    finite = torch.nan_to_num(kv, nan=0.5, posinf=0.5)
    wrong, _ = ref.masked_attention(q, *ref.split_kv(finite), heads, qlen, [min(c + 1, nk) for c in klen])
    assert ref.forward_ratio(wrong, q, k, v, heads, qlen, klen) > 100.0


def test_dense_twin_for_other_head_widths_has_the_same_semantics():
    bf, heads, hd, nq, nk, q, kv, g, qlen, klen = padded_case(float("nan"))
    want, _, wq, wkv = ref.reference(q, kv, heads, qlen, klen, g)
    ql, kvl = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    got = grad.attention_lengths_twin(ql, kvl, heads, hd ** -0.5, torch.tensor(qlen), torch.tensor(klen))
    gq, gkv = torch.autograd.grad(got, (ql, kvl), g)   # NaN in the padded rows of grad_out
    torch.testing.assert_close(got.detach(), want, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(gq, wq, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(gkv, wkv, rtol=1e-11, atol=1e-13)
    # device lengths out of range are clamped, None is full
    full = grad.attention_lengths_twin(q[:1], kv[:1], heads, hd ** -0.5, torch.tensor([nq + 7]), None)
    torch.testing.assert_close(full, grad.attention_twin(q[:1], kv[:1], heads, hd ** -0.5), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("side", ["query_lengths", "key_lengths"])
@pytest.mark.parametrize("bad", BAD_HOST_LENGTHS)
def test_bad_host_lengths_are_rejected_through_attention_before_any_launch(bad, side):
    # q, kv on the CPU and no backend object: the call must raise in lengths_tensor, before it looks at either
    q, kv = torch.zeros(2, 10, 16), torch.zeros(2, 10, 32)
    with pytest.raises(RuntimeError, match="lengths"):
        ops.HipBackend.attention(object(), q, kv, 2, **{side: bad})
    # a head width no kernel is built for takes the dense formulation: the same validation in front of it
    with pytest.raises(RuntimeError, match="lengths"):
        ops.HipBackend.attention(object(), q, kv, 4, **{side: bad})


def declared_parameters(name):
    text = open(os.path.join(ROOT, "include", "mocopci_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, f"{name} is not declared in include/mocopci_hip.h"
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_bound_and_exported_with_matching_argument_counts(name):
    params = declared_parameters(name)
    assert len(params) == len(_lib.SIGNATURES[name]), (name, len(params), len(_lib.SIGNATURES[name]))
    assert params[-1] == "mcp_stream_t stream" and "const int *qlen" in params and "const int *klen" in params
    plain = name[:-len("_lengths")]
    assert len(params) == len(declared_parameters(plain)) + 2
    assert hasattr(_lib.load(), name), f"{name} is not exported"


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    p = 16   # any non-null, 16-byte aligned address: nothing is launched
    BAD, UNSUPPORTED = 10001, 10002
    fwd = lambda hd, q=p, ql=p, kl=p, bf=1: lib.mcp_attention_lengths(bf, 1, 1, 1, hd, q, hd, p, hd, p, hd, 0, 1.0, ql, kl, p, hd, None)
    for hd in (8, 16, 32, 64, 256):
        assert fwd(hd, q=p + 4) == BAD          # float4 row traffic
        assert fwd(hd, ql=p + 2) == BAD         # int32 lengths
        assert fwd(hd, q=None) == BAD
        assert fwd(hd, bf=0) == BAD
        assert fwd(hd, q=p + 4, ql=None, kl=None) == BAD    # both null: mcp_attention, and so are its errors
    assert fwd(128) == UNSUPPORTED and fwd(128, ql=None, kl=None) == UNSUPPORTED and fwd(4) == UNSUPPORTED
    for fam, ok, other in (("small", 8, 32), ("wide", 32, 8)):
        lse = getattr(lib, f"mcp_attention_{fam}_lse_lengths")
        bwd = getattr(lib, f"mcp_attention_{fam}_grad_lse_lengths")
        f = lambda hd, q=p, ql=p, kl=p: lse(1, 1, 1, 1, hd, q, hd, p, hd, p, hd, 1.0, 0.0, 0, p, None, ql, kl, None)
        b = lambda hd, q=p, ql=p, kl=p, ws=1 << 20: bwd(1, 1, 1, 1, hd, q, hd, p, hd, p, hd, 1.0, 0.0, 0, p, p, p, p, p, p, ws, ql, kl, None)
        for call in (f, b):
            assert call(other) == UNSUPPORTED and call(128) == UNSUPPORTED
            assert call(other, ql=None, kl=None) == UNSUPPORTED
            assert call(ok, q=p + 4) == BAD and call(ok, q=p + 4, kl=None) == BAD and call(ok, q=p + 4, ql=None, kl=None) == BAD
            assert call(ok, kl=p + 1) == BAD
        assert b(ok, ws=0) == BAD               # workspace too small
