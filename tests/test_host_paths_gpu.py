"""-m gpu: the Python wrappers of PointConv and of the attention reach the library through the `_lengths` entries alone, with null
lengths when the caller passes none (mocopci_amd/ops.py).  Null lengths are the dense entries themselves, so a wrapper called without
lengths must give the bits of the raw dense C entry called directly -- on every form of the dispatch: the two low-level PointConv
kernels and the streaming one (b * s = 16422, just over the 16384 threshold), the fused Linear, the backward, the narrow and the wide
attention heads and both sides of the key-split rule at head width 256, and the key / value rotation.  Every comparison is
torch.equal."""
import ctypes

import pytest
import torch

from mocopci_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_SRC, K = 64, 32


def P(t, offset_floats=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset_floats)


def stream():
    return torch.cuda.current_stream().cuda_stream


def pointconv_inputs(b, s, d, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, scale=1.0: ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)
    s_xyz, new_xyz, s_points = r(b, N_SRC, 3), r(b, s, 3), r(b, N_SRC, d)
    idx = torch.randint(0, N_SRC, (b, s, K), generator=g, dtype=torch.int32).to(DEV)
    weights = [r(8, 3, scale=0.8), r(8, scale=0.3), r(8, 8, scale=0.6), r(8, scale=0.3), r(8, 8, scale=0.6), r(8, scale=0.3)]
    return s_xyz, new_xyz, s_points, idx, weights, r


@pytest.mark.parametrize("b,s,d", [(3, 77, 32), (2, 40, 256), (2, 8211, 32)], ids=["lowlevel256", "lowlevel1024", "stream"])
def test_pointconv_agg_without_lengths_is_the_dense_entry(b, s, d):
    s_xyz, new_xyz, s_points, idx, weights, _ = pointconv_inputs(b, s, d, seed=11 * d + s)
    got = ops.backend().pointconv_agg(s_xyz, new_xyz, s_points, idx, *weights)
    want = torch.empty((b, s, (d + 3) * 8), dtype=torch.float32, device=DEV)
    rc = _lib.load().mcp_pointconv_agg(b, N_SRC, s, d, K, P(s_xyz), P(new_xyz), P(s_points), P(idx), *(P(w) for w in weights), P(want), stream())
    assert rc == 0
    assert torch.equal(got, want)


def test_pointconv_linear_without_lengths_is_the_dense_entry():
    b, s, d = 3, 77, 32
    be = ops.backend()
    s_xyz, new_xyz, s_points, idx, weights, r = pointconv_inputs(b, s, d, seed=5)
    w, bias = r(d, (d + 3) * 8, scale=0.05), r(d, scale=0.5)
    packed = be.pointconv_linear_pack(w, bias)
    got = be.pointconv_linear(s_xyz, new_xyz, s_points, idx, *weights, w, bias, 0.1, packed=packed)
    want = torch.empty((b, s, d), dtype=torch.float32, device=DEV)
    rc = _lib.load().mcp_pointconv_linear(b, N_SRC, s, d, K, P(s_xyz), P(new_xyz), P(s_points), P(idx), *(P(t) for t in weights), P(packed), d, 0.1,
                                          P(want), stream())
    assert rc == 0
    assert torch.equal(got, want)


def test_pointconv_agg_gradients_without_lengths_are_the_dense_entrys():
    b, s, d = 3, 77, 32
    lib = _lib.load()
    s_xyz, new_xyz, s_points, idx, weights, r = pointconv_inputs(b, s, d, seed=23)
    gout = r(b, s, (d + 3) * 8)
    leaves = [t.clone().requires_grad_(True) for t in (new_xyz, *weights)]
    out = ops.backend().pointconv_agg(s_xyz, leaves[0], s_points, idx, *leaves[1:])
    got = torch.autograd.grad(out, leaves, gout)
    d_new = torch.empty_like(new_xyz)
    d_gxyz = torch.empty((b, s, K, 3), dtype=torch.float32, device=DEV)
    d_rows = torch.empty((b, s, K, d), dtype=torch.float32, device=DEV)
    d_w = torch.empty((lib.mcp_pointconv_agg_grad_floats(),), dtype=torch.float32, device=DEV)
    need = lib.mcp_pointconv_agg_grad_workspace_bytes(b, s)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    rc = lib.mcp_pointconv_agg_grad(b, N_SRC, s, d, K, P(s_xyz), P(new_xyz), P(s_points), P(idx), *(P(t) for t in weights), P(gout), P(d_new), P(d_gxyz),
                                    P(d_rows), P(d_w), P(ws), need, stream())
    assert rc == 0
    assert torch.equal(got[0], d_new)
    at = 0
    for name, w, gw in zip(("w0", "b0", "w1", "b1", "w2", "b2"), weights, got[1:]):
        assert torch.equal(gw, d_w[at:at + w.numel()].view(w.shape)), name
        at += w.numel()
    assert at == d_w.numel()


def attention_inputs(heads, hd, bf, nq, nk, seed):
    g = torch.Generator().manual_seed(seed)
    C = heads * hd
    return torch.randn(bf, nq, C, generator=g).to(DEV), torch.randn(bf, nk, 2 * C, generator=g).to(DEV)


# the last two: the pair on either side of the key-split rule at head width 256 (tests/test_attention_lengths_gpu.py)
@pytest.mark.parametrize("heads,hd,bf,nq,nk", [(2, 8, 2, 70, 45), (2, 32, 2, 70, 45), (3, 256, 2, 130, 100), (3, 256, 2, 100, 333)])
def test_attention_without_lengths_is_the_dense_entry(heads, hd, bf, nq, nk):
    q, kv = attention_inputs(heads, hd, bf, nq, nk, seed=hd + nq)
    C = heads * hd
    got = ops.backend().attention(q, kv, heads)
    want = torch.empty_like(q)
    entry = getattr(_lib.load(), "mcp_attention_small" if hd in (8, 16) else "mcp_attention_wide")
    rc = entry(bf, nq, nk, heads, hd, P(q), C, P(kv), 2 * C, P(kv, C), 2 * C, hd ** -0.5, P(want), C, stream())
    assert rc == 0
    assert torch.equal(got, want)


def test_attention_rot_without_lengths_is_the_dense_entry():
    heads, hd, bf, nq, nk = 2, 8, 2, 70, 45
    q, kv = attention_inputs(heads, hd, bf, nq, nk, seed=3)
    C = heads * hd
    k, v = kv[:, :, :C], kv[:, :, C:]
    got = ops.backend().attention_rot(q, k, v, heads, kv_shift=1)
    want = torch.empty_like(q)
    rc = _lib.load().mcp_attention(bf, nq, nk, heads, hd, P(q), C, P(kv), 2 * C, P(kv, C), 2 * C, 1, hd ** -0.5, P(want), C, stream())
    assert rc == 0
    assert torch.equal(got, want)
    assert not torch.equal(got, ops.backend().attention(q, kv, heads))   # the rotation is seen: element b reads the keys of element b + 1
