"""Layer-level point-set operators of the hot path on channel-last tensors, backed by
libmocopci_hip.so.  These are the fused counterparts of the reference's Python helpers
(models/m_models/mocopci.py:1130-1266,1456-1502; models/pointconv_util.py:67-192) that the
model harness (mocopci_amd/model.py) is written against.

Layout convention: xyz (B,N,3), features (B,N,C) -- one neighbour = one contiguous row --
instead of the reference's (B,C,N); indices are int32 end to end.

`HipBackend` is the product path.  The harness resolves operators through `backend()` so
that tests and bench.py's cpu_baseline leg can run the SAME graph on the CPU oracle by
calling `set_backend(...)`; nothing in this package imports the oracle, and HipBackend has
no CPU fallback (a CPU tensor raises).
"""
import contextlib
import ctypes
import threading

import torch

from . import _lib, grad

MCP_DIST_EXPANSION = 0
MCP_DIST_DIRECT = 1


_raw_stream = torch._C._cuda_getCurrentRawStream  # (device index) -> hipStream_t of torch's current stream, without the Python
_cur_device = torch._C._cuda_getDevice            # wrappers of torch.cuda.current_stream(): ~10 us per call, 90 calls per step


def _call(name, ref_tensor, *args):
    """One library call on torch's current stream of the tensor's device.  The device guard is taken only when the tensor lives
    on another device than the current one (the guard costs more host time than the launch itself)."""
    fn = getattr(_lib.load(), name)
    idx = ref_tensor.device.index
    if idx is None or idx == _cur_device():
        rc = fn(*args, _raw_stream(_cur_device() if idx is None else idx))
    else:
        with torch.cuda.device(idx):
            rc = fn(*args, _raw_stream(idx))
    if rc:
        _lib.check(rc)


def _opt(t, ptr=_lib.fptr):
    """Device pointer of an optional tensor: NULL for None."""
    return None if t is None else ptr(t)


def _ptr_array(tensors, ptr=_lib.fptr):
    """A host array of device pointers, NULL for None."""
    return (ctypes.c_void_p * len(tensors))(*[_opt(t, ptr) for t in tensors])


def _int_array(values):
    return (ctypes.c_int * len(values))(*values)


def _split_flat(buf, like):
    """A flat buffer cut into consecutive views with the shapes of the tensors of `like`, in their order (the weight gradients a
    backward kernel writes side by side)."""
    pieces, at = [], 0
    for t in like:
        pieces.append(buf[at:at + t.numel()].view(t.shape))
        at += t.numel()
    return pieces


def _two_lists(idx):
    """(ia, ib or None, neighbours per point) of a neighbour list given as the two searches' halves or as one tensor."""
    ia, ib = idx if isinstance(idx, (tuple, list)) else (idx, None)
    return ia, ib, ia.shape[-1] + (0 if ib is None else ib.shape[-1])


def _group_rows_fwd(points, idx):
    B, N, C = points.shape
    idx = idx.contiguous()
    T = idx[0].numel()
    out = torch.empty((*idx.shape, C), dtype=torch.float32, device=points.device)
    _call("mcp_group_rows", points, B, N, C, T, _lib.fptr(points), _lib.iptr(idx), _lib.fptr(out))
    return out


def _interp3_apply_fwd(feat, idx3, w3):
    B, N, _ = idx3.shape
    S, C = feat.shape[1], feat.shape[2]
    out = torch.empty((B, N, C), dtype=torch.float32, device=feat.device)
    _call("mcp_interp3_apply", feat, B, N, S, C, _lib.fptr(feat), _lib.iptr(idx3), _lib.fptr(w3), _lib.fptr(out))
    return out


class _Interp3ApplyFn(torch.autograd.Function):
    """mcp_interp3_apply with its deterministic backward (mcp_interp3_apply_grad_sorted): the weights' gradient as a gather-dot, the
    features' as a weighted segmented reduction over the CSR form of idx3 -- no (B,N,3,C) tensor (autograd over the unfused blend
    builds three)."""

    @staticmethod
    def forward(ctx, feat, idx3, w3):
        feat, idx3, w3 = feat.detach().contiguous(), idx3.contiguous(), w3.detach().contiguous()
        ctx.save_for_backward(feat, idx3, w3)
        return _interp3_apply_fwd(feat, idx3, w3)

    @staticmethod
    def backward(ctx, grad_out):
        feat, idx3, w3 = ctx.saved_tensors
        B, N, _ = idx3.shape
        S, C = feat.shape[1], feat.shape[2]
        grad_out = grad_out.contiguous()
        need_f, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        d_feat = torch.empty_like(feat) if need_f else None
        d_w3 = torch.empty_like(w3) if need_w else None
        order, seg = _scatter_segments(idx3, S) if need_f else (None, None)
        _call("mcp_interp3_apply_grad_sorted", feat, B, N, S, C, _lib.fptr(feat), _lib.iptr(idx3), _lib.fptr(w3), _lib.fptr(grad_out),
              None if order is None else _lib.iptr(order), None if seg is None else _lib.iptr(seg),
              None if d_feat is None else _lib.fptr(d_feat), None if d_w3 is None else _lib.fptr(d_w3))
        return d_feat, None, d_w3


class _Interp3WeightsFn(torch.autograd.Function):
    """mcp_interp3_weights with its hand-written backward (mcp_interp3_weights_grad): one thread per dense point recomputes the
    three distances; the per-neighbour gradients (B,N,3,3) reach the sparse set through the deterministic segmented scatter, with
    the (order, seg) pair of idx3 that _Interp3ApplyFn builds for the same list inside one segments_memo() block."""

    @staticmethod
    def forward(ctx, be, dense, sparse, idx3):
        dense, sparse = dense.detach().contiguous(), sparse.detach().contiguous()
        ctx.save_for_backward(dense, sparse, idx3)
        return be._interp3_weights(dense, sparse, idx3)

    @staticmethod
    def backward(ctx, grad_w3):
        dense, sparse, idx3 = ctx.saved_tensors
        B, N, _ = dense.shape
        S = sparse.shape[1]
        need_d, need_s = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grad_w3 = grad_w3.contiguous()
        d_dense = torch.empty_like(dense) if need_d else None
        d_nb = torch.empty((B, N, 3, 3), dtype=torch.float32, device=dense.device) if need_s else None
        _call("mcp_interp3_weights_grad", dense, B, N, S, _lib.fptr(dense), _lib.fptr(sparse), _lib.iptr(idx3), _lib.fptr(grad_w3),
              None if d_dense is None else _lib.fptr(d_dense), None if d_nb is None else _lib.fptr(d_nb))
        d_sparse = _group_rows_grad(d_nb, idx3, S) if need_s else None
        return None, d_dense, d_sparse, None


class _GroupRowsFn(torch.autograd.Function):
    """Row gather with its scatter-add backward (channel-last counterpart of GroupingOperation, pointnet2_utils.py:156-198)."""

    @staticmethod
    def forward(ctx, points, idx):
        idx = idx.contiguous()
        ctx.save_for_backward(idx)
        ctx.n = points.shape[1]
        return _group_rows_fwd(points.contiguous(), idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return _group_rows_grad(grad_out, idx, ctx.n), None


_segments_memo = None   # {key: (idx, (order, seg))} while a segments_memo() block is open (backward runs on autograd's own thread,
                        # so this is process-wide, not thread-local: one backward pass at a time, as in train.py)


@contextlib.contextmanager
def segments_memo():
    """Around one backward pass: the (order, seg) pair of a gather list is built once and serves every gradient scattered with
    that list -- the same neighbour list gathers coordinates, features and interpolation operands in several nodes of the graph.
    The memo holds the list itself, so its storage cannot be handed to another tensor while the block is open."""
    global _segments_memo
    outer, _segments_memo = _segments_memo, ({} if _segments_memo is None else _segments_memo)
    try:
        yield
    finally:
        _segments_memo = outer


def _scatter_segments(idx, n):
    """(order, seg) of a gather list (B,...) into rows 0..n-1: the gather positions sorted by destination row (stable) and the row
    boundaries in that order -- the operands of mcp_group_rows_grad_sorted; one pair serves every tensor gathered with the list.
    mcp_scatter_segments: a counting sort on the small keys (csrc/scatter_csr.hip) instead of a general stable key-value sort."""
    memo = _segments_memo
    if memo is None:
        return _build_segments(idx, n)
    key = (idx.data_ptr(), tuple(idx.shape), tuple(idx.stride()), idx.dtype, idx._version, n, idx.device.index)
    hit = memo.get(key)
    if hit is None:
        hit = memo[key] = (idx, _build_segments(idx, n), torch.cuda.current_stream(idx.device))
    elif hit[2] != torch.cuda.current_stream(idx.device):   # built on another stream of this backward pass
        done = torch.cuda.Event()
        done.record(hit[2])
        torch.cuda.current_stream(idx.device).wait_event(done)
        for t in hit[1]:
            t.record_stream(torch.cuda.current_stream(idx.device))
    return hit[1]


def _build_segments(idx, n):
    B = idx.shape[0]
    T = idx[0].numel()
    flat = idx.reshape(B, T)
    if flat.dtype != torch.int32:
        flat = flat.int()
    flat = flat.contiguous()
    order = torch.empty((B, T), dtype=torch.int32, device=idx.device)
    seg = torch.empty((B, n + 1), dtype=torch.int32, device=idx.device)
    need = _lib.load().mcp_scatter_segments_workspace_bytes(B, T, n)
    if need == 0:   # more destinations than the kernel's LDS histograms hold: a general stable sort
        keys, order64 = torch.sort(flat, dim=1, stable=True)
        bounds = torch.arange(n + 1, device=idx.device, dtype=keys.dtype).expand(B, n + 1).contiguous()
        return order64.int().contiguous(), torch.searchsorted(keys.contiguous(), bounds).int().contiguous()
    ws = torch.empty((need,), dtype=torch.uint8, device=idx.device)
    _call("mcp_scatter_segments", flat, B, T, n, _lib.iptr(flat), _lib.iptr(order), _lib.iptr(seg), ws.data_ptr(), need)
    return order, seg


def _group_rows_grad(grad_out, idx, n, segments=None):
    """Scatter-add of gathered rows' gradients (B,...,C) back to (B,n,C) as a deterministic segmented reduction: stable sort of the
    gather positions by destination row, in-order sums per row."""
    B, C = grad_out.shape[0], grad_out.shape[-1]
    T = idx[0].numel()
    grad_out = grad_out.contiguous()
    order, seg = segments if segments is not None else _scatter_segments(idx, n)
    grad_rows = torch.empty((B, n, C), dtype=torch.float32, device=grad_out.device)
    _call("mcp_group_rows_grad_sorted", grad_out, B, n, C, T, _lib.fptr(grad_out), _lib.iptr(order), _lib.iptr(seg), _lib.fptr(grad_rows))
    return grad_rows


class _PointConvAggFn(torch.autograd.Function):
    """mcp_pointconv_agg with its hand-written backward (mcp_pointconv_agg_grad): WeightNet recomputed per (centre, neighbour) pair in
    the backward kernel, per-neighbour gradients through the deterministic segmented scatter, weight gradients fixed-order sums.
    qlen: (B,) int32 device tensor or None -- per-element centre lengths, carried to the backward.  Both directions call the *_lengths
    entries: with a null qlen those are the dense entries themselves."""

    @staticmethod
    def forward(ctx, be, idx, s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2, qlen):
        args = [t.detach().contiguous() for t in (s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2)]
        ctx.save_for_backward(idx, *args, qlen)
        return be._pointconv_agg(*args[:3], idx, *args[3:], qlen=qlen)

    @staticmethod
    def backward(ctx, grad_out):
        idx, s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2, qlen = ctx.saved_tensors
        B, N, D = s_points.shape
        S = new_xyz.shape[1]
        lib, dev = _lib.load(), s_points.device
        grad_out = grad_out.contiguous()
        d_new = torch.empty_like(new_xyz)
        d_gxyz = torch.empty((B, S, 32, 3), dtype=torch.float32, device=dev)
        d_rows = torch.empty((B, S, 32, D), dtype=torch.float32, device=dev)
        d_w = torch.empty((lib.mcp_pointconv_agg_grad_floats(),), dtype=torch.float32, device=dev)
        need = lib.mcp_pointconv_agg_grad_workspace_bytes(B, S)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        _call("mcp_pointconv_agg_grad_lengths", s_points, B, N, S, D, 32, _lib.fptr(s_xyz), _lib.fptr(new_xyz), _lib.fptr(s_points), _lib.iptr(idx),
              _len_ptr(qlen), _lib.fptr(w0), _lib.fptr(b0), _lib.fptr(w1), _lib.fptr(b1), _lib.fptr(w2), _lib.fptr(b2), _lib.fptr(grad_out), _lib.fptr(d_new),
              _lib.fptr(d_gxyz), _lib.fptr(d_rows), _lib.fptr(d_w), ws.data_ptr(), need)
        d_sxyz = d_spoints = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[4]:
            if qlen is not None:
                # The rows of padded centres came back as zeros; their idx rows -- which may hold anything -- are replaced before the
                # scatter sorts them: padded centre i names source row i mod N in every slot (grad.spread_padded_rows).  (All of them
                # on row 0 -- what grad._masked_fusion_inputs does -- leaves ONE thread of the segmented reduction with every padded
                # entry: the backward of a half-padded 16 x 8192 batch took 111 times the dense call's time.)
                idx = grad.spread_padded_rows(idx, grad.live_points(qlen, B, S, dev), N)
            segments = _scatter_segments(idx, N)
            if ctx.needs_input_grad[2]:
                d_sxyz = _group_rows_grad(d_gxyz, idx, N, segments)
            if ctx.needs_input_grad[4]:
                d_spoints = _group_rows_grad(d_rows, idx, N, segments)
        return (None, None, d_sxyz, d_new, d_spoints, *_split_flat(d_w, (w0, b0, w1, b1, w2, b2)), None)   # (no gradient for the lengths)


class _CrossFn(torch.autograd.Function):
    """mcp_cross_volume with its hand-written backward (mcp_cross_grad at D = 64 / 128, mcp_cross256_grad at D = 256): recompute
    inside the backward kernel, the per-neighbour gradients through the deterministic segmented scatter (one sort serves both),
    weight gradients fixed-order sums."""

    @staticmethod
    def forward(ctx, be, ia, ib, xyz1, xyz2, points1, points2, wpos, bpos, wmlp, bmlp):
        args = [t.detach().contiguous() for t in (xyz1, xyz2, points1, points2, wpos, bpos, wmlp, bmlp)]
        ctx.save_for_backward(ia, ib, *args)
        return be.cross_volume(*args[:4], ia if ib is None else (ia, ib), be.cross_pack(*args[4:]))

    @staticmethod
    def backward(ctx, grad_out):
        ia, ib, xyz1, xyz2, points1, points2, wpos, bpos, wmlp, bmlp = ctx.saved_tensors
        B, N1, D = points1.shape
        N2 = xyz2.shape[1]
        lib, dev = _lib.load(), points1.device
        grad_out = grad_out.contiguous()
        d_xyz1, d_points1 = torch.empty_like(xyz1), torch.empty_like(points1)
        d_dir = torch.empty((B, N1, 32, 3), dtype=torch.float32, device=dev)
        d_rows = torch.empty((B, N1, 32, D), dtype=torch.float32, device=dev)
        if D == 256:   # its own entry: mcp_cross_grad keeps answering "unsupported" there
            entry, dims = "mcp_cross256_grad", (B, N1, N2, 32)
            floats, need = lib.mcp_cross256_grad_floats(), lib.mcp_cross256_grad_workspace_bytes(B, N1)
        else:
            entry, dims = "mcp_cross_grad", (B, N1, N2, D, 32)
            floats, need = lib.mcp_cross_grad_floats(D), lib.mcp_cross_grad_workspace_bytes(B, N1, D)
        d_w = torch.empty((floats,), dtype=torch.float32, device=dev)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        _call(entry, points1, *dims, _lib.fptr(xyz1), _lib.fptr(xyz2), _lib.fptr(points1), _lib.fptr(points2), _lib.iptr(ia),
              None if ib is None else _lib.iptr(ib), _lib.fptr(wpos), _lib.fptr(bpos), _lib.fptr(wmlp), _lib.fptr(bmlp), _lib.fptr(grad_out),
              _lib.fptr(d_xyz1), _lib.fptr(d_dir), _lib.fptr(d_points1), _lib.fptr(d_rows), _lib.fptr(d_w), ws.data_ptr(), need)
        d_xyz2 = d_points2 = None
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[6]:
            whole = ia if ib is None else torch.cat((ia, ib), dim=-1)
            segments = _scatter_segments(whole, N2)
            if ctx.needs_input_grad[4]:
                d_xyz2 = _group_rows_grad(d_dir, whole, N2, segments)
            if ctx.needs_input_grad[6]:
                d_points2 = _group_rows_grad(d_rows, whole, N2, segments)
        return (None, None, None, d_xyz1, d_xyz2, d_points1, d_points2, *_split_flat(d_w, (wpos, bpos, wmlp, bmlp)))


def _len_ptr(lens):
    """Device pointer of a lengths array as lengths_tensor returns it; None stays None (that side is full)."""
    return None if lens is None else _lib.iptr(lens)


class _AttentionFn(torch.autograd.Function):
    """The attention kernels with their hand-written backward, by head width: 8 / 16 mcp_attention_small_* (row statistics, dQ, dK/dV),
    32 / 64 / 256 mcp_attention_wide_* (D = dO . O, dQ, dK/dV on fp32 MFMA).  The forward keeps the rows' log-sum-exp for the backward
    (no statistics pass, no second forward there); dropout is the in-kernel hash mask.
    qlen / klen: (BF,) int32 device tensors or None -- per-element lengths, carried to the backward.  Both directions call the *_lengths
    entries: with both lengths null those are the dense entries themselves."""

    @staticmethod
    def _family(hd):
        return "mcp_attention_small" if hd in (8, 16) else "mcp_attention_wide"

    @staticmethod
    def forward(ctx, be, q, kv, heads, scale, drop_p, seed, qlen=None, klen=None):
        q, kv = q.detach().contiguous(), kv.detach().contiguous()
        BF, Nq, C = q.shape
        Nk = kv.shape[1]
        out = torch.empty((BF, Nq, C), dtype=torch.float32, device=q.device)
        lse = torch.empty((BF, heads, Nq), dtype=torch.float32, device=q.device)
        _call(_AttentionFn._family(C // heads) + "_lse_lengths", q, BF, Nq, Nk, heads, C // heads, _lib.fptr(q), C, _lib.fptr(kv), 2 * C,
              kv.data_ptr() + 4 * C, 2 * C, float(scale), float(drop_p), int(seed), out.data_ptr(), lse.data_ptr(), _len_ptr(qlen), _len_ptr(klen))
        ctx.heads, ctx.scale, ctx.drop_p, ctx.seed = heads, scale, drop_p, seed
        ctx.save_for_backward(q, kv, out, lse, qlen, klen)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, kv, out, lse, qlen, klen = ctx.saved_tensors
        BF, Nq, C = q.shape
        Nk, heads, hd = kv.shape[1], ctx.heads, C // ctx.heads
        lib, family = _lib.load(), _AttentionFn._family(hd)
        grad_out = grad_out.contiguous()
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        need = (lib.mcp_attention_small_grad_workspace_bytes(BF, Nq, heads) if hd in (8, 16)
                else lib.mcp_attention_wide_grad_workspace_bytes(BF, Nq, Nk, heads, hd))
        ws = torch.empty((need,), dtype=torch.uint8, device=q.device)
        _call(family + "_grad_lse_lengths", q, BF, Nq, Nk, heads, hd, q.data_ptr(), C, kv.data_ptr(), 2 * C, kv.data_ptr() + 4 * C, 2 * C,
              float(ctx.scale), float(ctx.drop_p), int(ctx.seed), _lib.fptr(out), _lib.fptr(grad_out), _lib.fptr(lse), _lib.fptr(dq), _lib.fptr(dkv),
              ws.data_ptr(), need, _len_ptr(qlen), _len_ptr(klen))
        return None, dq, dkv, None, None, None, None, None, None


class _AttentionSmallFn(_AttentionFn):
    """_AttentionFn under the name its autograd node carries at head dims 8 / 16 (profiles and graph checks tell the families apart)."""


class _AttentionWideFn(_AttentionFn):
    """_AttentionFn under the name its autograd node carries at head widths 32 / 64 / 256."""


def _prelu_drop_fwd(z, slope, drop_p=0.0, seed=0):
    """m * prelu(z, slope): slope a 1-element device tensor; drop_p = 0: plain PReLU (mcp_prelu_dropout)."""
    out = torch.empty_like(z)
    _call("mcp_prelu_dropout", z, z.numel(), _lib.fptr(z), _lib.fptr(slope), float(drop_p), int(seed), _lib.fptr(out))
    return out


def _prelu_drop_bwd(z, slope, grad_out, drop_p=0.0, seed=0):
    """(dz, dslope (1,)) of the above in one pass over z and grad_out (mcp_prelu_dropout_grad; dslope summed in a fixed order)."""
    dz, da = torch.empty_like(z), torch.empty((1,), dtype=torch.float32, device=z.device)
    need = _lib.load().mcp_prelu_dropout_grad_workspace_bytes(z.numel())
    ws = torch.empty((need,), dtype=torch.uint8, device=z.device)
    _call("mcp_prelu_dropout_grad", z, z.numel(), _lib.fptr(z), _lib.fptr(slope), _lib.fptr(grad_out), float(drop_p), int(seed),
          _lib.fptr(dz), _lib.fptr(da), ws.data_ptr(), need)
    return dz, da


class _PreluDropFn(torch.autograd.Function):
    """mcp_prelu_dropout / mcp_prelu_dropout_grad: PReLU (one slope, the live parameter) then dropout, one pass each way; only z is
    kept for the backward, which regenerates the mask from the seed."""

    @staticmethod
    def forward(ctx, z, slope, drop_p, seed):
        z = z.detach().contiguous()
        ctx.drop_p, ctx.seed, ctx.slope_shape = drop_p, seed, slope.shape
        slope = slope.detach().reshape(1).contiguous()
        ctx.save_for_backward(z, slope)
        return _prelu_drop_fwd(z, slope, drop_p, seed)

    @staticmethod
    def backward(ctx, grad_out):
        z, slope = ctx.saved_tensors
        dz, da = _prelu_drop_bwd(z, slope, grad_out.contiguous(), ctx.drop_p, ctx.seed)
        return dz, da.reshape(ctx.slope_shape), None, None


def _leaky_grad(gy, y, slope):
    """gy * act'(z) of a one-slope activation (0 <= slope <= 1) from its OUTPUT y (y > 0 exactly where z > 0): one pass."""
    return torch.ops.aten.leaky_relu_backward(gy, y, float(slope), True)


def _tall_matmul(a, w, bias=None):
    """a (rows, n) @ w (n, k) (+ bias) for rows >> n, k (the input gradient of a per-point Linear): the streaming forward kernel on w^T
    where it is built for the shape (the library GEMM takes ~160 us for 196608 x 64 @ 64 x 32 against ~30), the library otherwise."""
    be = backend()
    n, k = w.shape
    if a.is_cuda and hasattr(be, "linear_kernel_ok") and a.shape[0] >= 8192:
        a = a.contiguous()
        if be.linear_kernel_ok(a, k):
            return be.linear(a, w.t().contiguous(), bias, 1.0, None)
    return a @ w if bias is None else torch.addmm(bias, a, w)


def _wgrad(gz, x):
    """(gz^T x, column sums of gz) for gz (rows, n), x (rows, k): mcp_linear_wgrad (rows on the MFMA's contraction axis, fixed-order
    partial sums) where it takes the shape -- n beyond 256 in column blocks of 256 -- and the library GEMM + a reduce otherwise."""
    rows, n = gz.shape
    k = x.shape[1]
    lib = _lib.load() if gz.is_cuda else None
    blocks = [(c0, min(256, n - c0)) for c0 in range(0, n, 256)]
    if lib is None or rows < 2048 or any(lib.mcp_linear_wgrad_workspace_bytes(rows, nb, k) == 0 for _, nb in blocks):
        return gz.t() @ x, gz.sum(dim=0)
    gz, x = gz.contiguous(), x.contiguous()
    dw = torch.empty((n, k), dtype=torch.float32, device=gz.device)
    db = torch.empty((n,), dtype=torch.float32, device=gz.device)
    for c0, nb in blocks:
        need = lib.mcp_linear_wgrad_workspace_bytes(rows, nb, k)
        ws = torch.empty((need,), dtype=torch.uint8, device=gz.device)
        _call("mcp_linear_wgrad", gz, rows, nb, k, gz.data_ptr() + 4 * c0, n, _lib.fptr(x), k, dw.data_ptr() + 4 * c0 * k, db.data_ptr() + 4 * c0,
              ws.data_ptr(), need)
    return dw, db


class _Mlp2Fn(torch.autograd.Function):
    """mcp_mlp2 (Linear, one-slope PReLU, Linear, + residual) with an explicit backward on the streaming kernels: the hidden
    activation is rebuilt once (forward kernel), the two input-gradient products run on the forward kernel with transposed weights,
    the two weight gradients on mcp_linear_wgrad -- instead of autograd over the unfused twin (four library GEMMs on tall, narrow
    operands: 3.6 ms per training step at the pipeline's shapes)."""

    @staticmethod
    def forward(ctx, fused, x, res, w1, b1, w2, b2, slope):
        args = [None if t is None else t.detach() for t in (x, res, w1, b1, w2, b2)]
        sl = slope.detach() if isinstance(slope, torch.Tensor) else slope
        out = fused(*args, sl)
        ctx.slope_is_tensor = isinstance(slope, torch.Tensor)
        ctx.slope = None if ctx.slope_is_tensor else float(slope)
        ctx.has_res = res is not None
        ctx.save_for_backward(x, w1, b1, w2, *( [slope] if ctx.slope_is_tensor else []))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, w1, b1, w2, *rest = ctx.saved_tensors
        slope = rest[0] if ctx.slope_is_tensor else ctx.slope
        hdim, cin = w1.shape
        cout = w2.shape[0]
        x2 = x.reshape(-1, cin)
        gy = grad_out.reshape(-1, cout).contiguous()
        hid = _tall_matmul(x2, w1.t(), b1)
        g_act = _tall_matmul(gy, w2)                                   # (rows, hidden)
        dslope = None
        if ctx.slope_is_tensor and hid.is_cuda:                        # the live PReLU slope: one pass each for act and (g_hid, dslope)
            sl = slope.detach().reshape(1).contiguous()
            hid, g_act = hid.contiguous(), g_act.contiguous()
            act = _prelu_drop_fwd(hid, sl)
            g_hid, dslope = _prelu_drop_bwd(hid, sl, g_act)
            dslope = dslope.reshape(slope.shape) if ctx.needs_input_grad[7] else None
        else:
            pos = hid > 0
            act = torch.where(pos, hid, hid * slope)
            g_hid = torch.where(pos, g_act, g_act * slope)
            if ctx.slope_is_tensor and ctx.needs_input_grad[7]:
                dslope = (g_act * torch.where(pos, torch.zeros_like(hid), hid)).sum().reshape(slope.shape)
        dw2, db2 = _wgrad(gy, act)
        dw1, db1 = _wgrad(g_hid, x2)
        dx = _tall_matmul(g_hid, w1).reshape(x.shape) if ctx.needs_input_grad[1] else None
        dres = grad_out if ctx.has_res and ctx.needs_input_grad[2] else None
        return (None, dx, dres, dw1 if ctx.needs_input_grad[3] else None, db1 if (b1 is not None and ctx.needs_input_grad[4]) else None,
                dw2 if ctx.needs_input_grad[5] else None, db2 if ctx.needs_input_grad[6] else None, dslope)


class _LinearFn(torch.autograd.Function):
    """The fused Linear (+ one-slope activation, + residual) with an explicit backward: two GEMMs and a mask taken from the saved
    activation OUTPUT (for 0 <= slope <= 1 the output of act is positive exactly where its argument is), instead of evaluating the
    layer again under autograd.  With a residual AND an activation the kernel runs without the residual and the sum is made here
    (the same single rounded addition the kernel's epilogue does, so the same bits): the mask then comes from act(z) itself -- a
    mask recovered as (y - res) > 0 loses entries with 0 < act(z) < ulp(res) / 2."""

    @staticmethod
    def forward(ctx, fused, x, w, b, slope, res):
        act_res = res is not None and slope != 1.0
        y = fused(x.detach(), w.detach(), None if b is None else b.detach(), slope, None if (res is None or act_res) else res.detach())
        ctx.slope, ctx.has_b, ctx.has_res = float(slope), b is not None, res is not None
        ctx.save_for_backward(x, w, y if slope != 1.0 else None)
        return y + res.detach() if act_res else y

    @staticmethod
    def backward(ctx, grad_out):
        x, w, act = ctx.saved_tensors
        n, k = w.shape
        gy = grad_out.reshape(-1, n)
        if ctx.slope != 1.0:
            gz = _leaky_grad(gy, act.reshape(-1, n), ctx.slope)
        else:
            gz = gy
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            dx = _tall_matmul(gz, w).reshape(x.shape)                  # dx = gz W: the forward kernel again, on W^T
        if ctx.needs_input_grad[2] or (ctx.has_b and ctx.needs_input_grad[3]):
            dw, db = _wgrad(gz, x.reshape(-1, k))                      # dW = gz^T x and db in one kernel (csrc/linear_grad.hip)
            if not (ctx.has_b and ctx.needs_input_grad[3]):
                db = None
        dres = grad_out if ctx.has_res and ctx.needs_input_grad[5] else None
        return None, dx, dw, db, None, dres


class _TorchLinearFn(torch.autograd.Function):
    """A tall per-point Linear the fused kernel does not take (the 3 -> 32 lift, the 32 -> 3 head: widths that are not multiples
    of 4) -- the library's forward, but the backward of _LinearFn: the weight gradient of a (rows x 3) operand is otherwise a
    (3 x rows) x (rows x 32) library GEMM of 300-430 us (round 5 trace) against ~20 for mcp_linear_wgrad."""

    @staticmethod
    def forward(ctx, x, w, b, slope):
        y = torch.nn.functional.linear(x.detach(), w.detach(), None if b is None else b.detach())
        if slope != 1.0:
            y = torch.where(y > 0, y, y * slope)
        ctx.slope, ctx.has_b = float(slope), b is not None
        ctx.save_for_backward(x, w, y if slope != 1.0 else None)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, w, act = ctx.saved_tensors
        n, k = w.shape
        gy = grad_out.reshape(-1, n)
        gz = _leaky_grad(gy, act.reshape(-1, n), ctx.slope) if ctx.slope != 1.0 else gy
        dx = _tall_matmul(gz, w).reshape(x.shape) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw, db = _wgrad(gz, x.reshape(-1, k))
            if not (ctx.has_b and ctx.needs_input_grad[2]):
                db = None
        return dx, dw, db, None


def plain_linear(x, w, b, slope=1.0):
    """act(x W^T + b) on the library's GEMM with the streaming backward kernels (training forwards, tall inputs only)."""
    return _TorchLinearFn.apply(x, w, b, float(slope))


class _ChamferFn(torch.autograd.Function):
    """chamfer_loss (models/utils.py:36-45, pytorch3d defaults) per sample, with an explicit backward.  Forward: the two nearest-
    neighbour searches return the squared distances themselves (direct form), so the value is two row means -- nothing is gathered or
    re-evaluated.  Backward: d/dx_i = (2 g_b / N)(x_i - y[ixy_i]) - sum over {j: iyx_j = i} of (2 g_b / M)(y_j - x_i), the second term
    as the deterministic segmented scatter of the other direction's direct term (and symmetrically for y when it asks for a gradient:
    the ground truth of the training objective does not).  Autograd over the unfused form (grad.chamfer_twin) took ~45 launches per
    call, 15 calls per training step."""

    @staticmethod
    def forward(ctx, be, x, y):
        x, y = x.detach().contiguous(), y.detach().contiguous()
        ixy, dxy = be.knn(x, y, 1, mode=MCP_DIST_DIRECT, return_dist=True)
        iyx, dyx = be.knn(y, x, 1, mode=MCP_DIST_DIRECT, return_dist=True)
        ctx.save_for_backward(x, y, ixy, iyx)      # the index lists as (B,N,1) / (B,M,1)
        return dxy[..., 0].mean(1) + dyx[..., 0].mean(1)

    @staticmethod
    def backward(ctx, gv):
        x, y, ixy, iyx = ctx.saved_tensors
        B, N, _ = x.shape
        M = y.shape[1]
        gx_d = (x - _group_rows_fwd(y, ixy).squeeze(2)) * (gv * (2.0 / N)).view(B, 1, 1)
        gy_d = (y - _group_rows_fwd(x, iyx).squeeze(2)) * (gv * (2.0 / M)).view(B, 1, 1)
        gx = gx_d - _group_rows_grad(gy_d.unsqueeze(2), iyx, N) if ctx.needs_input_grad[1] else None
        gy = gy_d - _group_rows_grad(gx_d.unsqueeze(2), ixy, M) if ctx.needs_input_grad[2] else None
        return None, gx, gy


def lengths_tensor(lengths, batch, limit, device):
    """Per-cloud lengths as the (B,) int32 device array the length-aware kernels read.  A sequence of ints or a CPU tensor is
    validated here (one entry per batch element, 0 <= len <= limit; RuntimeError otherwise) and uploaded from pinned memory on
    the current stream, without a synchronisation.  A device tensor (int32 / int64) is trusted as it is: reading it back would
    be a synchronisation, and the kernels clamp every length to [0, limit] themselves."""
    if lengths is None:
        return None
    if torch.is_tensor(lengths) and lengths.is_cuda:
        if lengths.dtype not in (torch.int32, torch.int64) or lengths.numel() != batch:
            raise RuntimeError(f"lengths: expected {batch} int32/int64 entries, got {lengths.numel()} of {lengths.dtype}")
        return lengths.reshape(batch).to(torch.int32).contiguous()
    host = torch.as_tensor(lengths)
    if host.is_floating_point() or host.is_complex() or host.dtype == torch.bool:
        raise RuntimeError(f"lengths: expected integers, got {host.dtype}")
    host = host.reshape(-1).to(torch.int64)
    if host.numel() != batch:
        raise RuntimeError(f"lengths: expected one entry per batch element ({batch}), got {host.numel()}")
    if batch and (int(host.min()) < 0 or int(host.max()) > limit):
        raise RuntimeError(f"lengths: every entry must lie in [0, {limit}], got {host.tolist()}")
    if torch.device(device).type != "cuda":   # the CPU oracle backend's masked formulations: nothing to upload
        return host.to(torch.int32)
    return host.to(torch.int32).pin_memory().to(device, non_blocking=True)


def _valid_counts(lens, batch, limit, device):
    """(B,) int32 number of valid rows per element as the kernels see it (clamped; `limit` everywhere without lengths)."""
    if lens is None:
        return torch.full((batch,), limit, dtype=torch.int32, device=device)
    return lens.clamp(0, limit)


# ---- set-abstraction layer (csrc/group_mlp.hip) ----
GROUP_MLP_LDS_IMAGE_BYTES = 64 * 1024
GROUP_MLP_POOLS = {"max": 0, "max_pool": 0, "mean": 1, "avg": 1, "avg_pool": 1}


def group_mlp_supported(c, widths, nsample=1, use_xyz=True):
    """The shapes mcp_group_mlp is built for: c input feature channels, layer widths, neighbours per centre."""
    widths = list(widths)
    if not (1 <= len(widths) <= 3 and 1 <= nsample <= 64 and 0 <= c <= 128 and c % 4 == 0 and (c > 0 or use_xyz)):
        return False
    return all(w in (32, 64, 128) for w in widths[:-1]) and widths[-1] in (32, 64, 128, 256)


def group_mlp_image_bytes(c, widths):
    """Bytes of the split-bf16 weight pieces of a supported (c, widths): per layer 32-channel output tiles x k-steps x 3 pieces x
    64 lanes x 16 B, the feature k-steps of layer 1 rounded up to 1, 2, 4 or 8."""
    ks0 = (c + 15) // 16
    ks = [0 if ks0 == 0 else 1 << (ks0 - 1).bit_length()] + [w // 16 for w in widths[:-1]]
    return sum((w // 32) * k * 3 * 64 * 16 for w, k in zip(widths, ks))


def group_mlp_weights_in_lds(c, widths):
    """Python mirror of the kernel's one dispatch predicate (gm_weights_in_lds): the weight image is staged in LDS once per
    workgroup when it is at most 64 KB, and read through L2 otherwise."""
    return group_mlp_image_bytes(c, list(widths)) <= GROUP_MLP_LDS_IMAGE_BYTES


# Shape classes (column group 8 | 16 | 32 | 64, feature channels, widths) -> fewest centres B * M at which sampling-free
# "ball query + mcp_group_mlp" measured faster than the composition "mcp_query_and_group + folded convs + max" by more than the
# composition's own spread (tools/group_mlp_times.py -> profiles/group_mlp_times.json).  A class without a row keeps the composition.
# Measured at B = 8 (ms): 16384 -> 1024 / ns 16 / 4 -> 32/32/64 0.154 against 0.292 (spread 0.022) and 1024 -> 256 / ns 16 / 64 ->
# 64/64/128 0.060 against 0.134 (spread 0.018) qualify, 256 -> 64 / ns 8 / 128 -> 128/128/256 (0.103 against 0.113, spread 0.057) does
# not.  The table is still empty: filling it changes what existing callers run and is a change of its own.
GROUP_MLP_FUSED_CLASSES = {}


def group_mlp_class(c, widths, nsample):
    return (8 if nsample <= 8 else 16 if nsample <= 16 else 32 if nsample <= 32 else 64, int(c), tuple(int(w) for w in widths))


def _routes(table, cls, count):
    """One route predicate for every fused layer: the class has a row in the table and the call is at least that large."""
    least = table.get(cls)
    return least is not None and count >= least


def group_mlp_routes_fused(c, widths, nsample, centres):
    """The modules' route predicate: a pure function of the padded shapes."""
    return _routes(GROUP_MLP_FUSED_CLASSES, group_mlp_class(c, widths, nsample), centres)


def _fold_params(conv, bn):
    return conv.weight, conv.bias, getattr(bn, "weight", None), getattr(bn, "bias", None)


def _fold(bn, weight, bias, gamma, beta):
    """The float64 fold of fold_conv_bn / fold_conv_bn_grad on the tensors the caller chose (detached or in the graph); the running
    statistics are constants either way."""
    w = weight.double().flatten(1)
    b = bias.double() if bias is not None else w.new_zeros(w.shape[0])
    if bn is not None:
        g = gamma.double() if gamma is not None else w.new_ones(w.shape[0])
        beta = beta.double() if beta is not None else w.new_zeros(w.shape[0])
        scale = g / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        w, b = w * scale[:, None], (b - bn.running_mean.detach().double()) * scale + beta
    return w.float().contiguous(), b.float().contiguous()


def _det(t, contiguous=True):
    """An optional tensor out of the graph -- and, as the kernels of an autograd function read it, contiguous."""
    if t is None:
        return None
    return t.detach().contiguous() if contiguous else t.detach()


def _pairs(flat):
    """[(W, b), ...] of the flat parameter list an autograd function takes."""
    return list(zip(flat[0::2], flat[1::2]))


def _quads(flat):
    """[(W, b, gamma, beta), ...] of the flat parameter list an autograd function takes."""
    return list(zip(flat[0::4], flat[1::4], flat[2::4], flat[3::4]))


def _flat(groups):
    return [t for group in groups for t in group]


def _unused_zeros(t, wanted):
    """The gradient of coordinates that never enter a set-abstraction layer (use_xyz = False)."""
    return torch.zeros_like(t) if wanted else None


def fold_conv_bn(conv, bn=None):
    """(W (out, in), b (out,)) fp32 of a 1x1 convolution (or Linear) followed by an eval-mode BatchNorm with the layer's own eps:
    W' = W * g / sqrt(var + eps), b' = (b - mean) * g / sqrt(var + eps) + beta, folded in float64 and rounded once."""
    return _fold(bn, *[_det(t, False) for t in _fold_params(conv, bn)])


def fold_conv_bn_grad(conv, bn=None):
    """fold_conv_bn as an autograd function of conv.weight, conv.bias, bn.weight and bn.bias (the running statistics are constants):
    the same float64 expressions and the same single rounding, so the values have fold_conv_bn's bits; the gradient of (W', b')
    reaches the four parameters through autograd's chain rule.  For the differentiable fused layers (HipBackend.fp_mlp_layer)."""
    return _fold(bn, *_fold_params(conv, bn))


def _check_layers(name, layers, cin, widths):
    """Every layer's W (out, in) and its per-channel vectors -- b, or b, gamma, beta where None stands for an absent one -- against
    the first layer's input columns and the widths."""
    for (w, *vecs), k, o in zip(layers, [cin, *widths[:-1]], widths):
        if tuple(w.shape) != (o, k) or any(t is not None and tuple(t.shape) != (o,) for t in vecs):
            got = [tuple(w.shape), *(None if t is None else tuple(t.shape) for t in vecs)]
            raise RuntimeError(f"{name}: expected W {(o, k)} and {'b' if len(vecs) == 1 else 'b, gamma, beta'} {(o,)}, got {got}")


def _pack_image(name, lead, shape, ok, weights, cin=None, grad_alloc=False, floats_lead=None):
    """mcp_<name>_pack's image of [(W (out, in), b (out,)), ...] fp32 device tensors -> (packed, widths).  lead: the integers both
    mcp_<name>_packed_floats (floats_lead where it takes others) and mcp_<name>_pack take in front of (layers, widths); shape, ok:
    how the message names the shape, and what it must satisfy before the library is asked for a size; cin: the first layer's
    input columns where the (W, b) shapes are checked; grad_alloc: the image is one of the backward's buffers (_grad_empty)."""
    widths = [int(w.shape[0]) for w, _ in weights]
    wid = _int_array(widths)
    floats = getattr(_lib.load(), f"mcp_{name}_packed_floats")
    n = floats(*(lead if floats_lead is None else floats_lead), len(widths), wid) if len(widths) <= 3 and ok else 0
    if n == 0:
        raise _lib.Unsupported(f"{name}: unsupported shape {shape} widths={widths}")
    if cin is not None:
        _check_layers(name, weights, cin, widths)
    ws = [w.contiguous() for w, _ in weights]
    bs = [b.contiguous() for _, b in weights]
    dev = ws[0].device
    packed = _grad_empty((n,), torch.float32, dev) if grad_alloc else torch.empty((n,), dtype=torch.float32, device=dev)
    _call(f"mcp_{name}_pack", packed, *lead, len(widths), wid, _ptr_array(ws), _ptr_array(bs), _lib.fptr(packed))
    return packed, widths


def group_mlp_pack_weights(weights, use_xyz=True):
    """The MFMA-operand image of mcp_group_mlp from [(W (out, in), b (out,)), ...] fp32 device tensors -> (packed, widths)."""
    c, xyz = int(weights[0][0].shape[1]) - (3 if use_xyz else 0), int(bool(use_xyz))
    return _pack_image("group_mlp", (c, xyz), f"c={c}", c != 0 or xyz, weights, floats_lead=(c,))


def group_mlp_pack(convs, bns=None, use_xyz=True):
    """Pack the shared MLP of a set-abstraction layer once: convs are its 1x1 Conv2d (or Linear) modules in order, bns the eval-mode
    BatchNorm that follows each (None, or None entries, where there is none).  -> (packed, widths) for HipBackend.group_mlp."""
    bns = [None] * len(convs) if bns is None else list(bns)
    return group_mlp_pack_weights([fold_conv_bn(c, b) for c, b in zip(convs, bns)], use_xyz)


# ---- backward of the set-abstraction layer (csrc/group_mlp_grad.hip) ----
GROUP_MLP_GRAD_LDS_IMAGE_BYTES = 128 * 1024


def group_mlp_grad_supported(c, widths, nsample=1, use_xyz=True):
    """The shapes mcp_group_mlp_grad is built for: every shape of mcp_group_mlp (the kernel has one register class; nothing was
    narrowed)."""
    return group_mlp_supported(c, widths, nsample, use_xyz)


def group_mlp_grad_image_bytes(c, widths, use_xyz=True):
    """Bytes of the transposed-weight pieces of a supported shape: for l = L .. 2 the two k-steps per tile of gz_l into the tiles of
    layer l - 1, then the k-steps of gz_1 into the ceil((c + 3) / 32) tiles of dx (c without use_xyz)."""
    tiles = [w // 32 for w in widths]
    cin = c + (3 if use_xyz else 0)
    pieces = sum(2 * tiles[l] * tiles[l - 1] for l in range(1, len(tiles))) + 2 * tiles[0] * ((cin + 31) // 32)
    return pieces * 3 * 64 * 16


def group_mlp_grad_packed_floats(c, widths, use_xyz=True):
    """Floats of mcp_group_mlp_grad_pack's image: the forward image (pieces, position columns, biases), then the transposed pieces."""
    return (group_mlp_image_bytes(c, widths) + group_mlp_grad_image_bytes(c, widths, use_xyz)) // 4 + widths[0] // 32 * 128 + sum(widths)


def group_mlp_grad_weights_in_lds(c, widths, use_xyz=True):
    """Python mirror of the backward kernel's one staging predicate (gg_weights_in_lds): both parts of the image are staged in LDS
    once per workgroup when together they are at most 128 KB, and read through L2 otherwise."""
    widths = list(widths)
    return group_mlp_image_bytes(c, widths) + group_mlp_grad_image_bytes(c, widths, use_xyz) <= GROUP_MLP_GRAD_LDS_IMAGE_BYTES


# Shape classes (column group 8 | 16 | 32 | 64, feature channels, widths) -> fewest centres B * M at which the module's fused
# differentiable route (ball query, transposition, mcp_group_mlp forward, mcp_group_mlp_grad backward) measured faster, forward +
# backward, than the composition's forward + backward by more than the composition's own spread (tools/group_mlp_grad_times.py ->
# profiles/group_mlp_grad_times.json).  A class without a row keeps the composition.  Measured at B = 8 (ms, forward + backward):
# 16384 -> 1024 / ns 16 / 4 -> 32/32/64 1.533 against 1.329, 1024 -> 256 / ns 16 / 64 -> 64/64/128 1.119 against 0.930, 256 -> 64 / ns 8 /
# 128 -> 128/128/256 1.217 against 0.918: slower fused at all three, no class enters; grad_route = "always" takes the kernel.
GROUP_MLP_GRAD_FUSED_CLASSES = {}


def group_mlp_grad_routes_fused(c, widths, nsample, centres):
    """PointnetSAModuleMSG's route predicate when a gradient is wanted: a pure function of the padded shapes."""
    return _routes(GROUP_MLP_GRAD_FUSED_CLASSES, group_mlp_class(c, widths, nsample), centres)


def group_mlp_grad_pack_weights(weights, use_xyz=True):
    """mcp_group_mlp_grad_pack's image from [(W (out, in), b (out,)), ...] fp32 device tensors -> (packed, widths)."""
    cin, xyz = int(weights[0][0].shape[1]), int(bool(use_xyz))
    c = cin - (3 if use_xyz else 0)
    return _pack_image("group_mlp_grad", (c, xyz), f"c={c}", c >= 0, weights, cin=cin, grad_alloc=True)


class _GroupMlpLayerFn(torch.autograd.Function):
    """mcp_group_mlp with its hand-written backward (mcp_group_mlp_grad): the layer is re-evaluated inside the backward kernel, so
    only the inputs are kept (not the output: the kernel takes the winner slots and the last ReLU mask from its own recompute) --
    autograd over the composition keeps the (B, 3 + C, M, nsample) grouped tensor and one (B, C_l, M, nsample) per layer.
    Gradients: xyz, new_xyz, features, row_bias, every W and b; idx and the lengths get none."""

    @staticmethod
    def forward(ctx, be, pool, use_xyz, idx, ql, xyz, new_xyz, features, row_bias, *wb):
        xyz, new_xyz, features, row_bias, *wb = [_det(t) for t in (xyz, new_xyz, features, row_bias, *wb)]
        packed, widths = group_mlp_pack_weights(_pairs(wb), use_xyz)
        out = be._group_mlp(xyz, new_xyz, features, idx, packed, widths, pool, use_xyz, ql, row_bias)
        ctx.be, ctx.pool, ctx.use_xyz = be, pool, use_xyz
        ctx.save_for_backward(idx, ql, xyz, new_xyz, features, row_bias, *wb)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        idx, ql, xyz, new_xyz, features, row_bias, *wb = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_feat, d_xyz, d_new, d_rb, d_w, d_b, _ = ctx.be.group_mlp_grad(
            xyz, new_xyz, features, idx, _pairs(wb), grad_out, pool=ctx.pool, use_xyz=ctx.use_xyz, new_xyz_lengths=ql,
            row_bias=row_bias, want_features=need[7] and features is not None, want_xyz=need[5] and ctx.use_xyz,
            want_new_xyz=need[6] and ctx.use_xyz, want_row_bias=need[8] and row_bias is not None)
        if not ctx.use_xyz:
            d_xyz, d_new = _unused_zeros(xyz, need[5]), _unused_zeros(new_xyz, need[6])
        return (None, None, None, None, None, d_xyz, d_new, d_feat, d_rb, *_flat(zip(d_w, d_b)))


# ---- feature-propagation layer (csrc/fp_mlp.hip) ----
FP_MLP_LDS_IMAGE_BYTES = 64 * 1024
FP_MLP_RULES = {"given": 0, "pointnet2": 1, "flownet3d": 2}


def fp_mlp_supported(c2, c1, widths):
    """The shapes mcp_fp_mlp is built for: c2 channels of the known (interpolated) features, c1 of the skip row, layer widths."""
    widths = list(widths)
    if not (1 <= len(widths) <= 3 and 4 <= c2 <= 512 and c2 % 4 == 0 and 0 <= c1 <= 512 and c1 + c2 <= 768):
        return False
    return all(w in (32, 64, 128, 256) for w in widths)


def fp_mlp_image_bytes(c2, c1, widths):
    """Bytes of the split-bf16 weight pieces of a supported shape: per layer 32-channel output tiles x k-steps x 3 pieces x 64 lanes
    x 16 B; layer 1 has the k-steps of the interpolated part and those of the skip row, each rounded up on its own."""
    ks = [(c2 + 15) // 16 + (c1 + 15) // 16] + [w // 16 for w in widths[:-1]]
    return sum((w // 32) * k * 3 * 64 * 16 for w, k in zip(widths, ks))


def fp_mlp_weights_in_lds(c2, c1, widths):
    """Python mirror of the kernel's one staging predicate (fp_weights_in_lds): a weight image of at most 64 KB is staged whole in
    LDS, a larger one is streamed slab by slab through two LDS buffers."""
    return fp_mlp_image_bytes(c2, c1, list(widths)) <= FP_MLP_LDS_IMAGE_BYTES


def fp_mlp_tmax(widths):
    """Accumulator tiles per bank of the kernel instantiation that serves these widths (2, 4 or 8)."""
    widest = max(widths)
    return 2 if widest <= 64 else 4 if widest <= 128 else 8


# Shape classes (c2, c1, widths) -> fewest rows B * n at which "three_nn + mcp_fp_mlp" measured faster than the module's composition
# (three_nn, weights, three_interpolate, cat, folded convs) by more than the composition's own spread (tools/fp_mlp_times.py ->
# profiles/fp_mlp_times.json).  A class without a row keeps the composition.  Measured at B = 8: 256 + 3 -> 256/256 over n = 16384
# (0.516 against 0.807 ms, spread 0.071) enters; 256 + 128 -> 256/256 over n = 1024 (0.204 against 0.256, spread 0.075) and
# 128 + 4 -> 128/128/128 over n = 4096 (0.248 against 0.296, spread 0.065) are faster by less than the spread and stay out.
FP_MLP_FUSED_CLASSES = {(256, 3, (256, 256)): 8 * 16384}


def fp_mlp_class(c2, c1, widths):
    return (int(c2), int(c1), tuple(int(w) for w in widths))


def fp_mlp_routes_fused(c2, c1, widths, rows):
    """PointnetFPModule's route predicate: a pure function of the padded shapes."""
    return _routes(FP_MLP_FUSED_CLASSES, fp_mlp_class(c2, c1, widths), rows)


def _fp_pack(name, weights, c2, grad_alloc):
    """The fp family's images: the first c2 columns of the first W meet the interpolated features, the rest the skip row."""
    c2, cin = int(c2), int(weights[0][0].shape[1])
    return _pack_image(name, (c2, cin - c2), f"c2={c2} c1={cin - c2}", cin >= c2, weights, cin=cin, grad_alloc=grad_alloc)


def fp_mlp_pack_weights(weights, c2):
    """The MFMA-operand image of mcp_fp_mlp from [(W (out, in), b (out,)), ...] fp32 device tensors; the first c2 columns of the
    first W meet the interpolated features, the rest the skip row -> (packed, widths)."""
    return _fp_pack("fp_mlp", weights, c2, False)


def fp_mlp_pack(convs, bns=None, c2=None):
    """Pack the shared MLP of a feature-propagation layer once: convs are its 1x1 Conv2d (or Linear) modules in order, bns the
    eval-mode BatchNorm that follows each (None, or None entries, where there is none), c2 the channels of the interpolated part
    (the leading input columns of the first layer).  -> (packed, widths) for HipBackend.fp_mlp."""
    bns = [None] * len(convs) if bns is None else list(bns)
    return fp_mlp_pack_weights([fold_conv_bn(c, b) for c, b in zip(convs, bns)], c2)


# ---- backward of the feature-propagation layer (csrc/fp_mlp_grad.hip) ----
def fp_mlp_grad_supported(c2, c1, widths):
    """The shapes mcp_fp_mlp_grad is built for: every shape of mcp_fp_mlp (no register class was narrowed)."""
    return fp_mlp_supported(c2, c1, widths)


def fp_mlp_grad_image_bytes(c2, c1, widths):
    """Bytes of the backward slabs (the transposed weights) of a supported shape: for l = L .. 2 the two k-steps per tile of gz_l into
    the tiles of layer l - 1, then the k-steps of gz_1 into the ceil((c2 + c1) / 32) tiles of dx."""
    tiles = [w // 32 for w in widths]
    slabs = sum(2 * tiles[l] * tiles[l - 1] for l in range(1, len(tiles))) + 2 * tiles[0] * ((c2 + c1 + 31) // 32)
    return slabs * 3 * 64 * 16


def fp_mlp_grad_packed_floats(c2, c1, widths):
    """Floats of mcp_fp_mlp_grad_pack's image: the forward image (slabs, biases), then the backward slabs."""
    return (fp_mlp_image_bytes(c2, c1, widths) + fp_mlp_grad_image_bytes(c2, c1, widths)) // 4 + sum(widths)


def fp_mlp_grad_weights_in_lds(c2, c1, widths):
    """Python mirror of the backward kernel's one staging predicate (fg_whole): both halves of the image at most 64 KB."""
    return fp_mlp_weights_in_lds(c2, c1, widths) and fp_mlp_grad_image_bytes(c2, c1, list(widths)) <= FP_MLP_LDS_IMAGE_BYTES


# Shape classes (c2, c1, widths) -> fewest rows B * n at which the module's fused differentiable route (three_nn, transpositions,
# mcp_fp_mlp forward, mcp_fp_mlp_grad backward) measured faster, forward + backward, than the composition's forward + backward by
# more than the composition's own spread (tools/fp_mlp_grad_times.py -> profiles/fp_mlp_grad_times.json).  A class without a row
# keeps the composition.  Measured at B = 8 (ms, forward + backward): 256 + 3 -> 256/256 over n = 16384 (3.225 against 3.651, spread
# 0.055) enters; 256 + 128 -> 256/256 over n = 1024 (1.052 against 0.873) and 128 + 4 -> 128/128/128 over n = 4096 (0.998 against
# 0.903) are slower and stay out.
FP_MLP_GRAD_FUSED_CLASSES = {(256, 3, (256, 256)): 8 * 16384}


def fp_mlp_grad_routes_fused(c2, c1, widths, rows):
    """PointnetFPModule's route predicate when a gradient is wanted: a pure function of the padded shapes."""
    return _routes(FP_MLP_GRAD_FUSED_CLASSES, fp_mlp_class(c2, c1, widths), rows)


def _grad_empty(shape, dtype, device):
    """Every buffer the fused backward allocates (the tests refill them with NaN: each must be written before it is read)."""
    return torch.empty(shape, dtype=dtype, device=device)


def fp_mlp_grad_pack_weights(weights, c2):
    """mcp_fp_mlp_grad_pack's image from [(W (out, in), b (out,)), ...] fp32 device tensors -> (packed, widths)."""
    return _fp_pack("fp_mlp_grad", weights, c2, True)


class _FpMlpLayerFn(torch.autograd.Function):
    """mcp_fp_mlp with its hand-written backward (mcp_fp_mlp_grad): the layer is re-evaluated inside the backward kernel, so only
    the inputs are kept (not even the output: the kernel takes the last ReLU mask from its own recompute) -- autograd over the composition keeps (B, C2, n), (B, C2 + C1, n) and one (B, C, n) per layer.
    Gradients: known_feats, skip, every W and b; dist, w3 and the lengths get none (as the reference's ThreeNN / ThreeInterpolate)."""

    @staticmethod
    def forward(ctx, be, rule, idx, dist, w3, ulen, known_feats, skip, *wb):
        known_feats, skip, *wb = [_det(t) for t in (known_feats, skip, *wb)]
        packed, widths = fp_mlp_pack_weights(_pairs(wb), known_feats.shape[-1])
        out = be.fp_mlp(known_feats, skip, idx, dist, packed, widths, rule=rule, w3=w3, unknown_lengths=ulen)
        ctx.be, ctx.rule, ctx.has_skip = be, rule, skip is not None
        ctx.save_for_backward(idx, dist, w3, ulen, known_feats, skip, *wb)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        idx, dist, w3, ulen, known_feats, skip, *wb = ctx.saved_tensors
        d_known, d_skip, d_w, d_b, _ = ctx.be.fp_mlp_grad(known_feats, skip, idx, dist, _pairs(wb), grad_out, rule=ctx.rule, w3=w3, unknown_lengths=ulen,
                                                          want_known=ctx.needs_input_grad[6])
        return (None, None, None, None, None, None, d_known, d_skip if ctx.needs_input_grad[7] else None, *_flat(zip(d_w, d_b)))


# ---- feature-propagation layer with training-mode BatchNorm (csrc/fp_mlp_bn.hip) ----
def fp_mlp_bn_supported(c2, c1, widths):
    """The shapes mcp_fp_mlp_bn_forward / _backward are built for: every shape of mcp_fp_mlp."""
    return fp_mlp_supported(c2, c1, widths)


# Shape classes (c2, c1, widths) -> fewest rows B * n at which the module's fused training-mode route (three_nn, transpositions,
# mcp_fp_mlp_bn_forward, mcp_fp_mlp_bn_backward, the running-statistics update) measured faster, forward + backward, than the
# composition's forward + backward by more than the composition's own spread (tools/fp_mlp_bn_times.py ->
# profiles/fp_mlp_bn_times.json).  A class without a row keeps the composition.  Measured at B = 8 in train() (ms, forward +
# backward): 256 + 3 -> 256/256 over n = 16384 (3.304 against 3.692, spread 0.076) enters; 256 + 128 -> 256/256 over n = 1024 (1.139
# against 0.922) and 128 + 4 -> 128/128/128 over n = 4096 (1.483 against 1.334) are slower and stay out.
FP_MLP_BN_FUSED_CLASSES = {(256, 3, (256, 256)): 8 * 16384}


def fp_mlp_bn_routes_fused(c2, c1, widths, rows):
    """PointnetFPModule's route predicate under a training-mode BatchNorm: a pure function of the padded shapes."""
    return _routes(FP_MLP_BN_FUSED_CLASSES, fp_mlp_class(c2, c1, widths), rows)


def _bn_layer_outputs(ctx, out, mean, var, count):
    """What the forward of a *BnLayerFn returns: out, per layer (mean, biased variance), the live count; all but out are marked
    non-differentiable."""
    stats = _flat(zip(mean, var))
    ctx.mark_non_differentiable(*stats, count)
    return (out, *stats, count)


def _bn_layer_saved(ctx, own):
    """The saved tensors of a *BnLayerFn cut back: its `own` leading inputs, then [(W, b, gamma, beta), ...], [mean_l], [rstd_l]."""
    saved, L = ctx.saved_tensors, ctx.layers
    return (*saved[:own], _quads(saved[own:own + 4 * L]), saved[own + 4 * L:own + 5 * L], saved[own + 5 * L:])


class _FpMlpBnLayerFn(torch.autograd.Function):
    """mcp_fp_mlp_bn_forward with its hand-written backward (mcp_fp_mlp_bn_backward).  Kept between the two: the inputs and the
    per-layer (mean, rstd) -- no activation; the backward runs the forward passes again with the statistics given.  Outputs: out, then
    per layer (mean, biased variance), then the live count; all but out are marked non-differentiable.  Gradients: known_feats, skip,
    every W, b, gamma and beta; dist, w3 and the lengths get none."""

    @staticmethod
    def forward(ctx, be, rule, idx, dist, w3, ulen, eps, known_feats, skip, *params):
        known_feats, skip, *params = [_det(t) for t in (known_feats, skip, *params)]
        layers = _quads(params)
        out, mean, var, rstd, count = be.fp_mlp_bn_forward(known_feats, skip, idx, dist, layers, eps, rule=rule, w3=w3, unknown_lengths=ulen)
        ctx.be, ctx.rule, ctx.layers = be, rule, len(layers)
        ctx.save_for_backward(idx, dist, w3, ulen, known_feats, skip, *params, *mean, *rstd)
        return _bn_layer_outputs(ctx, out, mean, var, count)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, *_):
        idx, dist, w3, ulen, known_feats, skip, layers, mean, rstd = _bn_layer_saved(ctx, 6)
        d_known, d_skip, d_layers = ctx.be.fp_mlp_bn_backward(known_feats, skip, idx, dist, layers, mean, rstd, grad_out, rule=ctx.rule, w3=w3,
                                                              unknown_lengths=ulen, want_known=ctx.needs_input_grad[7])
        return (None, None, None, None, None, None, None, d_known, d_skip if ctx.needs_input_grad[8] else None, *_flat(d_layers))


# ---- set-abstraction layer with training-mode BatchNorm (csrc/group_mlp_bn.hip) ----
def group_mlp_bn_supported(c, widths, nsample=1, use_xyz=True):
    """The shapes mcp_group_mlp_bn_forward / _backward are built for: every shape of mcp_group_mlp (no row_bias)."""
    return group_mlp_supported(c, widths, nsample, use_xyz)


def group_mlp_bn_packed_floats(c, widths, use_xyz=True):
    """Floats of mcp_group_mlp_bn_pack's image, one for both directions: per layer 32-channel output tiles x k-steps x 3 pieces x 64
    lanes x 16 B (layer 1: the k-steps of c + 3 contiguous columns), the biases, then the transposed slabs -- for l = L .. 2 two
    k-steps per tile of gz_l into the tiles of layer l - 1, then those of gz_1 into the ceil((c + 3) / 32) tiles of dx."""
    tiles = [w // 32 for w in widths]
    cin = c + (3 if use_xyz else 0)
    ks = [(cin + 15) // 16] + [w // 16 for w in widths[:-1]]
    fwd = sum(t * k for t, k in zip(tiles, ks))
    bwd = sum(2 * tiles[l] * tiles[l - 1] for l in range(1, len(tiles))) + 2 * tiles[0] * ((cin + 31) // 32)
    return (fwd + bwd) * 3 * 64 * 4 + sum(widths)


# Shape classes (column group 8 | 16 | 32 | 64, feature channels, widths) -> fewest centres B * M at which the module's fused
# training-mode route (ball query, transposition, mcp_group_mlp_bn_forward, mcp_group_mlp_bn_backward, the running-statistics update)
# measured faster, forward + backward, than the composition's forward + backward by more than the composition's own spread
# (tools/group_mlp_bn_times.py -> profiles/group_mlp_bn_times.json).  A class without a row keeps the composition.
# Measured at B = 8 in train() (ms, forward + backward, composition first / fused / composition again): 16384 -> 1024 / ns 16 / 4 ->
# 32/32/64 1.224 / 1.326 / 1.299 (spread 0.897), 1024 -> 256 / ns 16 / 64 -> 64/64/128 1.115 / 1.179 / 1.170 (spread 0.261), 256 -> 64 /
# ns 8 / 128 -> 128/128/256 1.370 / 1.373 / 1.445 (spread 0.319): the fused route is 8 %, 6 % and 0.3 % slower than the composition's
# first row, inside the composition's own spread everywhere, and no class enters.  What the route does change is the memory the
# forward keeps for the backward: 4.7 MB against 144.7 MB at the first level.  Largest relative gradient difference between the
# routes: 3.6e-06.
# The table ships empty, as its two siblings do: filling it changes what existing callers run and is a change of its own.
GROUP_MLP_BN_FUSED_CLASSES = {}


def group_mlp_bn_routes_fused(c, widths, nsample, centres):
    """PointnetSAModuleMSG's route predicate under a training-mode BatchNorm: a pure function of the padded shapes."""
    return _routes(GROUP_MLP_BN_FUSED_CLASSES, group_mlp_class(c, widths, nsample), centres)


def group_mlp_bn_pack_weights(weights, use_xyz=True):
    """mcp_group_mlp_bn_pack's image from the unfolded [(W (out, in), b (out,)), ...] fp32 device tensors -> (packed, widths)."""
    c, xyz = int(weights[0][0].shape[1]) - (3 if use_xyz else 0), int(bool(use_xyz))
    return _pack_image("group_mlp_bn", (c, xyz), f"c={c}", c >= 0, weights, grad_alloc=True)


class _GroupMlpBnLayerFn(torch.autograd.Function):
    """mcp_group_mlp_bn_forward with its hand-written backward (mcp_group_mlp_bn_backward).  Kept between the two: the inputs and the
    per-layer (mean, rstd) -- no activation; the backward runs the forward passes again with the statistics given.  Outputs: out, then
    per layer (mean, biased variance), then the live count; all but out are marked non-differentiable.  Gradients: xyz, new_xyz,
    features, every W, b, gamma and beta; idx and the lengths get none."""

    @staticmethod
    def forward(ctx, be, pool, use_xyz, idx, ql, eps, xyz, new_xyz, features, *params):
        xyz, new_xyz, features, *params = [_det(t) for t in (xyz, new_xyz, features, *params)]
        layers = _quads(params)
        out, mean, var, rstd, count = be.group_mlp_bn_forward(xyz, new_xyz, features, idx, layers, eps, pool=pool, use_xyz=use_xyz, new_xyz_lengths=ql)
        ctx.be, ctx.pool, ctx.use_xyz, ctx.layers = be, pool, use_xyz, len(layers)
        ctx.save_for_backward(idx, ql, xyz, new_xyz, features, *params, *mean, *rstd)
        return _bn_layer_outputs(ctx, out, mean, var, count)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, *_):
        idx, ql, xyz, new_xyz, features, layers, mean, rstd = _bn_layer_saved(ctx, 5)
        need = ctx.needs_input_grad
        d_feat, d_xyz, d_new, d_layers = ctx.be.group_mlp_bn_backward(
            xyz, new_xyz, features, idx, layers, mean, rstd, grad_out, pool=ctx.pool, use_xyz=ctx.use_xyz, new_xyz_lengths=ql,
            want_features=need[8] and features is not None, want_xyz=need[6] and ctx.use_xyz, want_new_xyz=need[7] and ctx.use_xyz)
        if not ctx.use_xyz:
            d_xyz, d_new = _unused_zeros(xyz, need[6]), _unused_zeros(new_xyz, need[7])
        return (None, None, None, None, None, None, d_xyz, d_new, d_feat, *_flat(d_layers))


class _ChamferLengthsFn(torch.autograd.Function):
    """_ChamferFn over the valid prefixes of a padded batch (pytorch3d's x_lengths / y_lengths with its default reductions):
    value_b = sum_{i<xl} dxy_i / max(xl,1) + sum_{j<yl} dyx_j / max(yl,1).  Forward: the length-aware search returns 0 for every
    padded row, so the sums run over whole rows.  Backward: the same row gather and deterministic segmented scatter as _ChamferFn;
    the direct term of a padded row -- and of every row when the other cloud is empty -- is set to an exact zero, so what the
    scatter adds through those rows' index 0 is zero, and no padded coordinate reaches a gradient."""

    @staticmethod
    def forward(ctx, be, x, y, xl, yl):
        x, y = x.detach().contiguous(), y.detach().contiguous()
        B, N, _ = x.shape
        M = y.shape[1]
        with be.cloud_scope():   # where the searches prune, a cloud that is query here and reference there is sorted once
            ixy, dxy = be.knn(x, y, 1, mode=MCP_DIST_DIRECT, return_dist=True, query_lengths=xl, ref_lengths=yl)
            iyx, dyx = be.knn(y, x, 1, mode=MCP_DIST_DIRECT, return_dist=True, query_lengths=yl, ref_lengths=xl)
        xe, ye = _valid_counts(xl, B, N, x.device), _valid_counts(yl, B, M, x.device)
        xden, yden = xe.clamp(min=1).float(), ye.clamp(min=1).float()
        both = ((xe > 0) & (ye > 0)).view(B, 1, 1)
        xrow = (torch.arange(N, device=x.device).view(1, N, 1) < xe.view(B, 1, 1)) & both   # rows with a neighbour to point at
        yrow = (torch.arange(M, device=x.device).view(1, M, 1) < ye.view(B, 1, 1)) & both
        ctx.save_for_backward(x, y, ixy, iyx, xden, yden, xrow, yrow)
        return dxy[..., 0].sum(1) / xden + dyx[..., 0].sum(1) / yden

    @staticmethod
    def backward(ctx, gv):
        x, y, ixy, iyx, xden, yden, xrow, yrow = ctx.saved_tensors
        B, N, _ = x.shape
        M = y.shape[1]
        zero = gv.new_zeros(())
        gx_d = torch.where(xrow, (x - _group_rows_fwd(y, ixy).squeeze(2)) * (gv * 2.0 / xden).view(B, 1, 1), zero)
        gy_d = torch.where(yrow, (y - _group_rows_fwd(x, iyx).squeeze(2)) * (gv * 2.0 / yden).view(B, 1, 1), zero)
        gx = gx_d - _group_rows_grad(gy_d.unsqueeze(2), iyx, N) if ctx.needs_input_grad[1] else None
        gy = gy_d - _group_rows_grad(gx_d.unsqueeze(2), ixy, M) if ctx.needs_input_grad[2] else None
        return None, gx, gy, None, None


class _PtblockFn(torch.autograd.Function):
    """mcp_ptblock_attention with its hand-written backward (mcp_ptblock_grad): the block re-evaluated in the backward kernel, the
    per-neighbour gradients through the deterministic segmented scatter (one sort serves xyz, k and v), weight gradients fixed-order."""

    @staticmethod
    def forward(ctx, be, idx, xyz, q, k, v, *weights):
        xyz = xyz.detach().contiguous()
        q, k, v = q.detach(), k.detach(), v.detach()
        if not (q.stride() == k.stride() == v.stride() and q.stride(2) == 1 and q.stride(0) == q.shape[1] * q.stride(1)):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ws = [t.detach().contiguous() for t in weights]
        ctx.save_for_backward(idx, xyz, q, k, v, *ws)
        return be.ptblock_attention(xyz, q, k, v, idx, be.ptblock_pack(*ws))

    @staticmethod
    def backward(ctx, grad_out):
        idx, xyz, q, k, v, *ws = ctx.saved_tensors
        B, N, C = q.shape
        lib, dev = _lib.load(), q.device
        grad_out = grad_out.contiguous()
        d_xyz_c = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        d_xyz_rows = torch.empty((B, N, 16, 3), dtype=torch.float32, device=dev)
        d_q = torch.empty((B, N, C), dtype=torch.float32, device=dev)
        d_k_rows = torch.empty((B, N, 16, C), dtype=torch.float32, device=dev)
        d_v_rows = torch.empty((B, N, 16, C), dtype=torch.float32, device=dev)
        d_w = torch.empty((lib.mcp_ptblock_grad_floats(),), dtype=torch.float32, device=dev)
        need = lib.mcp_ptblock_grad_workspace_bytes(B, N)
        wsp = torch.empty((need,), dtype=torch.uint8, device=dev)
        _call("mcp_ptblock_grad", q, B, N, C, 16, q.stride(1), _lib.fptr(xyz), q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.iptr(idx),
              *[_lib.fptr(t) for t in ws], _lib.fptr(grad_out), _lib.fptr(d_xyz_c), _lib.fptr(d_xyz_rows), _lib.fptr(d_q), _lib.fptr(d_k_rows),
              _lib.fptr(d_v_rows), _lib.fptr(d_w), wsp.data_ptr(), need)
        segments = _scatter_segments(idx, N)
        d_xyz = d_xyz_c + _group_rows_grad(d_xyz_rows, idx, N, segments) if ctx.needs_input_grad[2] else None
        d_k = _group_rows_grad(d_k_rows, idx, N, segments) if ctx.needs_input_grad[4] else None
        d_v = _group_rows_grad(d_v_rows, idx, N, segments) if ctx.needs_input_grad[5] else None
        return (None, None, d_xyz, d_q, d_k, d_v, *_split_flat(d_w, ws))


def _scatter_lists(ia, ib, lens, n):
    """The fusion layer's neighbour list(s) as the segmented scatter of grad_nb (B,N,64,3) sorts them.  With lengths a padded point's
    rows of grad_nb are zeros and its list rows may hold anything -- the searches leave 0 there, so every padded entry of an element
    would land on row 0 and ONE thread of the reduction would walk them all (24 x 8192 points at half lengths: 186 ms against 0.43 ms,
    profiles/fusion_lengths_times.json; the effect _PointConvAggFn documents): padded point i names row i mod n instead
    (grad.spread_padded_rows).  Zeros land elsewhere: no sum changes."""
    idx = ia if ib is None else torch.cat((ia, ib), dim=-1)
    if lens is None:
        return idx
    return grad.spread_padded_rows(idx, grad.live_points(lens, idx.shape[0], idx.shape[1], idx.device), n)


def _fusion_lead(p1, p2, idx, lens, conv, null_lens=False):
    """The arguments every fusion entry starts with: B, N, the neighbours per point, p1, p2, the list(s), [the lengths,] and the
    tensors of conv (w1 .. b3, and what the entry takes right after them).  The length pointer stands there when there are lengths:
    the dense entries have no such argument -- or, null_lens, always (mcp_fusion_grad_lengths, which takes NULL)."""
    ia, ib, nb = _two_lists(idx)
    B, N, _ = p1.shape
    return (B, N, nb, _lib.fptr(p1), _lib.fptr(p2), _lib.iptr(ia), _opt(ib, _lib.iptr), *((_len_ptr(lens),) if null_lens or lens is not None else ()),
            *[_lib.fptr(t) for t in conv])


class _FusionBNFn(torch.autograd.Function):
    """The fusion layer of one reference call on BATCH statistics (net.train()), forward and backward on the multi-pass kernels of
    csrc/fusion_bn.hip.  Returns (out, bn, var): bn = per layer mean | rstd | gamma | beta, var = the biased batch variances (both
    non-differentiable by-products for the caller's running-estimate update); with per-cloud lengths (csrc/fusion_bn_lengths.hip)
    (out, bn, var, count)."""

    @staticmethod
    def forward(ctx, be, eps, ia, ib, lens, p1, p2, w1, b1, w2, b2, w3, b3, g1, e1, g2, e2, g3, e3):
        conv = [t.detach().contiguous() for t in (w1, b1, w2, b2, w3, b3)]
        p1, p2 = p1.detach().contiguous(), p2.detach().contiguous()
        ctx.has_lengths = lens is not None
        ctx.kept = lens is None or be.FUSION_BN_KEEP_SCORES_WITH_LENGTHS
        saved = ()
        if ctx.kept:
            rows = p1.shape[0] * p1.shape[1] * 64
            # kept for the backward: every neighbour's score, its layer-3 channel and zhat3 there (12 bytes per row) -- the backward's
            # first pass then has no layer to re-evaluate
            saved = (torch.empty((rows,), dtype=torch.int32, device=p1.device), torch.empty((rows,), dtype=torch.float32, device=p1.device),
                     torch.empty((rows,), dtype=torch.float32, device=p1.device))
        res = be.fusion_bn_forward(p1, p2, ia if ib is None else (ia, ib), conv, (g1, e1, g2, e2, g3, e3), eps, saved=saved or None, lengths=lens)
        ctx.save_for_backward(ia, ib, p1, p2, *conv, res[1], *(() if lens is None else (lens,)), *saved)
        ctx.mark_non_differentiable(*res[1:])
        return res   # (out, bn, var), with lengths (out, bn, var, count)

    @staticmethod
    def backward(ctx, grad_out, _gbn, _gvar, _gcount=None):
        ia, ib, p1, p2, *conv, bn = ctx.saved_tensors[:11]   # conv = (w1, b1, w2, b2, w3, b3)
        rest = ctx.saved_tensors[11:]
        lens = rest[0] if ctx.has_lengths else None
        save_c, save_z, save_s = rest[-3:] if ctx.kept else (None, None, None)
        B, N, _ = p1.shape
        rows = B * N * 64
        lib, dev = _lib.load(), p1.device
        grad_out = grad_out.contiguous()
        row_c = torch.empty((rows,), dtype=torch.int32, device=dev)
        row_dy, row_a = torch.empty((rows,), dtype=torch.float32, device=dev), torch.empty((rows,), dtype=torch.float32, device=dev)
        dy2, dy1 = torch.empty((rows, 64), dtype=torch.float32, device=dev), torch.empty((rows, 64), dtype=torch.float32, device=dev)
        d_p1 = torch.empty_like(p1)
        d_nb = torch.empty((B, N, 64, 3), dtype=torch.float32, device=dev)
        d_w = torch.empty((lib.mcp_fusion_grad_floats(),), dtype=torch.float32, device=dev)
        d_aff = torch.empty((512,), dtype=torch.float32, device=dev)
        need = lib.mcp_fusion_bn_grad_workspace_bytes(B, N)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        scratch = (_lib.iptr(row_c), _lib.fptr(row_dy), _lib.fptr(row_a), _lib.fptr(dy2), _lib.fptr(dy1), _lib.fptr(d_p1), _lib.fptr(d_nb), _lib.fptr(d_w),
                   _lib.fptr(d_aff), ws.data_ptr(), need)
        if lens is not None:   # (the condition under which _fusion_lead passes the length pointer)
            entry = "mcp_fusion_bn_backward_saved_lengths" if ctx.kept else "mcp_fusion_bn_backward_lengths"
        else:
            entry = "mcp_fusion_bn_backward_saved"
        keep = (_lib.iptr(save_c), _lib.fptr(save_z), _lib.fptr(save_s)) if ctx.kept else ()
        _call(entry, p1, *_fusion_lead(p1, p2, (ia, ib), lens, (*conv, bn, grad_out)), *keep, *scratch)
        d_p2 = None
        if ctx.needs_input_grad[6]:
            d_p2 = _group_rows_grad(d_nb, _scatter_lists(ia, ib, lens, p2.shape[1]), p2.shape[1])
        aff = [d_aff[0:64], d_aff[64:128], d_aff[128:192], d_aff[192:256], d_aff[256:384], d_aff[384:512]]
        return (None, None, None, None, None, d_p1, d_p2, *_split_flat(d_w, conv), *aff)


class _BNBatchFn(torch.autograd.Function):
    """BatchNorm on batch statistics of x (G,F,N,C), each group alone, with per-group lengths (csrc/bn_batch.hip), forward and
    backward.  Returns (y, mean, var, count); the last three are non-differentiable by-products for the caller's running-estimate
    update.  Kept for the backward: x, mean, var and the lengths -- xhat is formed again."""

    @staticmethod
    def forward(ctx, eps, lens, x, weight, bias):
        lib = _lib.load()
        x, weight, bias = x.detach().contiguous(), weight.detach().contiguous(), bias.detach().contiguous()
        G, Fr, N, C = x.shape
        dev = x.device
        mean, var = torch.empty((G, C), dtype=torch.float32, device=dev), torch.empty((G, C), dtype=torch.float32, device=dev)
        count = torch.empty((G,), dtype=torch.int32, device=dev)
        y = torch.empty_like(x)
        need = lib.mcp_bn_batch_workspace_bytes(G, Fr, N, C)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        _call("mcp_bn_batch_forward", x, G, Fr, N, C, _lib.fptr(x), None if lens is None else _lib.iptr(lens), _lib.fptr(weight), _lib.fptr(bias), float(eps),
              _lib.fptr(mean), _lib.fptr(var), _lib.iptr(count), _lib.fptr(y), ws.data_ptr(), need)
        ctx.eps, ctx.has_lengths = float(eps), lens is not None
        ctx.save_for_backward(x, weight, mean, var, *(() if lens is None else (lens,)))
        ctx.mark_non_differentiable(mean, var, count)
        return y, mean, var, count

    @staticmethod
    def backward(ctx, grad_y, _gmean, _gvar, _gcount):
        x, weight, mean, var = ctx.saved_tensors[:4]
        lens = ctx.saved_tensors[4] if ctx.has_lengths else None
        lib = _lib.load()
        G, Fr, N, C = x.shape
        dev = x.device
        grad_y = grad_y.contiguous()
        d_x = torch.empty_like(x)
        d_gamma, d_beta = torch.empty((C,), dtype=torch.float32, device=dev), torch.empty((C,), dtype=torch.float32, device=dev)
        need = lib.mcp_bn_batch_workspace_bytes(G, Fr, N, C)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        _call("mcp_bn_batch_backward", x, G, Fr, N, C, _lib.fptr(x), None if lens is None else _lib.iptr(lens), _lib.fptr(weight), _lib.fptr(mean),
              _lib.fptr(var), ctx.eps, _lib.fptr(grad_y), _lib.fptr(d_x), _lib.fptr(d_gamma), _lib.fptr(d_beta), ws.data_ptr(), need)
        return None, None, d_x, d_gamma, d_beta


class _FusionFn(torch.autograd.Function):
    """mcp_fusion with its hand-written backward (mcp_fusion_grad): the layer is re-evaluated inside the backward kernel, the
    neighbour gradients go through the deterministic segmented scatter, weight gradients are fixed-order sums.
    lens: (B,) int32 device tensor or None -- per-cloud lengths, carried to the backward.  Both directions call the *_lengths entries
    (csrc/fusion_lengths.hip): with null lengths those are the dense entries themselves."""

    @staticmethod
    def forward(ctx, be, ia, ib, lens, p1, p2, w1, b1, w2, b2, w3, b3):
        args = [t.detach().contiguous() for t in (p1, p2, w1, b1, w2, b2, w3, b3)]
        ctx.save_for_backward(ia, ib, *args, lens)
        return be._fusion_mlp(args[0], args[1], ia if ib is None else (ia, ib), *args[2:], lens=lens)

    @staticmethod
    def backward(ctx, grad_out):
        ia, ib, p1, p2, *conv, lens = ctx.saved_tensors   # conv = (w1, b1, w2, b2, w3, b3)
        B, N, _ = p1.shape
        lib = _lib.load()
        grad_out = grad_out.contiguous()
        d_p1 = torch.empty_like(p1)
        d_nb = torch.empty((B, N, 64, 3), dtype=torch.float32, device=p1.device)
        d_w = torch.empty((lib.mcp_fusion_grad_floats(),), dtype=torch.float32, device=p1.device)
        need = lib.mcp_fusion_grad_workspace_bytes(B, N)
        ws = torch.empty((need,), dtype=torch.uint8, device=p1.device)
        _call("mcp_fusion_grad_lengths", p1, *_fusion_lead(p1, p2, (ia, ib), lens, (*conv, grad_out), null_lens=True), _lib.fptr(d_p1),
              _lib.fptr(d_nb), _lib.fptr(d_w), ws.data_ptr(), need)
        d_p2 = None
        if ctx.needs_input_grad[5]:
            d_p2 = _group_rows_grad(d_nb, _scatter_lists(ia, ib, lens, p2.shape[1]), p2.shape[1])
        return (None, None, None, None, d_p1, d_p2, *_split_flat(d_w, conv))


# ---- the fused point layers' entries: each family's argument checks and leading arguments, stated once ----
def _check_grad_out(name, grad_out, shape):
    if tuple(grad_out.shape) != shape:
        raise RuntimeError(f"{name}: grad_out {tuple(grad_out.shape)}, expected {shape}")


def _group_check(name, xyz, new_xyz, features, idx, layers, use_xyz, grad_out=None):
    """The checks of the set-abstraction entries that take the layers themselves, [(W, b), ...] or [(W, b or None, gamma or None, beta
    or None), ...] -> ((B, N, M, C, nsample), widths).  grad_out: the _grad entry's, checked where it always was; the layer shapes
    of that entry are checked once, when its image is built (group_mlp_grad_pack_weights)."""
    B, N, _ = xyz.shape
    M, nsample = new_xyz.shape[1], idx.shape[2]
    C = 0 if features is None else features.shape[2]
    if tuple(idx.shape[:2]) != (B, M) or (features is not None and tuple(features.shape[:2]) != (B, N)):
        raise RuntimeError(f"{name}: idx {tuple(idx.shape)} / features do not match B={B}, N={N}, M={M}")
    widths = [int(l[0].shape[0]) for l in layers]
    cin = C + (3 if use_xyz else 0)
    if not group_mlp_supported(C, widths, nsample, use_xyz) or int(layers[0][0].shape[1]) != cin:   # (the _grad and _bn kernels take every shape of it)
        raise _lib.Unsupported(f"{name}: unsupported shape c={C} widths={widths} nsample={nsample}")
    if grad_out is not None:
        _check_grad_out(name, grad_out, (B, M, widths[-1]))
    else:
        _check_layers(name, layers, cin, widths)
    if B == 0 or N == 0 or M == 0:
        raise RuntimeError(f"{name}: empty batch, cloud or centre list")
    return (B, N, M, C, nsample), widths


def _group_lead(dims, pool, use_xyz, wid, xyz, new_xyz, features, idx, ql):
    """What mcp_group_mlp, mcp_group_mlp_grad, mcp_group_mlp_bn_forward and mcp_group_mlp_bn_backward take first: dims = (B, N, M, C,
    nsample), the flags, the widths, the clouds, the features, the list and the centre lengths."""
    return (*dims, int(bool(use_xyz)), GROUP_MLP_POOLS[pool], len(wid), wid, _lib.fptr(xyz), _lib.fptr(new_xyz), _opt(features), _lib.iptr(idx),
            _len_ptr(ql))


def _fp_check(name, known_feats, skip, idx, dist, rule, w3, layers, widths=None, grad_out=None):
    """The checks of the feature-propagation entries -> ((B, n, m, C2, C1, rule code), widths).  layers: [(W, b), ...] or [(W, b or None,
    gamma or None, beta or None), ...]; None for the eval call, which has an image and `widths` instead and takes an empty batch.
    grad_out: the _grad entry's, checked where it always was; the layer shapes of that entry are checked once, when its image is
    built (fp_mlp_grad_pack_weights)."""
    B, m, C2 = known_feats.shape
    n = idx.shape[1]
    C1 = 0 if skip is None else skip.shape[2]
    code = FP_MLP_RULES[rule]
    if tuple(idx.shape) != (B, n, 3) or (skip is not None and tuple(skip.shape[:2]) != (B, n)):
        raise RuntimeError(f"{name}: idx {tuple(idx.shape)} / skip do not match B={B}, n={n}")
    what, t = ("w3", w3) if code == 0 else ("dist", dist)
    if t is None or tuple(t.shape) != (B, n, 3):
        raise RuntimeError(f"{name}: rule {rule!r} needs {what} of shape {(B, n, 3)}")
    if layers is not None:
        widths = [int(l[0].shape[0]) for l in layers]
    if not fp_mlp_supported(C2, C1, widths) or (layers is not None and int(layers[0][0].shape[1]) != C2 + C1):   # (_grad, _bn: every shape of it)
        raise _lib.Unsupported(f"{name}: unsupported shape c2={C2} c1={C1} widths={widths}")
    if layers is not None:
        if grad_out is not None:
            _check_grad_out(name, grad_out, (B, n, widths[-1]))
        else:
            _check_layers(name, layers, C2 + C1, widths)
        if B == 0 or n == 0 or m == 0:
            raise RuntimeError(f"{name}: empty batch, unknown or known cloud")
    return (B, n, m, C2, C1, code), widths


def _fp_lead(dims, wid, known_feats, skip, idx, dist, w3, ul, packed):
    """What mcp_fp_mlp, mcp_fp_mlp_grad, mcp_fp_mlp_bn_forward and mcp_fp_mlp_bn_backward take first: dims = (B, n, m, C2, C1, rule code),
    the widths, the features, the skip rows (NULL without channels), the list, dist or -- rule "given" -- w3, the lengths, the image."""
    C1, code = dims[4], dims[5]
    return (*dims, len(wid), wid, _lib.fptr(known_feats), None if C1 == 0 else _lib.fptr(skip), _lib.iptr(idx), None if code == 0 else _lib.fptr(dist),
            _lib.fptr(w3) if code == 0 else None, _len_ptr(ul), _lib.fptr(packed))


def _bn_pairs(layers):
    """[(W, b), ...] of [(W, b or None, gamma, beta), ...] for the operand image: zeros stand for an absent bias."""
    return [(w, torch.zeros_like(w[:, 0]) if b is None else b) for w, b, _, _ in layers]


def _bn_affine(layers):
    """The host arrays of the layers' gamma and beta pointers (NULL where a layer has none)."""
    return _ptr_array([g for _, _, g, _ in layers]), _ptr_array([bt for _, _, _, bt in layers])


def _bn_eps(name, eps, layers):
    if len(eps) != len(layers) or not all(float(e) > 0 for e in eps):
        raise RuntimeError(f"{name}: one eps > 0 per layer")
    return (ctypes.c_float * len(eps))(*[float(e) for e in eps])


def _bn_grads(layers, dev):
    """One gradient buffer per parameter that is there -> ([(dW, db or None, dgamma or None, dbeta or None), ...], the four host arrays of
    their pointers)."""
    d_layers = [tuple(None if t is None else _grad_empty(tuple(t.shape), torch.float32, dev) for t in layer) for layer in layers]
    return d_layers, [_ptr_array([d[i] for d in d_layers]) for i in range(4)]


class HipBackend:
    name = "hip"

    def fps(self, xyz, npoint, with_points=False, lengths=None):
        """furthest_point_sample (pointnet2_utils.py:10-29): xyz (B,N,3) -> (B,npoint) int32.  with_points: also the sampled
        coordinates (B,npoint,3) -- the index_points_gather that follows in every caller -- from the same launch.
        lengths (pytorch3d's sample_farthest_points(points, lengths, K); forms: lengths_tensor): element b is the cloud
        xyz[b, :lengths[b]] alone -- its row is bit for bit the sampling of that slice (the reference keeps selecting when
        npoint > lengths[b]), an empty element gives index 0 and coordinates 0.0, and rows at or beyond a length are never read.
        Without lengths nothing changes."""
        xyz = xyz.detach()
        B, N, _ = xyz.shape
        if lengths is not None:
            lens = lengths_tensor(lengths, B, N, xyz.device)
            out = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
            pts = torch.empty((B, npoint, 3), dtype=torch.float32, device=xyz.device) if with_points else None
            # what the fastest form for this padded shape uses: the tiled kernel's sorted cloud (16384 < N <= 65536), the streaming
            # form's running distances beyond, 0 up to 16384 (mcp_fps_lengths_form names the form the call then takes)
            need = _lib.load().mcp_fps_lengths_pruned_workspace_bytes(B, N, npoint)
            ws = torch.empty((need,), dtype=torch.uint8, device=xyz.device) if need else None
            _call("mcp_furthest_point_sampling_lengths", xyz, B, N, npoint, _lib.fptr(xyz), _lib.iptr(lens), _lib.iptr(out),
                  None if pts is None else _lib.fptr(pts), ws.data_ptr() if need else None, need)
            return (out, pts) if with_points else out
        out = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
        need = _lib.load().mcp_fps_workspace_bytes(B, N, npoint)  # scratch for the tiled kernel (16384 < N <= 65536), else 0
        ws = torch.empty((need,), dtype=torch.uint8, device=xyz.device) if need else None
        if N <= 65536:  # a fresh sampling: the running distances stay inside the kernel (no (B,N) buffer to fill)
            pts = torch.empty((B, npoint, 3), dtype=torch.float32, device=xyz.device) if with_points else None
            try:
                _call("mcp_furthest_point_sampling_fresh", xyz, B, N, npoint, _lib.fptr(xyz), _lib.iptr(out), None if pts is None else _lib.fptr(pts),
                      ws.data_ptr() if need else None, need)
                return (out, pts) if with_points else out
            except _lib.Unsupported:  # only the streaming kernel applies to this shape: it keeps its running distances in temp
                pass
        temp = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
        _call("mcp_furthest_point_sampling_ws", xyz, B, N, npoint, _lib.fptr(xyz), _lib.fptr(temp), _lib.iptr(out),
              ws.data_ptr() if need else None, need)
        return (out, self.group_rows(xyz, out)) if with_points else out

    # clouds at least this large go through the Morton-sorted, box-pruned search (same results)
    # (plain attributes: A/B tools set them on the class; the package reads no tuning variables from the environment)
    PRUNE_MIN_REFS = 2048
    PRUNE_MIN_QUERIES = 1024
    # the same rule for a search with per-cloud lengths, on the PADDED sizes (the host never reads a length).  Its constants are the
    # smallest class measured to win WITH both cloud builds (profiles/knn_pruned_lengths_times.json): at 8 x 8192 x 8192 the pruned
    # route takes 0.099 ms against the exhaustive 0.144 (K = 1) and 0.113-0.145 against 0.216-0.377 (K = 32); at 8 x 2048 x 4096 it
    # loses, 0.065 against 0.037 and 0.072 against 0.056, as at 8 x 1024 x 2048 (two builds cost more than the whole exhaustive
    # search there).  Nothing in between is measured, so it stays exhaustive.
    PRUNE_LENGTHS_MIN_REFS = 8192
    PRUNE_LENGTHS_MIN_QUERIES = 8192

    @classmethod
    def prunes_with_lengths(cls, Q, N, k):
        """Whether a search with lengths of (B,Q,3) queries in (B,N,3) references takes the pruned route: a pure function of the
        padded shapes and k (the candidate lists hold 16-bit indices: N <= 65536)."""
        return cls.PRUNE_LENGTHS_MIN_REFS <= N <= 65536 and Q >= cls.PRUNE_LENGTHS_MIN_QUERIES and k <= 32

    def __init__(self):
        # .scope: {key: (tensor, sorted cloud, stream, built-event, lengths tensor or None)} while a cloud_scope is open
        self._tls = threading.local()
        self._tile = None

    @property
    def TILE(self):
        if self._tile is None:
            self._tile = _lib.load().mcp_knn_tile_size()
        return self._tile

    @contextlib.contextmanager
    def cloud_scope(self, seed=None):
        """Within this context the Morton-sorted form of a cloud is built once per tensor and reused by every search on it
        (the model searches the same clouds many times per forward).  The caller promises not to write into a cloud tensor
        while the scope is open -- model.forward opens one per call and never does.  Entries hold a strong reference to their
        tensor, so its storage cannot be recycled under the key; the scope is per thread and dropped on exit.  Outside a scope
        nothing is cached: every search rebuilds (one extra launch), so buffers a caller reuses between calls are always safe.
        seed: a dict to use as this scope's table (MoCoPCI.prefetch fills one ahead of the forward that then opens its scope on
        it); a seeded scope replaces an enclosing one until it exits."""
        outer = getattr(self._tls, "scope", None)
        self._tls.scope = seed if seed is not None else ({} if outer is None else outer)
        try:
            yield
        finally:
            self._tls.scope = outer

    def _build_cloud(self, xyz, lens=None):
        """lens: (B,) int32 device lengths (lengths_tensor) -- the sorted form of each element's first lens[b] rows, padding behind
        it in place (perm[s] = s); no padded row of xyz reaches the box, a key or a tile box."""
        B, N, _ = xyz.shape
        tiles = (N + self.TILE - 1) // self.TILE
        boxes = torch.empty((B, tiles, 6), dtype=torch.float32, device=xyz.device)
        if N <= 16384:  # one fused launch: bbox, Morton keys, in-LDS sort, gather, tile boxes
            sorted_xyz = torch.empty_like(xyz)
            perm = torch.empty((B, N), dtype=torch.int32, device=xyz.device)
            if lens is None:
                _call("mcp_build_cloud", xyz, B, N, _lib.fptr(xyz), _lib.fptr(sorted_xyz), _lib.iptr(perm), _lib.fptr(boxes))
            else:
                _call("mcp_build_cloud_lengths", xyz, B, N, _lib.fptr(xyz), _lib.iptr(lens), _lib.fptr(sorted_xyz), _lib.iptr(perm),
                      _lib.fptr(boxes))
        elif lens is not None:
            # the box over live rows only (a masked min / max: NaN or huge padding cannot leak), padding coded above every live point,
            # and a STABLE sort, so that the padding stays where it is
            live = torch.arange(N, device=xyz.device).view(1, N, 1) < lens.clamp(0, N).view(B, 1, 1)
            lo = torch.where(live, xyz, xyz.new_tensor(float("inf"))).amin(dim=1)
            hi = torch.where(live, xyz, xyz.new_tensor(float("-inf"))).amax(dim=1)
            box = torch.cat([lo, hi], dim=-1).contiguous()
            codes = torch.empty((B, N), dtype=torch.int32, device=xyz.device)
            _call("mcp_morton_codes_lengths", xyz, B, N, _lib.fptr(xyz), _lib.fptr(box), _lib.iptr(lens), _lib.iptr(codes))
            perm = torch.sort(codes, dim=1, stable=True)[1].int()
            sorted_xyz = self.group_rows(xyz, perm)   # rows beyond a length: copies of the padding, which the search never reads
            _call("mcp_tile_boxes_lengths", xyz, B, N, _lib.fptr(sorted_xyz), _lib.iptr(lens), _lib.fptr(boxes))
        else:
            box = torch.cat([xyz.amin(dim=1), xyz.amax(dim=1)], dim=-1).contiguous()
            codes = torch.empty((B, N), dtype=torch.int32, device=xyz.device)
            _call("mcp_morton_codes", xyz, B, N, _lib.fptr(xyz), _lib.fptr(box), _lib.iptr(codes))
            perm = torch.sort(codes, dim=1)[1].int()
            sorted_xyz = self.group_rows(xyz, perm)
            _call("mcp_tile_boxes", xyz, B, N, _lib.fptr(sorted_xyz), _lib.fptr(boxes))
        return sorted_xyz, perm, boxes

    def _sorted_cloud(self, xyz, lens=None):
        """Morton order of a cloud: (sorted xyz, perm int32, tile boxes); cached only inside a cloud_scope.  lens: see _build_cloud;
        the lengths tensor is part of the key (and is kept alive by the entry), so a cloud sorted under lengths is served only to
        searches with that very lengths tensor, and a length-free one only to length-free searches.  The key is the data_ptr of the
        (B,) int32 device array the kernels read: an int32 device tensor keeps its own, but lengths_tensor makes a fresh array of a
        list, a CPU tensor or an int64 device tensor on every call, so such lengths share a sorted cloud only when the caller
        converts them once (as chamfer and compat.knn_points do for their own searches) and passes the result."""
        scope = getattr(self._tls, "scope", None)
        if scope is None:
            return self._build_cloud(xyz, lens)
        cur = torch.cuda.current_stream(xyz.device)
        key = (xyz.data_ptr(), tuple(xyz.shape), xyz.device.index, None if lens is None else lens.data_ptr())
        hit = scope.get(key)
        if hit is not None:
            cloud, stream, done = hit[1:4]
            if stream != cur:  # built on another stream of this forward: order + lifetime
                cur.wait_event(done)
                for t in cloud:
                    t.record_stream(cur)
            return cloud
        cloud = self._build_cloud(xyz, lens)
        done = torch.cuda.Event()
        done.record(cur)
        scope[key] = (xyz, cloud, cur, done, lens)
        return cloud

    def _holds_cloud(self, xyz, lens=None):
        """Whether the open cloud_scope (if any) already holds the sorted form of this cloud under these lengths."""
        scope = getattr(self._tls, "scope", None)
        return scope is not None and (xyz.data_ptr(), tuple(xyz.shape), xyz.device.index, None if lens is None else lens.data_ptr()) in scope

    def prebuild_cloud(self, xyz, lengths=None):
        """Build the Morton-sorted form of a cloud now, on the current stream, when a later search of this cloud_scope will want
        it (a cloud large enough for the pruned search): lets a caller put the build on a side stream, off the critical path --
        and sends the scope's ball queries on this cloud through the pruned search.  lengths: the (B,) int32 device tensor the
        later searches will pass (the sorted cloud is keyed by it).  No-op outside a scope or for small clouds."""
        if getattr(self._tls, "scope", None) is not None and self.PRUNE_MIN_REFS <= xyz.shape[1] <= 65536:
            self._sorted_cloud(xyz.detach(), None if lengths is None else lengths_tensor(lengths, xyz.shape[0], xyz.shape[1], xyz.device))

    def knn(self, query, ref, k, mode=MCP_DIST_EXPANSION, return_dist=False, query_lengths=None, ref_lengths=None):
        """knn_point(k, ref, query) (mocopci.py:1158-1169): (B,Q,3),(B,N,3) -> (B,Q,k) int32,
        ascending by (distance, index).
        query_lengths / ref_lengths (pytorch3d's lengths1 / lengths2; see lengths_tensor for the accepted forms): element b searches
        only ref[b, :ref_lengths[b]] and only query[b, :query_lengths[b]] is live.  Live rows get what the search of the two prefixes
        on their own returns (fewer than k references: the tail repeats the last valid entry; none: index 0, distance 0); padded
        query rows get index 0 and distance 0; padded rows of either cloud are never read.  Without lengths nothing changes.
        With lengths the padded sizes choose the route (prunes_with_lengths): the pruned search over clouds sorted under their
        lengths, or the exhaustive kernels -- the same bits either way."""
        query, ref = query.detach(), ref.detach()  # an index-producing search: no gradient (pointnet2_utils.py:31-33)
        B, Q, _ = query.shape
        N = ref.shape[1]
        idx = torch.empty((B, Q, k), dtype=torch.int32, device=query.device)
        dist = torch.empty((B, Q, k), dtype=torch.float32, device=query.device) if return_dist else None
        if query_lengths is not None or ref_lengths is not None:
            ql, rl = lengths_tensor(query_lengths, B, Q, query.device), lengths_tensor(ref_lengths, B, N, query.device)
            qlp, rlp = None if ql is None else _lib.iptr(ql), None if rl is None else _lib.iptr(rl)
            if self.prunes_with_lengths(Q, N, k):
                _lib.fptr(query), _lib.fptr(ref)  # validate before building the sorted clouds
                rs, rperm, boxes = self._sorted_cloud(ref, rl)   # a side without a length: the length-free cloud
                same = query.data_ptr() == ref.data_ptr() and query.shape == ref.shape and query_lengths is ref_lengths
                qs, qperm, _ = (rs, rperm, boxes) if same else self._sorted_cloud(query, ql)
                _call("mcp_knn_pruned_lengths", query, B, Q, N, k, mode, _lib.fptr(qs), _lib.iptr(qperm), _lib.fptr(rs), _lib.iptr(rperm),
                      _lib.fptr(boxes), qlp, rlp, _lib.iptr(idx), _lib.fptr(dist) if return_dist else None)
            else:
                _call("mcp_knn_lengths", query, B, Q, N, k, mode, _lib.fptr(query), _lib.fptr(ref), qlp, rlp, _lib.iptr(idx),
                      _lib.fptr(dist) if return_dist else None)
        elif N >= self.PRUNE_MIN_REFS and Q >= self.PRUNE_MIN_QUERIES and k <= 32 and N <= 65536:
            _lib.fptr(query), _lib.fptr(ref)  # validate before building the sorted clouds
            rs, rperm, boxes = self._sorted_cloud(ref)
            same = query.data_ptr() == ref.data_ptr() and query.shape == ref.shape
            qs, qperm, _ = (rs, rperm, boxes) if same else self._sorted_cloud(query)
            _call("mcp_knn_pruned", query, B, Q, N, k, mode, _lib.fptr(qs), _lib.iptr(qperm), _lib.fptr(rs), _lib.iptr(rperm),
                  _lib.fptr(boxes), _lib.iptr(idx), _lib.fptr(dist) if return_dist else None)
        else:
            _call("mcp_knn", query, B, Q, N, k, mode, _lib.fptr(query), _lib.fptr(ref), _lib.iptr(idx),
                  _lib.fptr(dist) if return_dist else None)
        return (idx, dist) if return_dist else idx

    # ball query: when the box-pruned search (csrc/ball_query_pruned.hip) replaces the exhaustive scan.  The search alone is 4-11 x
    # faster than the scan at the small radii (8 x 2048 centres in 8 x 16384 points, r = 0.5 / nsample 16: 0.019 ms against 0.134;
    # profiles/ball_query_lengths_times.json) and level with it at r = 4 / nsample 8, where the scan stops early -- but a cloud build
    # costs 0.09 ms at N = 16384 and 0.46 ms beyond it, so build + search beats the scan only at two of that shape's four radii (0.111
    # against 0.134 ms), ties one, loses the fourth (0.127 against 0.034) and loses everywhere at 8 x 40960.  The radius is no shape:
    # no class of padded shapes wins with the build included, so the shape rule is off (a bound no supported cloud reaches) and the
    # pruned route is taken where the build is already paid -- the open cloud_scope holds the cloud sorted under these lengths
    # (prebuild_cloud, an earlier ball query that pruned, or a pruned KNN search): four radii on one prebuilt cloud take 0.177 ms
    # against 0.418 for four scans.
    BALL_PRUNE_MIN_REFS = 1 << 30
    BALL_PRUNE_MIN_CENTRES = 1024

    @classmethod
    def ball_prunable(cls, N, nsample):
        """What the pruned ball query supports: one list entry per lane (nsample <= 64), 16 tile bounds per lane (N <= 65536)."""
        return N <= 65536 and nsample <= 64

    @classmethod
    def prunes_ball(cls, M, N, nsample):
        """Whether a ball query of (B,M,3) centres in a (B,N,3) cloud builds the sorted cloud and takes the pruned route: a pure
        function of the padded shapes and nsample, with the two class attributes above as its thresholds."""
        return cls.ball_prunable(N, nsample) and N >= cls.BALL_PRUNE_MIN_REFS and M >= cls.BALL_PRUNE_MIN_CENTRES

    def ball_query(self, xyz, new_xyz, radius, nsample, xyz_lengths=None, new_xyz_lengths=None, return_count=False):
        """ball_query(radius, nsample, xyz, new_xyz) (pointnet2_utils.py:200-225) on a padded batch: xyz (B,N,3), centres new_xyz
        (B,M,3) -> idx (B,M,nsample) int32, with return_count also cnt (B,M) int32.
        xyz_lengths / new_xyz_lengths (forms: lengths_tensor): element b is xyz[b, :xyz_lengths[b]] with the centres
        new_xyz[b, :new_xyz_lengths[b]].  A live centre gets the first nsample indices inside the ball in ascending order, padded with
        the first hit, zeros without a hit -- the reference's row for the two prefixes; a padded centre gets zeros.  cnt = min(hits,
        nsample), 0 for padded centres: it tells "no hit" from "only point 0 hit".  Rows at or beyond a length are never read.
        Route: the box-pruned search when the padded shapes say so (prunes_ball) or when the open cloud_scope already holds this
        cloud sorted under these lengths (inside a scope several radii on one cloud share one build); the exhaustive scan
        otherwise -- the same bits either way.  As everywhere, lengths share a sorted cloud only as one int32 device tensor."""
        xyz, new_xyz = xyz.detach(), new_xyz.detach()  # an index-producing search: no gradient
        B, N, _ = xyz.shape
        M = new_xyz.shape[1]
        rl, ql = lengths_tensor(xyz_lengths, B, N, xyz.device), lengths_tensor(new_xyz_lengths, B, M, xyz.device)
        rlp, qlp = None if rl is None else _lib.iptr(rl), None if ql is None else _lib.iptr(ql)
        idx = torch.empty((B, M, nsample), dtype=torch.int32, device=xyz.device)
        cnt = torch.empty((B, M), dtype=torch.int32, device=xyz.device) if return_count else None
        cntp = _lib.iptr(cnt) if return_count else None
        if self.prunes_ball(M, N, nsample) or (self.ball_prunable(N, nsample) and self._holds_cloud(xyz, rl)):
            _lib.fptr(xyz), _lib.fptr(new_xyz)  # validate before building the sorted cloud
            rs, rperm, boxes = self._sorted_cloud(xyz, rl)
            _call("mcp_ball_query_pruned", xyz, B, N, M, float(radius), int(nsample), _lib.fptr(new_xyz), _lib.fptr(rs), _lib.iptr(rperm),
                  _lib.fptr(boxes), qlp, rlp, _lib.iptr(idx), cntp)
        else:
            _call("mcp_ball_query_lengths", xyz, B, N, M, float(radius), int(nsample), _lib.fptr(new_xyz), _lib.fptr(xyz), qlp, rlp,
                  _lib.iptr(idx), cntp)
        return (idx, cnt) if return_count else idx

    def knn_bruteforce(self, query, ref, k, mode=MCP_DIST_EXPANSION, return_dist=False, query_lengths=None, ref_lengths=None):
        """The exhaustive kernel regardless of size (tests compare both paths), with or without per-cloud lengths."""
        B, Q, _ = query.shape
        N = ref.shape[1]
        idx = torch.empty((B, Q, k), dtype=torch.int32, device=query.device)
        dist = torch.empty((B, Q, k), dtype=torch.float32, device=query.device) if return_dist else None
        if query_lengths is not None or ref_lengths is not None:
            ql, rl = lengths_tensor(query_lengths, B, Q, query.device), lengths_tensor(ref_lengths, B, N, query.device)
            _call("mcp_knn_lengths", query, B, Q, N, k, mode, _lib.fptr(query), _lib.fptr(ref), None if ql is None else _lib.iptr(ql),
                  None if rl is None else _lib.iptr(rl), _lib.iptr(idx), _lib.fptr(dist) if return_dist else None)
            return (idx, dist) if return_dist else idx
        _call("mcp_knn", query, B, Q, N, k, mode, _lib.fptr(query), _lib.fptr(ref), _lib.iptr(idx),
              _lib.fptr(dist) if return_dist else None)
        return (idx, dist) if return_dist else idx

    def knn_cosine(self, qfeat, rfeat, k, return_dist=False, query_lengths=None, ref_lengths=None):
        """knn_point_cosine(k, rfeat, qfeat) (pointconv_util.py:111-153) on channel-last features:
        (B,Q,C),(B,N,C) -> (B,Q,k) int32, ascending by (1 - cosine, index).  MFMA kernel, C in {64,128,256}.
        query_lengths / ref_lengths (forms: lengths_tensor): element b searches only rfeat[b, :ref_lengths[b]] and only
        qfeat[b, :query_lengths[b]] is live.  Live rows get what the search of the two prefixes on their own returns (fewer than k
        references: the tail repeats the last valid entry; none: index 0, distance 0); padded query rows get index 0 and distance 0;
        padded rows of either set are never read.  Without lengths nothing changes."""
        qfeat, rfeat = qfeat.detach().contiguous(), rfeat.detach().contiguous()
        B, Q, C = qfeat.shape
        N = rfeat.shape[1]
        idx = torch.empty((B, Q, k), dtype=torch.int32, device=qfeat.device)
        dist = torch.empty((B, Q, k), dtype=torch.float32, device=qfeat.device) if return_dist else None
        ws = torch.empty((B * (Q + N) * C,), dtype=torch.float32, device=qfeat.device)
        if query_lengths is not None or ref_lengths is not None:
            ql, rl = lengths_tensor(query_lengths, B, Q, qfeat.device), lengths_tensor(ref_lengths, B, N, qfeat.device)
            _call("mcp_knn_cosine_lengths", qfeat, B, Q, N, C, k, _lib.fptr(qfeat), _lib.fptr(rfeat), None if ql is None else _lib.iptr(ql),
                  None if rl is None else _lib.iptr(rl), _lib.iptr(idx), _lib.fptr(dist) if return_dist else None, _lib.fptr(ws))
            return (idx, dist) if return_dist else idx
        _call("mcp_knn_cosine", qfeat, B, Q, N, C, k, _lib.fptr(qfeat), _lib.fptr(rfeat), _lib.iptr(idx),
              _lib.fptr(dist) if return_dist else None, _lib.fptr(ws))
        return (idx, dist) if return_dist else idx

    def group_rows(self, points, idx):
        """index_points_group / index_points_gather (mocopci.py:1190-1215): points (B,N,C),
        idx (B,...) int32 -> (B,...,C).  Differentiable w.r.t. points (deterministic segmented-reduction backward)."""
        if points.requires_grad and torch.is_grad_enabled():
            return _GroupRowsFn.apply(points, idx)
        return _group_rows_fwd(points.contiguous(), idx)

    def group_rows_add_leaky(self, points, idx, centre, slope=0.1):
        """leaky(points[idx] + centre[:, :, None, :]): points (B,N,C), idx (B,S,K), centre (B,S,C) -> (B,S,K,C)
        (first layer of the unfused cross(), pointconv_util.py:762-770)."""
        B, N, C = points.shape
        _, S, K = idx.shape
        out = torch.empty((B, S, K, C), dtype=torch.float32, device=points.device)
        _call("mcp_group_rows_add_leaky", points, B, N, C, S, K, ctypes.c_float(slope), _lib.fptr(points), _lib.iptr(idx.contiguous()),
              _lib.fptr(centre), _lib.fptr(out))
        return out

    def _interp3_weights(self, dense, sparse, idx3):
        B, N, _ = dense.shape
        w3 = torch.empty((B, N, 3), dtype=torch.float32, device=dense.device)
        _call("mcp_interp3_weights", dense, B, N, sparse.shape[1], _lib.fptr(dense), _lib.fptr(sparse), _lib.iptr(idx3), _lib.fptr(w3))
        return w3

    def interp3_search(self, dense, sparse):
        """3-NN search + inverse-distance weights of UpsampleFlow (mocopci.py:1494-1498).  The weights are differentiable
        w.r.t. both coordinate sets (the reference's are: warped coordinates depend on predicted flows)."""
        dense, sparse = dense.contiguous(), sparse.contiguous()
        idx3 = self.knn(dense.detach(), sparse.detach(), 3)  # spatially pruned for the large levels, exhaustive below
        w3 = _Interp3WeightsFn.apply(self, dense, sparse, idx3) if grad.wants_grad(dense, sparse) else self._interp3_weights(dense, sparse, idx3)
        return idx3, w3

    def interp3_apply(self, feat, idx3, w3):
        """Blend of the three neighbours' rows; differentiable w.r.t. feat and the weights."""
        if grad.wants_grad(feat, w3):
            if not self.EXPLICIT_INTERP3_GRAD:   # A/B switch: autograd over the unfused blend
                return grad.run(lambda f, i, w: _interp3_apply_fwd(f.contiguous(), i.contiguous(), w.contiguous()),
                                lambda f, i, w: grad.interp3_apply_twin(self.group_rows, f, i, w), feat, idx3, w3)
            return _Interp3ApplyFn.apply(feat, idx3, w3)
        return _interp3_apply_fwd(feat.contiguous(), idx3.contiguous(), w3.contiguous())

    EXPLICIT_INTERP3_GRAD = True

    def interp3(self, dense, sparse, feat):
        """UpsampleFlow.forward (mocopci.py:1485-1502): dense (B,N,3), sparse (B,S,3), feat (B,S,C) -> (B,N,C)."""
        B, N, _ = dense.shape
        S, C = feat.shape[1], feat.shape[2]
        # large levels: spatially pruned 3-NN search.  The same two-step route carries the gradients (the fused small-level
        # kernel below has no autograd node), so it is also taken whenever one is wanted.
        if (S >= self.PRUNE_MIN_REFS and N >= self.PRUNE_MIN_QUERIES) or grad.wants_grad(dense, sparse, feat):
            idx3, w3 = self.interp3_search(dense, sparse)
            return self.interp3_apply(feat, idx3, w3)
        idx3 = torch.empty((B, N, 3), dtype=torch.int32, device=dense.device)
        w3 = torch.empty((B, N, 3), dtype=torch.float32, device=dense.device)
        out = torch.empty((B, N, C), dtype=torch.float32, device=dense.device)
        _call("mcp_interp3", dense, B, N, S, C, _lib.fptr(dense), _lib.fptr(sparse), _lib.fptr(feat), _lib.fptr(out),
              _lib.iptr(idx3), _lib.fptr(w3))
        return out

    def fusion_mlp(self, p1, p2, idx, w1, b1, w2, b2, w3, b3, lengths=None):
        """fusion after the neighbour searches (mocopci.py:803-819), BN folded into (w,b): -> (B,N,3).  Differentiable.
        lengths (forms: lengths_tensor): rows of p1 / p2 at or beyond lengths[b] are padding.  With 64 neighbours per point (2 x 32
        or one list of 64) the kernels take the lengths themselves (mcp_fusion_lengths / mcp_fusion_grad_lengths,
        csrc/fusion_lengths.hip): a padded point costs one branch, nothing of its rows of p1 and idx is read -- they may hold
        anything -- and nothing is masked around the call.  Every sum of this layer is per point, so lengths only save work: out is
        zero on padded rows, live rows have the bits of the dense call on the cloud alone, and gradients reach live rows only (the
        weight gradients are the dense sums with the padded points' terms left out).  The indices of live points must point at
        live rows of p2.  Other list widths: the dense kernel plus masking (padded rows of p1 and p2 replaced by zeros and padded
        rows of idx by 0 before the call, out masked after it), same results."""
        ia, ib, nb = _two_lists(idx)
        kernel_lists = nb == 64
        if lengths is not None and kernel_lists:
            lens = lengths_tensor(lengths, p1.shape[0], p1.shape[1], p1.device)
            if not grad.wants_grad(p1, p2, w1, b1, w2, b2, w3, b3):
                return self._fusion_mlp(p1, p2, idx, w1, b1, w2, b2, w3, b3, lens=lens)
            return _FusionFn.apply(self, ia.contiguous(), None if ib is None else ib.contiguous(), lens, p1, p2, w1, b1, w2, b2, w3, b3)
        if lengths is not None:
            B, N, _ = p1.shape
            live = grad.live_points(lengths_tensor(lengths, B, N, p1.device), B, N, p1.device).unsqueeze(-1)
            zero = p1.new_zeros(())
            halves = idx if isinstance(idx, (tuple, list)) else (idx,)
            halves = tuple(torch.where(live, h, torch.zeros((), dtype=h.dtype, device=h.device)) for h in halves)
            out = self.fusion_mlp(torch.where(live, p1, zero), torch.where(live, p2, zero), halves if len(halves) > 1 else halves[0], w1, b1, w2, b2, w3, b3)
            return torch.where(live, out, zero)
        if not grad.wants_grad(p1, p2, w1, b1, w2, b2, w3, b3):
            return self._fusion_mlp(p1, p2, idx, w1, b1, w2, b2, w3, b3)
        if not kernel_lists:   # the kernels take the 2 x 32 lists only: autograd over the unfused twin
            return grad.fusion_twin(self.group_rows, p1, p2, idx, w1, b1, w2, b2, w3, b3)
        return _FusionFn.apply(self, ia.contiguous(), None if ib is None else ib.contiguous(), None, p1, p2, w1, b1, w2, b2, w3, b3)

    # Under lengths, True: the forward keeps every live neighbour's score (mcp_fusion_bn_forward_save_lengths) and the backward's first
    # pass reads them (mcp_fusion_bn_backward_saved_lengths), as the dense route does.  False (the A/B): the forward keeps nothing and
    # the backward's first pass re-evaluates the layer (mcp_fusion_bn_forward_lengths / mcp_fusion_bn_backward_lengths).  Same bits.
    FUSION_BN_KEEP_SCORES_WITH_LENGTHS = True

    def fusion_bn(self, p1, p2, idx, conv, affine, eps, lengths=None):
        """The fusion layer of ONE reference call on batch statistics, differentiable w.r.t. p1, p2, the conv weights and the
        BatchNorm weight / bias: -> (out (B,N,3), bn, var) -- see _FusionBNFn.
        lengths (forms: lengths_tensor): the rows of p1 and p2 at or beyond lengths[b] are padding (mcp_fusion_bn_forward_save_lengths /
        mcp_fusion_bn_backward_saved_lengths; FUSION_BN_KEEP_SCORES_WITH_LENGTHS = False: mcp_fusion_bn_forward_lengths /
        mcp_fusion_bn_backward_lengths): every statistic and every gradient runs over the live points' rows only, out and the
        gradients of p1 are zero on padded rows, whose values and index rows are never read.  -> (out, bn, var, count) with count the
        live points (one int32 on the device; the statistics' rows are 64 * count).  The indices of live points must point at live
        rows of p2."""
        ia, ib, nb = _two_lists(idx)
        if nb != 64:
            raise ValueError("fusion_bn: the batch-statistics kernels take 64 neighbours per point (2 x 32 or one list of 64)")
        lens = lengths_tensor(lengths, p1.shape[0], p1.shape[1], p1.device)
        return _FusionBNFn.apply(self, float(eps), ia.contiguous(), None if ib is None else ib.contiguous(), lens, p1, p2, *conv, *affine)

    def fusion_bn_forward(self, p1, p2, idx, conv, affine, eps, saved=None, lengths=None):
        """The fusion layer of ONE reference call on batch statistics (net.train(); mocopci.py:810-819 with nn.BatchNorm2d in training
        mode): conv = (w1, b1, w2, b2, w3, b3) raw conv weights, affine = (gamma1, beta1, gamma2, beta2, gamma3, beta3).
        -> out (B,N,3), bn (1024: per layer mean | rstd | gamma | beta), var (256: biased batch variances 64 | 64 | 128).  No autograd.
        saved: (int32, float32, float32) tensors of B*N*64 elements that receive every neighbour's arg-max channel, zhat3 there and score
        (mcp_fusion_bn_forward_save; what mcp_fusion_bn_backward_saved reads).
        lengths: per-cloud lengths (see fusion_bn) -> (out, bn, var, count); together with saved the rows of live points are kept
        (mcp_fusion_bn_forward_save_lengths), a padded point's rows of the three tensors stay as they were."""
        lib = _lib.load()
        p1, p2 = p1.contiguous(), p2.contiguous()
        conv = [t.detach().contiguous() for t in conv]
        B, N, _ = p1.shape
        bn = torch.empty((lib.mcp_fusion_bn_floats(),), dtype=torch.float32, device=p1.device)
        at = 0
        for c, (g, b) in zip((64, 64, 128), zip(affine[0::2], affine[1::2])):
            bn[at + 2 * c:at + 3 * c] = g.detach()
            bn[at + 3 * c:at + 4 * c] = b.detach()
            at += 4 * c
        var = torch.empty((256,), dtype=torch.float32, device=p1.device)
        out = torch.empty((B, N, 3), dtype=torch.float32, device=p1.device)
        need = lib.mcp_fusion_bn_workspace_bytes(B, N)
        ws = torch.empty((need,), dtype=torch.uint8, device=p1.device)
        keep = () if saved is None else (_lib.iptr(saved[0]), _lib.fptr(saved[1]), _lib.fptr(saved[2]))
        if lengths is not None:
            lens = lengths_tensor(lengths, B, N, p1.device)
            count = torch.empty((1,), dtype=torch.int32, device=p1.device)
            _call("mcp_fusion_bn_forward_lengths" if saved is None else "mcp_fusion_bn_forward_save_lengths", p1, *_fusion_lead(p1, p2, idx, lens, conv),
                  float(eps), _lib.fptr(bn), _lib.fptr(var), _lib.fptr(out), _lib.iptr(count), *keep, ws.data_ptr(), need)
            return out, bn, var, count.view(())
        _call("mcp_fusion_bn_forward" if saved is None else "mcp_fusion_bn_forward_save", p1, *_fusion_lead(p1, p2, idx, None, conv),
              float(eps), _lib.fptr(bn), _lib.fptr(var), _lib.fptr(out), *keep, ws.data_ptr(), need)
        return out, bn, var

    BN_BATCH_CHANNELS = (32, 64, 128, 256)

    def bn_batch(self, x, weight, bias, eps, lengths=None):
        """BatchNorm on BATCH statistics (net.train()) of x (G,F,N,C) or (G,N,C), channels last: each of the G groups is normalised
        with its own mean and biased variance (the reference's per-sample loops, mocopci.py:503-506, :554-561), differentiable
        w.r.t. x, weight and bias (mcp_bn_batch_forward / mcp_bn_batch_backward).  -> (y, mean (G,C), var (G,C), count (G) int32).
        lengths (forms: lengths_tensor; one entry per group, at most N): row (f, i) of group g is live iff i < lengths[g]; the
        statistics and the backward's mean terms run over the count[g] = F * lengths[g] live rows, y and the gradient of x are zero
        on padded rows, whose values are never read.  A group without a live row: mean 0, var 0.  No synchronisation.
        C outside 32 / 64 / 128 / 256: the masked torch formulation (grad.bn_batch_lengths_twin), same definition."""
        if x.dim() not in (3, 4):
            raise ValueError(f"bn_batch: x must be (G,F,N,C) or (G,N,C), got {tuple(x.shape)}")
        G, N, C = x.shape[0], x.shape[-2], x.shape[-1]
        lens = lengths_tensor(lengths, G, N, x.device)
        if C not in self.BN_BATCH_CHANNELS or x.dtype != torch.float32 or x.numel() == 0:
            return grad.bn_batch_lengths_twin(x, weight, bias, eps, lens)
        y, mean, var, count = _BNBatchFn.apply(float(eps), lens, x.reshape(G, -1, N, C), weight, bias)
        return y.reshape(x.shape), mean, var, count

    def _fusion_mlp(self, p1, p2, idx, w1, b1, w2, b2, w3, b3, lens=None):
        p1, p2, *conv = (t.contiguous() for t in (p1, p2, w1, b1, w2, b2, w3, b3))
        B, N, _ = p1.shape
        out = torch.empty((B, N, 3), dtype=torch.float32, device=p1.device)
        # idx: the two searches' lists as they are, or one (B,N,64) list; per-cloud lengths: the kernel of csrc/fusion_lengths.hip
        _call("mcp_fusion" if lens is None else "mcp_fusion_lengths", p1, *_fusion_lead(p1, p2, idx, lens, conv), _lib.fptr(out))
        return out

    def cross_pack(self, wpos, bpos, wmlp, bmlp):
        """Pack one cross layer's weights into the kernel's MFMA-operand image (do this once per layer)."""
        D = wmlp.shape[0]
        lib = _lib.load()
        n = lib.mcp_cross_packed_floats(D)
        if n == 0:
            raise RuntimeError(f"cross_volume supports D in (64, 128, 256), got {D}")
        packed = torch.empty((n,), dtype=torch.float32, device=wmlp.device)
        _call("mcp_cross_pack", wmlp, D, _lib.fptr(wpos.contiguous()), _lib.fptr(bpos.contiguous()), _lib.fptr(wmlp.contiguous()),
              _lib.fptr(bmlp.contiguous()), _lib.fptr(packed))
        return packed

    def cross_volume(self, xyz1, xyz2, points1, points2, idx, packed, bmap=None, shared=0):
        """cross() after its neighbour searches (pointconv_util.py:750-781): -> (B,N1,D); D in {64,128,256};
        packed = cross_pack(wpos, bpos, wmlp, bmlp).  bmap (B int32) + shared (1 points1, 2 points2, 4 first index list): those
        tensors hold a smaller batch and element b is read from their element bmap[b] (replicated inputs are not copied)."""
        B, N1 = xyz1.shape[0], xyz1.shape[1]
        D = points1.shape[2]
        N2 = xyz2.shape[1]
        out = torch.empty((B, N1, D), dtype=torch.float32, device=points1.device)
        ia, ib, k = _two_lists(idx)   # the 16 + 16 halves as the searches produce them, or one list
        if bmap is not None and (shared & 4) and ib is None:
            raise RuntimeError("a shared index list needs the two-list form")
        _call("mcp_cross_volume", points1, B, N1, N2, D, k, _lib.fptr(xyz1), _lib.fptr(xyz2), _lib.fptr(points1),
              _lib.fptr(points2), _lib.iptr(ia), None if ib is None else _lib.iptr(ib), None if bmap is None else _lib.iptr(bmap), int(shared),
              _lib.fptr(packed), _lib.fptr(out))
        return out

    def cross_layer(self, xyz1, xyz2, points1, points2, idx, wpos, bpos, wmlp, bmlp, packed=None, bmap=None, shared=0):
        """cross() from the layer's own weights; differentiable w.r.t. coordinates, features and weights.  packed: the
        cross_pack image of these weights when the caller keeps one (inference); built on the fly otherwise.  bmap / shared:
        see cross_volume (inference only: a training forward passes the replicated tensors)."""
        def fused(x1, x2, f1, f2, i, wp, bp, wm, bm):
            pk = packed if packed is not None else self.cross_pack(wp, bp, wm, bm)
            return self.cross_volume(x1.contiguous(), x2.contiguous(), f1.contiguous(), f2.contiguous(), i, pk, bmap=bmap, shared=shared)
        if bmap is not None:
            return fused(xyz1, xyz2, points1, points2, idx, wpos, bpos, wmlp, bmlp)
        ia, ib, k_total = _two_lists(idx)   # the backward kernel is built for the 32-neighbour lists
        if grad.wants_grad(xyz1, xyz2, points1, points2, wpos, bpos, wmlp, bmlp) and k_total == 32 and wmlp.shape[0] in (64, 128, 256):
            return _CrossFn.apply(self, ia.contiguous(), None if ib is None else ib.contiguous(), xyz1, xyz2, points1, points2, wpos, bpos, wmlp, bmlp)
        return grad.run(fused, lambda *a: grad.cross_twin(self.group_rows, *a), xyz1, xyz2, points1, points2, idx, wpos, bpos, wmlp, bmlp)

    def group_mlp(self, xyz, new_xyz, features, idx, packed, widths, pool="max", use_xyz=True, new_xyz_lengths=None, row_bias=None):
        """Set-abstraction layer after its neighbour search (PointnetSAModule[MSG]; SetConv / FlowEmbedding, models/layers.py:76-117)
        in one launch: xyz (B,N,3), centres new_xyz (B,M,3), features (B,N,C) channel-last or None, idx (B,M,nsample) int32,
        (packed, widths) = group_mlp_pack(...) -> (B,M,widths[-1]): the pool ("max" | "mean") over the nsample slots of the shared
        MLP of [xyz[idx] - new_xyz (use_xyz) | features[idx]], every layer followed by ReLU.  row_bias (B,M,widths[0]) is added
        before the first ReLU (the centre's own features through the first layer's columns for them: FlowEmbedding's concatenation).
        new_xyz_lengths (forms: lengths_tensor): centres at or beyond the length give zeros and their rows are never read.
        No gradient here: group_mlp_layer is the differentiable form.  Unsupported shapes raise _lib.Unsupported."""
        return self._group_mlp(xyz, new_xyz, features, idx, packed, widths, pool, use_xyz, new_xyz_lengths, row_bias)

    def _group_mlp(self, xyz, new_xyz, features, idx, packed, widths, pool, use_xyz, new_xyz_lengths, row_bias):
        """The launch of group_mlp, shared with the differentiable layer's forward."""
        B, N, _ = xyz.shape
        M, nsample = new_xyz.shape[1], idx.shape[2]
        C = 0 if features is None else features.shape[2]
        widths = [int(w) for w in widths]
        ql = lengths_tensor(new_xyz_lengths, B, M, xyz.device)
        out = torch.empty((B, M, widths[-1]), dtype=torch.float32, device=xyz.device)
        if B == 0 or M == 0:
            return out
        if row_bias is not None and tuple(row_bias.shape) != (B, M, widths[0]):
            raise RuntimeError(f"row_bias: expected {(B, M, widths[0])}, got {tuple(row_bias.shape)}")
        _call("mcp_group_mlp", xyz, *_group_lead((B, N, M, C, nsample), pool, use_xyz, _int_array(widths), xyz, new_xyz, features, idx, ql),
              _opt(row_bias), _lib.fptr(packed), _lib.fptr(out))
        return out

    def group_mlp_grad(self, xyz, new_xyz, features, idx, weights, grad_out, pool="max", use_xyz=True, new_xyz_lengths=None, row_bias=None,
                       want_features=True, want_xyz=True, want_new_xyz=True, want_row_bias=True, recompute_out=False):
        """Backward of group_mlp for weights = [(W, b), ...] (folded, fp32) and grad_out (B,M,widths[-1]): one per-pair kernel, the
        deterministic scatters and one weight-gradient product per layer (mcp_group_mlp_grad) -> (grad_features (B,N,C), grad_xyz
        (B,N,3), grad_new_xyz (B,M,3), grad_row_bias (B,M,widths[0]) -- each None when not wanted or not part of the layer --, [dW_l],
        [db_l], the recomputed out or None).  Bit-reproducible; unsupported shapes raise _lib.Unsupported."""
        dims, widths = _group_check("group_mlp_grad", xyz, new_xyz, features, idx, weights, use_xyz, grad_out=grad_out)
        B, N, M, C, nsample = dims
        dev = xyz.device
        if row_bias is not None and tuple(row_bias.shape) != (B, M, widths[0]):
            raise RuntimeError(f"row_bias: expected {(B, M, widths[0])}, got {tuple(row_bias.shape)}")
        ql = lengths_tensor(new_xyz_lengths, B, M, dev)
        grad_out = grad_out.contiguous()
        packed, _ = group_mlp_grad_pack_weights(weights, use_xyz)
        wid = _int_array(widths)
        need = _lib.load().mcp_group_mlp_grad_workspace_bytes(B, M, C, nsample, int(bool(use_xyz)), len(widths), wid)
        if need == 0:
            raise _lib.Unsupported(f"group_mlp_grad: unsupported shape c={C} widths={widths} pairs={B * M * nsample}")
        want_features, want_xyz, want_new_xyz = bool(want_features) and C > 0, bool(want_xyz) and use_xyz, bool(want_new_xyz) and use_xyz
        want_row_bias = bool(want_row_bias) and row_bias is not None
        ws = _grad_empty((need,), torch.uint8, dev)
        d_feat = _grad_empty((B, N, C), torch.float32, dev) if want_features else None
        d_xyz = _grad_empty((B, N, 3), torch.float32, dev) if want_xyz else None
        d_new = _grad_empty((B, M, 3), torch.float32, dev) if want_new_xyz else None
        d_rb = _grad_empty((B, M, widths[0]), torch.float32, dev) if want_row_bias else None
        d_w = [_grad_empty(tuple(w.shape), torch.float32, dev) for w, _ in weights]
        d_b = [_grad_empty(tuple(b.shape), torch.float32, dev) for _, b in weights]
        out = _grad_empty((B, M, widths[-1]), torch.float32, dev) if recompute_out else None
        order, seg = _scatter_segments(idx.reshape(B, M * nsample), N) if (want_features or want_xyz) else (None, None)
        _call("mcp_group_mlp_grad", xyz, *_group_lead(dims, pool, use_xyz, wid, xyz, new_xyz, features, idx, ql), _opt(row_bias), _lib.fptr(packed),
              _lib.fptr(grad_out), _opt(order, _lib.iptr), _opt(seg, _lib.iptr), _opt(d_feat), _opt(d_xyz), _opt(d_new), _opt(d_rb), _ptr_array(d_w),
              _ptr_array(d_b), _opt(out), ws.data_ptr(), need)
        return d_feat, d_xyz, d_new, d_rb, d_w, d_b, out

    def group_mlp_layer(self, xyz, new_xyz, features, idx, weights, pool="max", use_xyz=True, new_xyz_lengths=None, row_bias=None):
        """The set-abstraction layer from its own weights [(W (out, in), b (out,)), ...] (BatchNorm folded in: fold_conv_bn_grad keeps
        the parameters in the graph); arguments as group_mlp.  Without a wanted gradient it is group_mlp on a pack of `weights`; with
        one it is an autograd function -- mcp_group_mlp forward, mcp_group_mlp_grad backward -- that returns gradients for xyz,
        new_xyz, features, row_bias and every W and b, each only when needed, and keeps only its inputs."""
        flat = _flat(weights)
        if not grad.wants_grad(xyz, new_xyz, features, row_bias, *flat):
            packed, widths = group_mlp_pack_weights([(w.detach(), b.detach()) for w, b in weights], use_xyz)
            xyz, new_xyz, features, row_bias = [_det(t, False) for t in (xyz, new_xyz, features, row_bias)]
            return self._group_mlp(xyz, new_xyz, features, idx, packed, widths, pool, use_xyz, new_xyz_lengths, row_bias)
        B, M = new_xyz.shape[0], new_xyz.shape[1]
        C = 0 if features is None else features.shape[2]
        if not group_mlp_grad_supported(C, [int(w.shape[0]) for w, _ in weights], idx.shape[2], use_xyz):
            raise _lib.Unsupported(f"group_mlp_layer: unsupported shape c={C} widths={[int(w.shape[0]) for w, _ in weights]} nsample={idx.shape[2]}")
        ql = lengths_tensor(new_xyz_lengths, B, M, xyz.device)
        return _GroupMlpLayerFn.apply(self, pool, bool(use_xyz), idx.contiguous(), ql, xyz, new_xyz, features, row_bias, *flat)

    def fp_mlp(self, known_feats, skip, idx, dist, packed, widths, rule="pointnet2", w3=None, unknown_lengths=None):
        """Feature-propagation layer after its three-neighbour search (PointnetFPModule; FeaturePropagation, models/layers.py:150-178)
        in one launch: known_feats (B,m,C2) and skip (B,n,C1) or None channel-last, idx / dist (B,n,3) as three_nn returns them,
        (packed, widths) = fp_mlp_pack(...) -> (B,n,widths[-1]): the shared MLP, every layer followed by ReLU, of
        [w0 f[i0] + w1 f[i1] + w2 f[i2] | skip].  rule: "pointnet2" (1 / (dist + 1e-8), normalised), "flownet3d" (1 / max(dist^2,
        1e-10), normalised) or "given" (w3 (B,n,3) as it is; dist may be None).  A slot with dist = +inf weighs exactly 0 under the
        two computed rules.  unknown_lengths (forms: lengths_tensor): rows at or beyond the length give zeros and are never read.
        Inference only (no gradient); unsupported shapes raise _lib.Unsupported."""
        dims, widths = _fp_check("fp_mlp", known_feats, skip, idx, dist, rule, w3, None, widths=[int(w) for w in widths])
        B, n, m, C2, C1, _ = dims
        wid = _int_array(widths)
        if packed.numel() != _lib.load().mcp_fp_mlp_packed_floats(C2, C1, len(widths), wid):
            raise RuntimeError("fp_mlp: the packed image was built for another shape")
        ul = lengths_tensor(unknown_lengths, B, n, known_feats.device)
        out = torch.empty((B, n, widths[-1]), dtype=torch.float32, device=known_feats.device)
        if B == 0 or n == 0:
            return out
        if m == 0:
            raise RuntimeError("fp_mlp: the known cloud is empty")
        _call("mcp_fp_mlp", known_feats, *_fp_lead(dims, wid, known_feats, skip, idx, dist, w3, ul, packed), _lib.fptr(out))
        return out

    def fp_mlp_grad(self, known_feats, skip, idx, dist, weights, grad_out, rule="pointnet2", w3=None, unknown_lengths=None, want_known=True,
                    recompute_out=False):
        """Backward of fp_mlp for weights = [(W, b), ...] (folded, fp32) and grad_out (B,n,widths[-1]) in one kernel launch plus the
        deterministic scatter and one weight-gradient product per layer (mcp_fp_mlp_grad) -> (grad_known_feats (B,m,C2) or None,
        grad_skip (B,n,C1) or None, [dW_l], [db_l], the recomputed out or None).  Bit-reproducible; unsupported shapes raise."""
        dims, widths = _fp_check("fp_mlp_grad", known_feats, skip, idx, dist, rule, w3, weights, grad_out=grad_out)
        B, n, m, C2, C1, _ = dims
        dev = known_feats.device
        ul = lengths_tensor(unknown_lengths, B, n, dev)
        grad_out = grad_out.contiguous()
        packed, _ = fp_mlp_grad_pack_weights(weights, C2)
        wid = _int_array(widths)
        need = _lib.load().mcp_fp_mlp_grad_workspace_bytes(B, n, C2, C1, len(widths), wid)
        if need == 0:
            raise _lib.Unsupported(f"fp_mlp_grad: unsupported shape c2={C2} c1={C1} widths={widths} rows={B * n}")
        ws = _grad_empty((need,), torch.uint8, dev)
        d_known = _grad_empty((B, m, C2), torch.float32, dev) if want_known else None
        d_skip = _grad_empty((B, n, C1), torch.float32, dev) if C1 else None
        d_w = [_grad_empty(tuple(w.shape), torch.float32, dev) for w, _ in weights]
        d_b = [_grad_empty(tuple(b.shape), torch.float32, dev) for _, b in weights]
        out = _grad_empty((B, n, widths[-1]), torch.float32, dev) if recompute_out else None
        order, seg = _scatter_segments(idx, m) if want_known else (None, None)
        _call("mcp_fp_mlp_grad", known_feats, *_fp_lead(dims, wid, known_feats, skip, idx, dist, w3, ul, packed), _lib.fptr(grad_out),
              _opt(order, _lib.iptr), _opt(seg, _lib.iptr), _opt(d_known), _opt(d_skip), _ptr_array(d_w), _ptr_array(d_b), _opt(out), ws.data_ptr(), need)
        return d_known, d_skip, d_w, d_b, out

    def fp_mlp_layer(self, known_feats, skip, idx, dist, weights, rule="pointnet2", w3=None, unknown_lengths=None):
        """The feature-propagation layer from its own weights [(W (out, in), b (out,)), ...] (BatchNorm folded in: fold_conv_bn_grad
        keeps the parameters in the graph); arguments as fp_mlp.  Without a wanted gradient it is fp_mlp on a pack of `weights`;
        with one it is an autograd function -- mcp_fp_mlp forward, mcp_fp_mlp_grad backward -- that returns gradients for
        known_feats, skip and every W and b, and keeps only its inputs."""
        flat = _flat(weights)
        if not grad.wants_grad(known_feats, skip, *flat):
            packed, widths = fp_mlp_pack_weights([(w.detach(), b.detach()) for w, b in weights], known_feats.shape[-1])
            return self.fp_mlp(known_feats.detach(), None if skip is None else skip.detach(), idx, dist, packed, widths, rule=rule, w3=w3,
                               unknown_lengths=unknown_lengths)
        B, n = idx.shape[0], idx.shape[1]
        ul = lengths_tensor(unknown_lengths, B, n, known_feats.device)
        return _FpMlpLayerFn.apply(self, rule, idx.contiguous(), dist, w3, ul, known_feats, skip, *flat)

    def fp_mlp_bn_forward(self, known_feats, skip, idx, dist, layers, eps, rule="pointnet2", w3=None, unknown_lengths=None):
        """The feature-propagation layer with batch statistics (mcp_fp_mlp_bn_forward): arguments as fp_mlp, layers = [(W (out, in),
        b or None, gamma or None, beta or None), ...] fp32, eps one float per layer -> (out (B,n,widths[-1]), [mean_l], [biased
        var_l], [rstd_l], count (1,) int32: the live rows, on the device).  Padded rows give zeros and enter no statistic."""
        dims, widths = _fp_check("fp_mlp_bn_forward", known_feats, skip, idx, dist, rule, w3, layers)
        B, n, m, C2, C1, _ = dims
        eps = _bn_eps("fp_mlp_bn_forward", eps, layers)
        dev = known_feats.device
        ul = lengths_tensor(unknown_lengths, B, n, dev)
        packed, _ = fp_mlp_pack_weights(_bn_pairs(layers), C2)
        wid = _int_array(widths)
        need = _lib.load().mcp_fp_mlp_bn_workspace_bytes(B, n, C2, C1, len(widths), wid, 0)
        if need == 0:
            raise _lib.Unsupported(f"fp_mlp_bn_forward: unsupported shape c2={C2} c1={C1} widths={widths} rows={B * n}")
        ws = _grad_empty((need,), torch.uint8, dev)
        out = _grad_empty((B, n, widths[-1]), torch.float32, dev)
        mean, var, rstd = ([_grad_empty((o,), torch.float32, dev) for o in widths] for _ in range(3))
        count = _grad_empty((1,), torch.int32, dev)
        _call("mcp_fp_mlp_bn_forward", known_feats, *_fp_lead(dims, wid, known_feats, skip, idx, dist, w3, ul, packed), *_bn_affine(layers), eps,
              _lib.fptr(out), _ptr_array(mean), _ptr_array(var), _ptr_array(rstd), _lib.iptr(count), ws.data_ptr(), need)
        return out, mean, var, rstd, count

    def fp_mlp_bn_backward(self, known_feats, skip, idx, dist, layers, mean, rstd, grad_out, rule="pointnet2", w3=None, unknown_lengths=None,
                           want_known=True):
        """Backward of fp_mlp_bn_forward (mcp_fp_mlp_bn_backward) from the forward's inputs, its per-layer (mean, rstd) and grad_out
        (B,n,widths[-1]) -> (grad_known_feats (B,m,C2) or None, grad_skip (B,n,C1) or None, [(dW, db or None, dgamma or None, dbeta
        or None), ...]; a parameter that is None gets None).  Bit-reproducible; unsupported shapes raise."""
        dims, widths = _fp_check("fp_mlp_bn_backward", known_feats, skip, idx, dist, rule, w3, layers)
        B, n, m, C2, C1, _ = dims
        _check_grad_out("fp_mlp_bn_backward", grad_out, (B, n, widths[-1]))
        dev = known_feats.device
        ul = lengths_tensor(unknown_lengths, B, n, dev)
        grad_out = grad_out.contiguous()
        packed, _ = fp_mlp_grad_pack_weights(_bn_pairs(layers), C2)
        wid = _int_array(widths)
        need = _lib.load().mcp_fp_mlp_bn_workspace_bytes(B, n, C2, C1, len(widths), wid, 1)
        if need == 0:
            raise _lib.Unsupported(f"fp_mlp_bn_backward: unsupported shape c2={C2} c1={C1} widths={widths} rows={B * n}")
        ws = _grad_empty((need,), torch.uint8, dev)
        d_known = _grad_empty((B, m, C2), torch.float32, dev) if want_known else None
        d_skip = _grad_empty((B, n, C1), torch.float32, dev) if C1 else None
        d_layers, d_arrays = _bn_grads(layers, dev)
        order, seg = _scatter_segments(idx, m) if want_known else (None, None)
        _call("mcp_fp_mlp_bn_backward", known_feats, *_fp_lead(dims, wid, known_feats, skip, idx, dist, w3, ul, packed), *_bn_affine(layers),
              _ptr_array(mean), _ptr_array(rstd), _lib.fptr(grad_out), _opt(order, _lib.iptr), _opt(seg, _lib.iptr), _opt(d_known), _opt(d_skip),
              *d_arrays, ws.data_ptr(), need)
        return d_known, d_skip, d_layers

    def fp_mlp_bn_layer(self, known_feats, skip, idx, dist, layers, rule="pointnet2", w3=None, unknown_lengths=None):
        """The feature-propagation layer under a training-mode BatchNorm from its own parameters: layers = [(W (out, in), b or None,
        gamma or None, beta or None, eps), ...]; other arguments as fp_mlp -> (out (B,n,widths[-1]), [(mean_l, biased var_l), ...],
        count (1,) int32 on the device).  An autograd function -- mcp_fp_mlp_bn_forward, mcp_fp_mlp_bn_backward -- with gradients for
        known_feats, skip and every W, b, gamma, beta; the statistics and the count are not differentiable.  It runs with or without
        a wanted gradient (the caller's running statistics need the batch statistics either way)."""
        B, n = idx.shape[0], idx.shape[1]
        ul = lengths_tensor(unknown_lengths, B, n, known_feats.device)
        flat = _flat(layer[:4] for layer in layers)
        out, *rest = _FpMlpBnLayerFn.apply(self, rule, idx.contiguous(), dist, w3, ul, tuple(float(layer[4]) for layer in layers), known_feats, skip, *flat)
        return out, _pairs(rest[:-1]), rest[-1]

    def group_mlp_bn_forward(self, xyz, new_xyz, features, idx, layers, eps, pool="max", use_xyz=True, new_xyz_lengths=None):
        """The set-abstraction layer with batch statistics (mcp_group_mlp_bn_forward): arguments as group_mlp, layers = [(W (out, in),
        b or None, gamma or None, beta or None), ...] fp32 with W_1's position columns first, eps one float per layer -> (out
        (B,M,widths[-1]), [mean_l], [biased var_l], [rstd_l], count (1,) int32: the live (centre, slot) pairs, on the device).
        Padded centres give zeros and enter no statistic."""
        dims, widths = _group_check("group_mlp_bn_forward", xyz, new_xyz, features, idx, layers, use_xyz)
        B, N, M, C, nsample = dims
        eps = _bn_eps("group_mlp_bn_forward", eps, layers)
        dev = xyz.device
        ql = lengths_tensor(new_xyz_lengths, B, M, dev)
        packed, _ = group_mlp_bn_pack_weights(_bn_pairs(layers), use_xyz)
        wid = _int_array(widths)
        need = _lib.load().mcp_group_mlp_bn_workspace_bytes(B, M, C, nsample, int(bool(use_xyz)), len(widths), wid, 0)
        if need == 0:
            raise _lib.Unsupported(f"group_mlp_bn_forward: unsupported shape c={C} widths={widths} pairs={B * M * nsample}")
        ws = _grad_empty((need,), torch.uint8, dev)
        out = _grad_empty((B, M, widths[-1]), torch.float32, dev)
        mean, var, rstd = ([_grad_empty((o,), torch.float32, dev) for o in widths] for _ in range(3))
        count = _grad_empty((1,), torch.int32, dev)
        _call("mcp_group_mlp_bn_forward", xyz, *_group_lead(dims, pool, use_xyz, wid, xyz, new_xyz, features, idx, ql), _lib.fptr(packed),
              *_bn_affine(layers), eps, _lib.fptr(out), _ptr_array(mean), _ptr_array(var), _ptr_array(rstd), _lib.iptr(count), ws.data_ptr(), need)
        return out, mean, var, rstd, count

    def group_mlp_bn_backward(self, xyz, new_xyz, features, idx, layers, mean, rstd, grad_out, pool="max", use_xyz=True, new_xyz_lengths=None,
                              want_features=True, want_xyz=True, want_new_xyz=True):
        """Backward of group_mlp_bn_forward (mcp_group_mlp_bn_backward) from the forward's inputs, its per-layer (mean, rstd) and
        grad_out (B,M,widths[-1]) -> (grad_features (B,N,C), grad_xyz (B,N,3), grad_new_xyz (B,M,3) -- each None when not wanted or not
        part of the layer --, [(dW, db or None, dgamma or None, dbeta or None), ...]; a parameter that is None gets None).
        Bit-reproducible; unsupported shapes raise."""
        dims, widths = _group_check("group_mlp_bn_backward", xyz, new_xyz, features, idx, layers, use_xyz)
        B, N, M, C, nsample = dims
        _check_grad_out("group_mlp_bn_backward", grad_out, (B, M, widths[-1]))
        dev = xyz.device
        ql = lengths_tensor(new_xyz_lengths, B, M, dev)
        grad_out = grad_out.contiguous()
        packed, _ = group_mlp_bn_pack_weights(_bn_pairs(layers), use_xyz)
        wid = _int_array(widths)
        need = _lib.load().mcp_group_mlp_bn_workspace_bytes(B, M, C, nsample, int(bool(use_xyz)), len(widths), wid, 1)
        if need == 0:
            raise _lib.Unsupported(f"group_mlp_bn_backward: unsupported shape c={C} widths={widths} pairs={B * M * nsample}")
        want_features, want_xyz, want_new_xyz = bool(want_features) and C > 0, bool(want_xyz) and use_xyz, bool(want_new_xyz) and use_xyz
        ws = _grad_empty((need,), torch.uint8, dev)
        d_feat = _grad_empty((B, N, C), torch.float32, dev) if want_features else None
        d_xyz = _grad_empty((B, N, 3), torch.float32, dev) if want_xyz else None
        d_new = _grad_empty((B, M, 3), torch.float32, dev) if want_new_xyz else None
        d_layers, d_arrays = _bn_grads(layers, dev)
        order, seg = _scatter_segments(idx.reshape(B, M * nsample), N) if (want_features or want_xyz) else (None, None)
        _call("mcp_group_mlp_bn_backward", xyz, *_group_lead(dims, pool, use_xyz, wid, xyz, new_xyz, features, idx, ql), _lib.fptr(packed),
              *_bn_affine(layers), _ptr_array(mean), _ptr_array(rstd), _lib.fptr(grad_out), _opt(order, _lib.iptr), _opt(seg, _lib.iptr),
              _opt(d_feat), _opt(d_xyz), _opt(d_new), *d_arrays, ws.data_ptr(), need)
        return d_feat, d_xyz, d_new, d_layers

    def group_mlp_bn_layer(self, xyz, new_xyz, features, idx, layers, pool="max", use_xyz=True, new_xyz_lengths=None):
        """The set-abstraction layer under a training-mode BatchNorm from its own parameters: layers = [(W (out, in), b or None, gamma or
        None, beta or None, eps), ...]; other arguments as group_mlp -> (out (B,M,widths[-1]), [(mean_l, biased var_l), ...], count
        (1,) int32 on the device: the live (centre, slot) pairs).  An autograd function -- mcp_group_mlp_bn_forward,
        mcp_group_mlp_bn_backward -- with gradients for xyz, new_xyz, features and every W, b, gamma, beta; idx, the lengths, the
        statistics and the count get none.  It runs with or without a wanted gradient (the caller's running statistics need the batch
        statistics either way)."""
        B, M = new_xyz.shape[0], new_xyz.shape[1]
        ql = lengths_tensor(new_xyz_lengths, B, M, xyz.device)
        flat = _flat(layer[:4] for layer in layers)
        out, *rest = _GroupMlpBnLayerFn.apply(self, pool, bool(use_xyz), idx.contiguous(), ql, tuple(float(layer[4]) for layer in layers), xyz, new_xyz,
                                              features, *flat)
        return out, _pairs(rest[:-1]), rest[-1]

    def ptblock_layer(self, xyz, q, k, v, idx, weights, packed=None):
        """TransformerBlock vector attention from the block's own weights (wd1,bd1,wd2,bd2,wg1,bg1,wg2,bg2); differentiable."""
        def fused(x, q_, k_, v_, i, *w):
            pk = packed if packed is not None else self.ptblock_pack(*w)
            return self.ptblock_attention(x.contiguous(), q_, k_, v_, i, pk)
        if grad.wants_grad(xyz, q, k, v, *weights) and q.shape[-1] == 64 and idx.shape[-1] == 16:
            return _PtblockFn.apply(self, idx.contiguous(), xyz, q, k, v, *weights)
        return grad.run(fused, lambda *a: grad.ptblock_twin(self.group_rows, *a), xyz, q, k, v, idx, *weights)

    def ptblock_pack(self, wd1, bd1, wd2, bd2, wg1, bg1, wg2, bg2):
        """Pack fc_delta / fc_gamma of a TransformerBlock (pointT_layer2.py:42-51) into the kernel's operand image."""
        packed = torch.empty((_lib.load().mcp_ptblock_packed_floats(),), dtype=torch.float32, device=wd2.device)
        args = [t.contiguous() for t in (wd1, bd1, wd2, bd2, wg1, bg1, wg2, bg2)]
        _call("mcp_ptblock_pack", wd2, *[_lib.fptr(t) for t in args], _lib.fptr(packed))
        return packed

    def ptblock_attention(self, xyz, q, k, v, idx, packed):
        """Vector attention of TransformerBlock.forward (pointT_layer2.py:68-75) after knn + projections: -> (B,N,64).
        q, k, v: (B,N,64) tensors, or last-axis slices of one packed (B,N,192) projection (read in place through the row stride)."""
        B, N, C = q.shape
        rs = q.stride(1)
        for t in (q, k, v):
            if not (t.is_cuda and t.dtype == torch.float32 and t.shape == (B, N, C) and t.stride() == (N * rs, rs, 1)):
                raise RuntimeError("q, k, v must be float32 CUDA tensors of one shape with unit channel stride and a common row stride")
        out = torch.empty((B, N, C), dtype=torch.float32, device=q.device)
        _call("mcp_ptblock_attention", q, B, N, C, idx.shape[-1], rs, _lib.fptr(xyz), q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.iptr(idx),
              _lib.fptr(packed), _lib.fptr(out))
        return out

    def pointconv_agg(self, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, centre_lengths=None):
        """PointConv grouping + WeightNet + aggregation (mocopci.py:1330-1335): -> (B,S,(3+D)*8).  Differentiable.
        centre_lengths: per-element number of live centres of a padded batch (see lengths_tensor; None = all S): centre i of element
        b is live iff i < centre_lengths[b].  Live centres get the dense call's bits; a padded centre has none of its inputs read
        (its idx row, new_xyz, the gathered rows, the upstream gradient: they may hold NaN or out-of-range indices), its row is
        exact zeros, as are its gradient rows, and it adds nothing to the WeightNet's weight gradients.  No synchronisation."""
        D = s_points.shape[-1]
        qlen = lengths_tensor(centre_lengths, new_xyz.shape[0], new_xyz.shape[1], s_points.device)   # None stays None
        if not grad.wants_grad(s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2):
            return self._pointconv_agg(s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, qlen=qlen)
        if idx.shape[-1] != 32 or D % 4 or D > 256 or tuple(w2.shape) != (8, 8):   # no backward kernel: the (masked) torch formulation
            twin = ((lambda *a: grad.pointconv_agg_twin(self.group_rows, *a)) if qlen is None
                    else (lambda *a: grad.pointconv_agg_lengths_twin(self.group_rows, *a, qlen)))
            return grad.run(lambda *a: self._pointconv_agg(*a, qlen=qlen), twin, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2)
        return _PointConvAggFn.apply(self, idx.contiguous(), s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2, qlen)

    def _pointconv_agg(self, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, qlen=None):
        s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2 = (t.contiguous() for t in (s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2))
        B, N, D = s_points.shape
        S = new_xyz.shape[1]
        out = torch.empty((B, S, (D + 3) * 8), dtype=torch.float32, device=s_points.device)
        # qlen None: a null pointer, and the entry is mcp_pointconv_agg itself
        _call("mcp_pointconv_agg_lengths", s_points, B, N, S, D, idx.shape[-1], _lib.fptr(s_xyz), _lib.fptr(new_xyz), _lib.fptr(s_points),
              _lib.iptr(idx), _len_ptr(qlen), _lib.fptr(w0), _lib.fptr(b0), _lib.fptr(w1), _lib.fptr(b1), _lib.fptr(w2), _lib.fptr(b2),
              _lib.fptr(out))
        return out

    _PCL_MIN_ROWS = 16384   # from here mcp_linear runs linear_kernel, whose arithmetic the one-launch form reproduces bit for bit

    def pointconv_linear_supported(self, d, c_out, k=32, rows=None):
        """Shapes mcp_pointconv_linear is built for (levels 0 / 1 of the encoder and the refinement stage's PointConvD).  With
        `rows` (= B * S centres): whether the model should use it -- only where its output is bit-identical to pointconv_agg +
        linear, i.e. where that Linear would run the full-K kernel and not the split-K / library forms of the few-row launches."""
        return k == 32 and (d, c_out) in ((32, 32), (64, 64)) and (rows is None or rows >= self._PCL_MIN_ROWS)

    def pointconv_linear_pack(self, w, b):
        """Operand image of PointConv's Linear: the same image linear() uses for the (B,S,(3+D)*8) aggregate."""
        return self.linear_pack(w, b, [w.shape[1]])

    def pointconv_linear(self, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, w, b, slope, packed=None, centre_lengths=None):
        """PointConv after the sampling in one launch (mocopci.py:1330-1342): grouping, WeightNet, aggregation, Linear, LeakyReLU ->
        (B,S,C_out).  Inference only (a training forward uses pointconv_agg + linear, which carry gradients).
        packed: pointconv_linear_pack(w, b) if kept.  centre_lengths: as in pointconv_agg; a padded centre's row is zero, not
        leaky(bias)."""
        s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2 = (t.contiguous() for t in (s_xyz, new_xyz, s_points, w0, b0, w1, b1, w2, b2))
        B, N, D = s_points.shape
        S, n = new_xyz.shape[1], w.shape[0]
        pk = packed if packed is not None else self.pointconv_linear_pack(w, b)
        out = torch.empty((B, S, n), dtype=torch.float32, device=s_points.device)
        qlen = lengths_tensor(centre_lengths, B, S, s_points.device)   # None stays None: the entry is then mcp_pointconv_linear itself
        _call("mcp_pointconv_linear_lengths", s_points, B, N, S, D, idx.shape[-1], _lib.fptr(s_xyz), _lib.fptr(new_xyz),
              _lib.fptr(s_points), _lib.iptr(idx), _len_ptr(qlen), _lib.fptr(w0), _lib.fptr(b0), _lib.fptr(w1), _lib.fptr(b1),
              _lib.fptr(w2), _lib.fptr(b2), _lib.fptr(pk), n, float(slope), _lib.fptr(out))
        return out

    def attention(self, q, kv, heads, scale=None, dropout_p=0.0, query_lengths=None, key_lengths=None):
        """softmax(q k^T * scale) v per head, reading the projection outputs in place: q (BF,Nq,C), kv (BF,Nk,2C)
        laid out [k | v] as the reference's kv Linear produces (mocopci.py:74-75, :653-654) -> (BF,Nq,C).  dropout_p > 0: attention
        dropout on the softmax matrix inside the kernel (head dims 8 / 16 / 32 / 64 / 256), the mask a counter-based hash seeded from
        torch's CPU generator (reproducible under torch.manual_seed; see mcp_attention_small_dropout, mcp_attention_wide_dropout).
        query_lengths / key_lengths: per-element lengths of a padded batch (see lengths_tensor; None = full): rows below the query
        length attend to the keys below the key length; rows at or beyond it, and every row of an element without keys, are zeros, as
        are the gradients of padded rows.  Padding may hold anything (NaN, inf).  No synchronisation."""
        BF, Nq, C = q.shape
        Nk = kv.shape[1]
        hd = C // heads
        if scale is None:
            scale = hd ** -0.5
        qlen = lengths_tensor(query_lengths, BF, Nq, q.device)   # None stays None
        klen = lengths_tensor(key_lengths, BF, Nk, q.device)
        if hd not in (8, 16, 32, 64, 256):  # head dims neither kernel is built for: the dense (masked) formulation, the twins' arithmetic
            if dropout_p > 0.0:
                raise RuntimeError("attention dropout inside the kernel: head dims 8 / 16 / 32 / 64 / 256")
            if qlen is None and klen is None:
                return grad.attention_twin(q, kv, heads, float(scale))
            return grad.attention_lengths_twin(q, kv, heads, float(scale), qlen, klen)
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if dropout_p > 0.0 else 0  # CPU generator: no device synchronisation
        if grad.wants_grad(q, kv):
            fn = _AttentionSmallFn if hd in (8, 16) else _AttentionWideFn
            return fn.apply(self, q, kv, heads, float(scale), float(dropout_p), seed, qlen, klen)
        return self._attention(q, kv, heads, float(scale), float(dropout_p), seed, qlen, klen)

    def _attention(self, q, kv, heads, scale, drop_p=0.0, seed=0, qlen=None, klen=None):
        """The forward alone: qlen / klen (BF,) int32 device tensors or None.  With both None the *_lengths entries below are the dense
        ones (mcp_attention; mcp_attention_{small,wide}_dropout, which is the *_lse forward without its log-sum-exp).
        Head dims 8/16: S on MFMA, P.V on packed FMAs; 32/64/256 (ei3, Cross_Frame_Att): both products on MFMA."""
        q, kv = q.contiguous(), kv.contiguous()
        BF, Nq, C = q.shape
        Nk, hd = kv.shape[1], C // heads
        out = torch.empty((BF, Nq, C), dtype=torch.float32, device=q.device)
        if drop_p > 0.0:   # the training forward without its log-sum-exp
            _call(_AttentionFn._family(hd) + "_lse_lengths", q, BF, Nq, Nk, heads, hd, q.data_ptr(), C, kv.data_ptr(), 2 * C, kv.data_ptr() + 4 * C, 2 * C,
                  float(scale), float(drop_p), int(seed), out.data_ptr(), None, _len_ptr(qlen), _len_ptr(klen))
            return out
        _call("mcp_attention_lengths", q, BF, Nq, Nk, heads, hd, q.data_ptr(), C, kv.data_ptr(), 2 * C, kv.data_ptr() + 4 * C, 2 * C, 0,
              float(scale), _len_ptr(qlen), _len_ptr(klen), out.data_ptr(), C)
        return out

    _attention_lengths = _attention   # the name the padded-batch callers use, same arguments

    def prelu_dropout(self, z, slope, drop_p):
        """dropout(prelu(z, slope), drop_p) of a training forward (Mlp_T's act + drop, mocopci.py:1561-1562) as one pass, with a
        one-pass backward; slope: the layer's 1-element parameter.  The mask is a counter-based hash seeded from torch's CPU
        generator per call (reproducible under torch.manual_seed), as in attention()."""
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())  # CPU generator: no device synchronisation
        if slope.numel() != 1:
            raise RuntimeError("prelu_dropout: one slope for all channels (nn.PReLU())")
        return _PreluDropFn.apply(z, slope, float(drop_p), seed)

    def attention_rot(self, q, k, v, heads, kv_shift, scale=None, query_lengths=None, key_lengths=None):
        """Attention over one stacked batch whose keys / values come from batch element (b + kv_shift) mod BF: q, k, v are
        (BF,N,C) views with unit channel stride (e.g. column slices of one packed projection, read in place).  Inference only.
        query_lengths / key_lengths: as attention(); key_lengths is indexed by the k / v tensors' own batch element, so the queries
        of element b see key_lengths[(b + kv_shift) mod BF]."""
        BF, Nq, C = q.shape
        Nk, hd = k.shape[1], C // heads
        for t, n in ((q, Nq), (k, Nk), (v, Nk)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(0) == n * t.stride(1)):
                raise RuntimeError("attention_rot: (BF,N,C) float32 CUDA views with unit channel stride and dense batches")
        out = torch.empty((BF, Nq, C), dtype=torch.float32, device=q.device)
        qlen, klen = lengths_tensor(query_lengths, BF, Nq, q.device), lengths_tensor(key_lengths, BF, Nk, q.device)   # None stays None
        _call("mcp_attention_lengths", q, BF, Nq, Nk, heads, hd, q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), v.data_ptr(),
              v.stride(1), int(kv_shift), float(hd ** -0.5 if scale is None else scale), _len_ptr(qlen), _len_ptr(klen), out.data_ptr(), C)
        return out

    def add_layernorm(self, x, y=None, bias=None, eps=1e-6):
        """(z - mean z) * rsqrt(var z + eps) over the last axis, z = x (+ y) (+ bias): one kernel (csrc/norm.hip).  Inference only."""
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        y2 = None if y is None else y.reshape(-1, C)
        if x2.stride(1) != 1 or (y2 is not None and y2.stride(1) != 1):
            raise RuntimeError("add_layernorm: unit channel stride")
        out = torch.empty((x2.shape[0], C), dtype=torch.float32, device=x.device)
        _call("mcp_add_layernorm", x, x2.shape[0], C, _lib.fptr(x2) if x2.is_contiguous() else x2.data_ptr(), x2.stride(0),
              None if y2 is None else y2.data_ptr(), 0 if y2 is None else y2.stride(0), None if bias is None else _lib.fptr(bias), None, None,
              float(eps), _lib.fptr(out), C)
        return out.reshape(x.shape)

    def mfa_prepare(self, fea, src_self, src_partner, te_self, te_partner, scale, shift):
        """(x, xn, xr) of Multi_Frame_Att from the computed flow embeddings in one launch (csrc/norm.hip): fea (M,N,C), index lists
        (R,) int32, time codes (R,C), norm1's eval scale / shift (C) -> three (R,N,C) tensors.  Inference only."""
        M, N, C = fea.shape
        R = src_self.shape[0]
        x, xn, xr = (torch.empty((R, N, C), dtype=torch.float32, device=fea.device) for _ in range(3))
        _call("mcp_mfa_prepare", fea, R, N, C, _lib.fptr(fea), _lib.iptr(src_self), _lib.iptr(src_partner), _lib.fptr(te_self), _lib.fptr(te_partner),
              _lib.fptr(scale), _lib.fptr(shift), _lib.fptr(x), _lib.fptr(xn), _lib.fptr(xr))
        return x, xn, xr

    # ---- per-point Linear with fused epilogue (csrc/linear.hip) ----
    @staticmethod
    def _pieces(xs):
        """The input pieces as 2-D row views (rows, k_i) with unit channel stride, 16-byte aligned rows; None if one of them
        cannot be read in place."""
        out = []
        for t in (xs if isinstance(xs, (tuple, list)) else (xs,)):
            k = t.shape[-1]
            v = t.reshape(-1, k) if t.is_contiguous() else (t if t.dim() == 2 else None)
            if v is None and t.stride(-1) == 1:  # a last-axis slice of a contiguous tensor: rows keep the parent's stride
                lead = t.shape[:-1]
                st = t.stride()
                ok = all(st[i] == st[i + 1] * lead[i + 1] for i in range(len(lead) - 1))
                v = t.as_strided((t.numel() // k, k), (st[-2], 1)) if ok else None
            if v is None or v.stride(1) != 1 or v.stride(0) % 4 or v.data_ptr() % 16 or k % 4 or v.dtype != torch.float32 or not v.is_cuda:
                return None
            out.append(v)
        return out

    def linear_supported(self, xs, n, few_rows=True, policy_rows=None):
        """Whether linear() takes this call.  policy_rows: decide (and run, see linear()) as for that many rows -- a caller that
        computes a subset of the rows of a tall product asks for the tall product's kernel, so that both give the same bits.  Beyond what the kernel can do, a shape policy: the fused kernel beats the BLAS
        chain for tall inputs with moderate K (tools/linear_ab.py, MI355X: 1.3-1.9x at rows >= 16384, K <= 320, e.g. 58 -> 31 us
        for 196608 x 32 -> 64 + LeakyReLU) and, since its K loop is staged four chunks per barrier, for the K = 536 -> 64 PointConv
        projections (171 -> 146 us at 196608 rows); it loses for few rows (one 256-row workgroup per 8 waves: 2048-8192 rows do
        not cover the chip) and for long K at wide N (2072 -> 256), which stay on the library.  few_rows=False: without the
        split-K few-row kernel (a training forward keeps the library's fp32 GEMMs there, as the gradient tests were pinned)."""
        if self._NO_LINEAR:
            return False
        ps = self._pieces(xs)
        if ps is None or len(ps) > 3 or len({p.shape[0] for p in ps}) != 1:
            return False
        k = sum(p.shape[1] for p in ps)
        rows = ps[0].shape[0] if policy_rows is None else int(policy_rows)
        if few_rows and self._LIN_FEW_MIN_ROWS <= rows < self._LIN_MIN_ROWS:
            # few rows (the lower pyramid levels): the split-K kernel -- four waves share a 32-row tile and split its K chunks -- beats
            # the library GEMM + activation pair up to 256 output columns (tools/linear_fewrows_ab.py: 33 -> 26 us at 4096 x 1048 ->
            # 256, 25 -> 12 us at 8192 x 128 -> 128); wider outputs re-read and re-split x per 64-column block and lose
            if n > 256 or k < 64 or k > self._LIN_FEW_MAX_K:
                return False
        elif rows < self._LIN_MIN_ROWS or n > self._LIN_MAX_N or (k > self._LIN_MAX_K and not (k <= 2 * self._LIN_MAX_K and n <= 64)):
            return False
        ks = (ctypes.c_int * len(ps))(*[p.shape[1] for p in ps])
        return _lib.load().mcp_linear_packed_floats(n, len(ps), ks) != 0

    def linear_kernel_ok(self, x2d, n):
        """Whether the fused Linear KERNEL can take (rows, K) -> n at all (capability, not the inference shape policy above): used by
        the backward products, where the alternative is a library GEMM on a tall, narrow operand."""
        ps = self._pieces(x2d)
        if self._NO_LINEAR or ps is None or len(ps) != 1:
            return False
        ks = (ctypes.c_int * 1)(ps[0].shape[1])
        return _lib.load().mcp_linear_packed_floats(n, 1, ks) != 0

    # shape policy of the fused Linear (measured optimum; tools/linear_ab.py overrides them on the class)
    _NO_LINEAR = False
    _NO_NARROW = False
    _LIN_MIN_ROWS = 16384
    _LIN_FEW_MIN_ROWS = 2048   # rows from which the split-K few-row kernel is used (0 < rows < _LIN_MIN_ROWS); 1 << 30 turns it off
    _LIN_FEW_MAX_K = 1100
    _LIN_MAX_K = 320
    _LIN_MAX_N = 192

    def linear_pack(self, w, b, ks):
        """Operand image of one Linear whose K axis is the concatenation of pieces of widths ks (split once per layer)."""
        n = w.shape[0]
        kk = (ctypes.c_int * len(ks))(*ks)
        nf = _lib.load().mcp_linear_packed_floats(n, len(ks), kk)
        if nf == 0:
            raise RuntimeError(f"linear does not support n={n}, pieces={list(ks)}")
        packed = torch.empty((nf,), dtype=torch.float32, device=w.device)
        _call("mcp_linear_pack", w, n, len(ks), kk, _lib.fptr(w.contiguous()), None if b is None else _lib.fptr(b.contiguous()), _lib.fptr(packed))
        return packed

    def linear(self, xs, w, b=None, slope=1.0, res=None, packed=None, policy_rows=None):
        """act(W [x_0 | x_1 | x_2] + b) [+ res] over the last axis (policy_rows: the kernel of a product with that many rows, see
        linear_supported): xs one tensor or up to three pieces of a concatenation (read in
        place, column slices allowed); act(v) = v > 0 ? v : slope v (1.0: none, 0.1: LeakyReLU, 0: ReLU, a PReLU slope).
        One kernel instead of cat + GEMM + activation + add.  Differentiable.  packed: linear_pack(w, b, widths) if kept.  A kept
        pack belongs to one piece layout (each piece is padded to whole 32-channel chunks): pieces that want a gradient run
        concatenated, on a pack of the concatenation, and the kept one is not used there."""
        def fused(xs_, w_, b_, slope_, res_, packed_=packed):
            ps = self._pieces(xs_)
            ks = [p.shape[1] for p in ps]
            pk = packed_ if packed_ is not None else self.linear_pack(w_, b_, ks)
            rows, n = ps[0].shape[0], w_.shape[0]
            first = xs_[0] if isinstance(xs_, (tuple, list)) else xs_
            out = torch.empty((rows, n), dtype=torch.float32, device=first.device)
            r2 = None if res_ is None else res_.reshape(rows, n).contiguous()
            xp = (ctypes.c_void_p * len(ps))(*[p.data_ptr() for p in ps])
            st = (ctypes.c_int * len(ps))(*[p.stride(0) for p in ps])
            kk = (ctypes.c_int * len(ps))(*ks)
            _call("mcp_linear_as", first, rows, rows if policy_rows is None else int(policy_rows), n, len(ps), xp, st, kk, float(slope_), _lib.fptr(pk),
                  None if r2 is None else _lib.fptr(r2), n, _lib.fptr(out), n)
            return out.reshape(*first.shape[:-1], n)
        if isinstance(xs, (tuple, list)) and grad.wants_grad(*xs, w, b, res):
            # training: the pieces are concatenated (autograd splits the gradient again) so that the layer takes the explicit
            # backward below -- the streaming dx / dW kernels -- instead of plain autograd over library GEMMs.  The caller's pack
            # is laid out for the pieces ([36, 36] pads to 4 chunks, [72] has 3), so the concatenation is packed for itself.
            cat = torch.cat(list(xs), dim=-1)
            if isinstance(slope, (int, float)) and 0.0 <= slope <= 1.0 and self.linear_supported(cat, w.shape[0], few_rows=False):
                return _LinearFn.apply(lambda *a: fused(*a, packed_=None), cat, w, b, float(slope), res)
            return grad.linear_twin(cat, w, b, slope, res)
        if grad.wants_grad(xs, w, b, res) and isinstance(slope, (int, float)) and 0.0 <= slope <= 1.0:
            return _LinearFn.apply(fused, xs, w, b, float(slope), res)
        return grad.run(fused, grad.linear_twin, xs, w, b, slope, res)

    def linear_narrow_supported(self, rows, k, n):
        """act-then-Linear with at most 4 outputs over K in {256, 512, 1024} (see linear_narrow)."""
        return not (self._NO_LINEAR or self._NO_NARROW) and n <= 4 and k in (256, 512, 1024) and rows >= 1024

    def linear_narrow(self, x, w, b, in_slope):
        """b + W . act(x) over the last axis, act(v) = v > 0 ? v : in_slope v, W (n <= 4, K): the flow tail of Mlp_T (PReLU, then
        fc2 and mapping_xyz as one 4C -> 3 map) as one streaming kernel instead of an activation launch and a 3-column GEMM."""
        def fused(x_, w_, b_, slope_):
            x2 = x_.reshape(-1, x_.shape[-1])
            x2 = x2 if x2.stride(1) == 1 and x2.stride(0) % 4 == 0 and x2.data_ptr() % 16 == 0 else x2.contiguous()
            rows, k, n = x2.shape[0], x2.shape[1], w_.shape[0]
            out = torch.empty((rows, n), dtype=torch.float32, device=x_.device)
            _call("mcp_linear_narrow", x_, rows, k, n, _lib.fptr(x2) if x2.is_contiguous() else x2.data_ptr(), x2.stride(0), _lib.fptr(w_.contiguous()),
                  None if b_ is None else _lib.fptr(b_.contiguous()), float(slope_), _lib.fptr(out), n)
            return out.reshape(*x_.shape[:-1], n)
        twin = lambda x_, w_, b_, slope_: torch.nn.functional.linear(torch.where(x_ > 0, x_, x_ * slope_), w_, b_)
        return grad.run(fused, twin, x, w, b, in_slope)

    def mlp2_pack(self, w1, b1, w2, b2):
        """Operand image of one two-layer MLP for mlp2 (split once; do this once per block).  A bias given as None is packed as zeros."""
        hidden, cin = w1.shape
        cout = w2.shape[0]
        n = _lib.load().mcp_mlp2_packed_floats(cin, hidden, cout)
        if n == 0:
            raise RuntimeError(f"mlp2 does not support cin={cin}, hidden={hidden}, cout={cout}")
        if b1 is None:
            b1 = torch.zeros((hidden,), dtype=torch.float32, device=w1.device)
        if b2 is None:
            b2 = torch.zeros((cout,), dtype=torch.float32, device=w1.device)
        packed = torch.empty((n,), dtype=torch.float32, device=w1.device)
        _call("mcp_mlp2_pack", w1, cin, hidden, cout, _lib.fptr(w1.contiguous()), _lib.fptr(b1.contiguous()), _lib.fptr(w2.contiguous()),
              _lib.fptr(b2.contiguous()), _lib.fptr(packed))
        return packed

    def mlp2(self, x, w1, b1, w2, b2, slope, res=None, packed=None):
        """out = [res +] W2 act(W1 x + b1) + b2 over the last axis, act = PReLU with one slope: Mlp_T and the flow heads of the
        frame-attention blocks (mocopci.py:1558-1565, :566-567, :510-511) as ONE kernel; the hidden activation is never written.
        x (..., cin) -> (..., cout); slope: a float, or the 1-element PReLU parameter (then it receives a gradient too).
        Differentiable w.r.t. x, res and the weights.  packed: mlp2_pack(w1, b1, w2, b2) when the caller keeps one."""
        def fused(x_, res_, w1_, b1_, w2_, b2_, slope_):
            pk = packed if packed is not None else self.mlp2_pack(w1_, b1_, w2_, b2_)
            cin, hidden, cout = w1_.shape[1], w1_.shape[0], w2_.shape[0]
            x2 = x_.reshape(-1, cin)
            if not (x2.stride(1) == 1 and x2.stride(0) % 4 == 0 and x2.data_ptr() % 16 == 0):
                x2 = x2.contiguous()
            r2 = None if res_ is None else res_.reshape(-1, cout).contiguous()
            out = torch.empty((x2.shape[0], cout), dtype=torch.float32, device=x_.device)
            _call("mcp_mlp2", x_, x2.shape[0], cin, hidden, cout, float(slope_), x2.data_ptr(), x2.stride(0), None if r2 is None else _lib.fptr(r2), cout,
                  _lib.fptr(pk), _lib.fptr(out), cout)
            return out.reshape(*x_.shape[:-1], cout)
        if grad.wants_grad(x, res, w1, b1, w2, b2, slope) and b2 is not None:
            return _Mlp2Fn.apply(fused, x, res, w1, b1, w2, b2, slope)
        return grad.run(fused, grad.mlp2_twin, x, res, w1, b1, w2, b2, slope)

    def mlp2_supported(self, cin, hidden, cout):
        """Shapes the fused kernel is built for (the ones where it beats the BLAS chain); A/B tools set _NO_MLP2 on the class."""
        return not self._NO_MLP2 and _lib.load().mcp_mlp2_packed_floats(cin, hidden, cout) != 0

    _NO_MLP2 = False

    EXPLICIT_CHAMFER_GRAD = True

    def chamfer(self, x, y, per_sample=False, x_lengths=None, y_lengths=None):
        """chamfer_loss (models/utils.py:36-45; pytorch3d defaults): x (B,N,3), y (B,M,3) -> 0-dim tensor.  As a training loss
        (train.py:135-160) it is differentiable w.r.t. both clouds: the nearest neighbours come from the search kernel and the
        squared distances to them are re-evaluated differentiably.  per_sample: the (B,) values whose mean that is -- several terms
        of the objective that share a ground-truth cloud are then ONE call on a stacked batch (training.multiscale_loss).
        x_lengths / y_lengths (forms: lengths_tensor): only x[b, :xl] and y[b, :yl] count; the value of sample b is
        sum_{i<xl} d_i / max(xl,1) + sum_{j<yl} d_j / max(yl,1), gradient rows at or beyond a length are exact zeros, and padded
        rows are never read.  Without lengths nothing changes."""
        if x_lengths is not None or y_lengths is not None:
            B, N, _ = x.shape
            M = y.shape[1]
            xl, yl = lengths_tensor(x_lengths, B, N, x.device), lengths_tensor(y_lengths, B, M, x.device)
            if grad.wants_grad(x, y):
                v = _ChamferLengthsFn.apply(self, x, y, xl, yl)
            else:
                x, y = x.contiguous(), y.contiguous()
                if self.prunes_with_lengths(N, M, 1) or self.prunes_with_lengths(M, N, 1):
                    # a direction whose padded shapes qualify takes the pruned search, the other one the exhaustive kernels (knn
                    # decides); one scope, so a cloud that is query here and reference there is sorted once
                    with self.cloud_scope():
                        dxy = self.knn(x, y, 1, mode=MCP_DIST_DIRECT, return_dist=True, query_lengths=xl, ref_lengths=yl)[1][..., 0]
                        dyx = self.knn(y, x, 1, mode=MCP_DIST_DIRECT, return_dist=True, query_lengths=yl, ref_lengths=xl)[1][..., 0]
                else:
                    dxy = torch.empty((B, N), dtype=torch.float32, device=x.device)
                    dyx = torch.empty((B, M), dtype=torch.float32, device=x.device)
                    _call("mcp_chamfer_nn_lengths", x, B, N, M, _lib.fptr(x), _lib.fptr(y), None if xl is None else _lib.iptr(xl),
                          None if yl is None else _lib.iptr(yl), _lib.fptr(dxy), _lib.fptr(dyx))
                v = (dxy.sum(1) / _valid_counts(xl, B, N, x.device).clamp(min=1).float()
                     + dyx.sum(1) / _valid_counts(yl, B, M, x.device).clamp(min=1).float())
            return v if per_sample else v.mean()
        if grad.wants_grad(x, y):
            if self.EXPLICIT_CHAMFER_GRAD:
                v = _ChamferFn.apply(self, x, y)
                return v if per_sample else v.mean()
            x, y = x.contiguous(), y.contiguous()   # A/B: autograd over the unfused form
            ixy = self.knn(x.detach(), y.detach(), 1, mode=MCP_DIST_DIRECT)[..., 0].contiguous()
            iyx = self.knn(y.detach(), x.detach(), 1, mode=MCP_DIST_DIRECT)[..., 0].contiguous()
            return grad.chamfer_twin(self.group_rows, x, y, ixy, iyx, per_sample)
        B, N, _ = x.shape
        M = y.shape[1]
        dxy = torch.empty((B, N), dtype=torch.float32, device=x.device)
        dyx = torch.empty((B, M), dtype=torch.float32, device=x.device)
        _call("mcp_chamfer_nn", x, B, N, M, _lib.fptr(x), _lib.fptr(y), _lib.fptr(dxy), _lib.fptr(dyx))
        v = dxy.mean(1) + dyx.mean(1)
        return v if per_sample else v.mean()


_backend = HipBackend()


def backend():
    return _backend


def set_backend(b):
    """Swap the operator backend (tests / cpu_baseline only). Returns the previous one."""
    global _backend
    prev, _backend = _backend, b
    return prev


# ---- instrumentation passthrough (bench.py) ----
KERNEL_IDS = {"fps": 1, "knn": 2, "group_rows": 3, "interp3": 4, "knn_cosine": 5, "fusion": 6, "cross": 7, "pointconv": 8, "attention": 9, "ptblock": 10, "mlp": 11, "linear": 12}


def prof_enable(kernel_names):
    """Time every launch of the named kernels (iterable of KERNEL_IDS keys) with hipEvents; None/() disables."""
    mask = 0
    for name in (kernel_names or ()):
        mask |= 1 << KERNEL_IDS[name]
    _lib.check(_lib.load().mcp_prof_enable(mask))


def prof_collect(kernel_name):
    n = ctypes.c_int(0)
    ms = ctypes.c_float(0.0)
    _lib.check(_lib.load().mcp_prof_collect(KERNEL_IDS[kernel_name], ctypes.byref(n), ctypes.byref(ms)))
    return n.value, ms.value
