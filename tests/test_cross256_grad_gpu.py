"""-m gpu: the hand-written backward of the D = 256 cost volume (mcp_cross256_grad, csrc/cross256_grad.hip) behind
HipBackend.cross_layer: against autograd over the unfused layer (grad.cross_twin) on the device, against float64 autograd over the
same layer, bit-reproducibility, the C ABI's error contract, and the autograd graph (no RecomputeFn node any more).

Bounds: max|hip - ref| <= 2e-4 max|ref| + 2e-5 per gradient, the project's bound for the D = 64 / 128 kernels (tests/test_grad_gpu.py),
for both references.  (point, channel) pairs whose arg-max neighbour or LeakyReLU branch is decided by rounding -- found in float64
by that test's rule, unchanged -- get a zero upstream gradient; the rule must keep more than 0.9 of the pairs."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from mocopci_amd import _lib, grad, ops
from tests.fused_grad_reference import cross_clear

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["xyz1", "xyz2", "points1", "points2", "wpos", "bpos", "wmlp", "bmlp"]
D = 256


def cloud(seed, b, n, scale=10.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(b, n, 3, generator=g) * 2 - 1) * scale


def rnd(seed, *shape, scale=1.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale


def graph_nodes(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(nx for nx, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


def inputs(b, n1, n2):
    xyz1, xyz2 = cloud(140, b, n1).to(DEV), cloud(141, b, n2).to(DEV)
    f1, f2 = rnd(142, b, n1, D).to(DEV), rnd(143, b, n2, D).to(DEV)
    w = [rnd(144, D, 3, scale=0.3).to(DEV), rnd(145, D, scale=0.1).to(DEV), rnd(146, D, D, scale=D ** -0.5).to(DEV), rnd(147, D, scale=0.1).to(DEV)]
    return xyz1, xyz2, f1, f2, w, rnd(148, b, n1, D).to(DEV)


def layer64(xyz1, xyz2, f1, f2, idx, wpos, bpos, wmlp, bmlp):
    """The layer in float64 up to z (B,N1,K,D); idx (B,N1,K) long."""
    bi = torch.arange(xyz1.shape[0], device=xyz1.device).view(-1, 1, 1)
    u = f2[bi, idx] + f1.unsqueeze(2) + (xyz2[bi, idx] - xyz1.unsqueeze(2)) @ wpos.T + bpos
    return u, F.leaky_relu(u, 0.1) @ wmlp.T + bmlp


def test_new_entry_points_exist_and_the_old_one_keeps_its_answer():
    lib = _lib.load()
    assert lib.mcp_cross256_grad_floats() == 256 * 256 + 5 * 256
    assert lib.mcp_cross_grad_floats(256) == 0          # unchanged on purpose
    assert lib.mcp_cross256_grad_workspace_bytes(16, 256) > 0 and lib.mcp_cross256_grad_workspace_bytes(0, 256) == 0


def test_cross_layer_at_256_has_no_recompute_node():
    be = ops.backend()
    xyz1, xyz2, f1, f2, w, _ = inputs(2, 300, 300)
    half = be.knn(xyz1, xyz2, 16)
    for idx in ((half, half), be.knn(xyz1, xyz2, 32)):
        leaves = [t.clone().requires_grad_(True) for t in (xyz1, xyz2, f1, f2, *w)]
        out = be.cross_layer(*leaves[:4], idx, *leaves[4:])
        names = graph_nodes(out)
        assert "RecomputeFnBackward" not in names and "_CrossFnBackward" in names, names
        with torch.no_grad():   # forward bits are the inference kernel's
            assert torch.equal(out.detach(), be.cross_layer(xyz1, xyz2, f1, f2, idx, *w))


@pytest.mark.parametrize("b,n1,n2", [(3, 1237, 1500), (16, 256, 256), (1, 40, 40)], ids=["ragged", "training-shape", "40-points"])
def test_cross256_backward_matches_the_unfused_layer_and_float64_and_repeats_bit_for_bit(b, n1, n2):
    """Construction of test_cross_backward_kernel_matches_the_unfused_layer_and_repeats_bit_for_bit (tests/test_grad_gpu.py) at d = 256:
    identical 16 + 16 halves (every maximum tied between two list positions) and one 32-list; a ragged point count, the training shape
    (both directions stacked: 16 x 256), and one cloud of 40 points (fewer than one workgroup takes per round)."""
    be = ops.backend()
    xyz1, xyz2, f1, f2, w, g0 = inputs(b, n1, n2)
    half = be.knn(xyz1, xyz2, 16)

    def grads(fn, idx, g):
        leaves = [t.detach().clone().requires_grad_(True) for t in (xyz1, xyz2, f1, f2, *w)]
        return torch.autograd.grad(fn(*leaves[:4], idx, *leaves[4:]), leaves, g)
    for form, idx in (("halves", (half, half)), ("32-list", be.knn(xyz1, xyz2, 32))):
        uniq = (idx[0] if isinstance(idx, tuple) else idx).long()
        d64 = [t.double() for t in (xyz1, xyz2, f1, f2, *w)]
        u64, z64 = layer64(*d64[:4], uniq, *d64[4:])
        clear = cross_clear(u64, z64)
        del u64, z64
        kept = float(clear.float().mean())
        print(f"\n[{form} b={b} n1={n1}] kept (point, channel) pairs: {kept:.3f}")
        assert kept > 0.9
        g = g0 * clear.float()
        hip = grads(be.cross_layer, idx, g)
        again = grads(be.cross_layer, idx, g)
        twin = grads(lambda a, b_, c, e, i, *ww: grad.cross_twin(be.group_rows, a, b_, c, e, i, *ww), idx, g)
        # float64 autograd over the same layer with the same masked upstream gradient
        leaves64 = [t.clone().requires_grad_(True) for t in d64]
        whole = grad.whole(idx).long()
        out64 = F.leaky_relu(layer64(*leaves64[:4], whole, *leaves64[4:])[1], 0.1).max(dim=2)[0]
        ref = torch.autograd.grad(out64, leaves64, g.double())
        del out64
        print(f"{'gradient':9s} {'max|f64|':>10s} {'hip-f64':>10s} {'twin-f64':>10s} {'ratio':>7s} {'hip-twin':>10s}")
        failures = []
        for name, a, a2, t32, r64 in zip(NAMES, hip, again, twin, ref):
            e_hip, e_twin = float((a.double() - r64).abs().max()), float((t32.double() - r64).abs().max())
            e_ht, s64, s32 = float((a - t32).abs().max()), float(r64.abs().max()), float(t32.abs().max())
            print(f"{name:9s} {s64:10.3e} {e_hip:10.3e} {e_twin:10.3e} {e_hip / max(e_twin, 1e-30):7.2f} {e_ht:10.3e}")
            if not torch.equal(a, a2):
                failures.append(f"{name}: two runs differ")
            if not torch.isfinite(a).all():
                failures.append(f"{name}: not finite")
            if not e_ht <= 2e-4 * s32 + 2e-5:
                failures.append(f"{name}: |hip - twin| {e_ht:.2e}, gradient scale {s32:.2e}")
            if not e_hip <= 2e-4 * s64 + 2e-5:
                failures.append(f"{name}: |hip - f64| {e_hip:.2e}, gradient scale {s64:.2e}")
        assert not failures, f"[{form}] " + "; ".join(failures)


def test_cross256_grad_rejects_bad_arguments_without_launching():
    lib = _lib.load()
    b, n = 1, 64
    f = lambda *s: torch.zeros(*s, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    xyz, pts, idx = f(b, n, 3), f(b, n, D), torch.zeros(b, n, 32, dtype=torch.int32, device=DEV)
    w = [f(D, 3), f(D), f(D, D), f(D)]
    need = lib.mcp_cross256_grad_workspace_bytes(b, n)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    outs = [torch.full(s, 7.0, device=DEV) for s in ((b, n, 3), (b, n, 32, 3), (b, n, D), (b, n, 32, D), (lib.mcp_cross256_grad_floats(),))]

    def call(k, wsb, weights=True):
        o = [P(t) for t in outs]
        if not weights:
            o[4] = None
        return lib.mcp_cross256_grad(b, n, n, k, P(xyz), P(xyz), P(pts), P(pts), P(idx), None, *[P(t) for t in w], P(pts), *o, P(ws), wsb, st)
    assert call(31, need) == 10002                 # MCP_ERR_UNSUPPORTED: the layer's k is 32
    assert call(32, need - 1) == 10001             # MCP_ERR_BAD_ARG: workspace one byte short
    assert call(32, need, weights=False) == 10001  # MCP_ERR_BAD_ARG: null grad_weights
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs) and not bool(ws.any())   # nothing ran
    assert call(32, need) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 0.0).all()) for t in outs)   # zero upstream gradient: every output written, all zeros


def test_equal_maxima_go_to_the_lowest_list_position():
    """The ABI's tie rule, seen directly in the per-neighbour outputs: with a 32-list whose second half repeats the first, every
    maximum is tied between positions j and j + 16, and only positions 0..15 may receive a gradient."""
    lib, be = _lib.load(), ops.backend()
    b, n = 2, 300
    xyz1, xyz2, f1, f2, w, g = inputs(b, n, n)
    half = be.knn(xyz1, xyz2, 16)
    idx = torch.cat((half, half), dim=-1).contiguous()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    need = lib.mcp_cross256_grad_workspace_bytes(b, n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    d_xyz1, d_dir, d_p1 = torch.empty(b, n, 3, device=DEV), torch.empty(b, n, 32, 3, device=DEV), torch.empty(b, n, D, device=DEV)
    d_rows, d_w = torch.empty(b, n, 32, D, device=DEV), torch.empty(lib.mcp_cross256_grad_floats(), device=DEV)
    rc = lib.mcp_cross256_grad(b, n, n, 32, P(xyz1), P(xyz2), P(f1), P(f2), P(idx), None, *[P(t) for t in w], P(g), P(d_xyz1), P(d_dir), P(d_p1),
                               P(d_rows), P(d_w), P(ws), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((d_rows[:, :, 16:] == 0).all()) and bool((d_dir[:, :, 16:] == 0).all())
    assert float(d_rows[:, :, :16].abs().max()) > 0.1 and float(d_dir[:, :, :16].abs().max()) > 0.1
    # the same list as its two halves: the same bits
    d_rows2, d_dir2, d_w2 = torch.empty_like(d_rows), torch.empty_like(d_dir), torch.empty_like(d_w)
    rc = lib.mcp_cross256_grad(b, n, n, 32, P(xyz1), P(xyz2), P(f1), P(f2), P(half), P(half), *[P(t) for t in w], P(g), P(d_xyz1), P(d_dir2), P(d_p1),
                               P(d_rows2), P(d_w2), P(ws), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(d_rows, d_rows2) and torch.equal(d_dir, d_dir2) and torch.equal(d_w, d_w2)
