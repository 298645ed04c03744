"""-m gpu: the backward of the per-point Linear and the two-layer MLP on the routes a training step takes -- the weight-gradient kernel
(csrc/linear_grad.hip) at every tiles-per-wave instantiation, staging form and stage count, the input-gradient products on the
streaming forward kernels (ops._tall_matmul), and the composed backward functions (_Mlp2Fn, _LinearFn, _TorchLinearFn) at row counts
above their thresholds (8192 rows for the input-gradient product, 2048 for the weight gradient) -- against float64.
tests/kernel_variants.py names what each weight-gradient case reaches; test_kernel_variants_cpu.py checks that the cases reach it all.

Tolerances follow the arithmetic.  dW = gz^T x is a `rows`-long sum of exact fp32 products (v_mfma_f32_32x32x2_f32) added in fp32:
an element is within

    c * 2^-24 * sqrt(rows) * (|gz|^T |x|)        (db: c * 2^-24 * sqrt(rows) * sum |gz|)

of the exact value, c = 2 as for the other fp32-accurate products (tests/dense_reference.py).  Every case also shows that the bound is
tight enough to matter: the float64 result WITHOUT the last row -- what a kernel that mishandled its tail would return -- misses it.
The input-gradient products are held to the forward kernels' own bound and two-term self-check; the composed functions to the bound
of test_grad_gpu.compare_grads (2e-4 of the gradient's largest entry + 2e-5) against float64 autograd over the plain formula, and each
of them states which library entry points its backward must reach."""
import math

import pytest
import torch

from mocopci_amd import _lib, ops
from tests import kernel_variants as kv
from tests.dense_reference import SELF_ROWS, U, linear_ratio, positive_mean_data, two_term   # linear_ratio: c = C_LINEAR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_WGRAD = 2.0
SENTINEL = -12345.0
KINK = 1e-4   # an activation input this close to zero has no sign at fp32 precision: its upstream gradient is zeroed on both sides


def _placed(data, spec):
    """The (rows, w) float32 `data` on the device as the case places it: contiguous, or as columns c0 : c0 + w of a (rows, W) tensor
    whose other columns hold NaN.  Returns (view, row stride)."""
    if spec is None:
        return data.to(DEV), data.shape[1]
    W, c0 = spec
    wide = torch.full((data.shape[0], W), float("nan"), device=DEV)
    wide[:, c0:c0 + data.shape[1]] = data.to(DEV)
    return wide[:, c0:c0 + data.shape[1]], W


# ---- mcp_linear_wgrad -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kv.WGRAD_CASES, ids=kv.wgrad_case_id)
def test_linear_wgrad_variant_matches_float64(case):
    lib = _lib.load()
    rows, n = case["rows"], case["n"]
    if case["k"] is None:   # the largest k the entry point takes at this n, found by asking it
        k = next(kk for kk in range(1280, 0, -1) if lib.mcp_linear_wgrad_workspace_bytes(rows, n, kk))
        assert k == kv.wgrad_max_k(n) and lib.mcp_linear_wgrad_workspace_bytes(rows, n, k + 32) == 0
    else:
        k = case["k"]
    _, _, _, gs, xs, go, xo = kv.wgrad_shape(case)
    g = torch.Generator().manual_seed(rows * 7 + n * 3 + k)
    gz_h, x_h = torch.randn(rows, n, generator=g), torch.randn(rows, k, generator=g)
    gz, gs_ = _placed(gz_h, case["gz"])
    x, xs_ = _placed(x_h, case["x"])
    assert (gs_, xs_) == (gs, xs) and gz.data_ptr() % 16 == (4 * go) % 16 and x.data_ptr() % 16 == (4 * xo) % 16   # the launch the mirror describes
    need = lib.mcp_linear_wgrad_workspace_bytes(rows, n, k)
    assert need == kv.wgrad_launch(rows, n, k, gs, xs, go, xo)["workgroups"] * (n * k + n) * 4
    N, c0 = case["block"] or (n, 0)

    def call():
        dw, db = torch.full((N, k), SENTINEL, device=DEV), torch.full((N,), SENTINEL, device=DEV)
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
        ops._call("mcp_linear_wgrad", gz, rows, n, k, gz.data_ptr(), gs, x.data_ptr(), xs, dw.data_ptr() + 4 * c0 * k, db.data_ptr() + 4 * c0, ws.data_ptr(), need)
        return dw, db
    dw, db = call()
    dw2, db2 = call()
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "not bit-reproducible"
    outside = torch.ones(N, dtype=torch.bool, device=DEV)
    outside[c0:c0 + n] = False
    assert bool((dw[outside] == SENTINEL).all()) and bool((db[outside] == SENTINEL).all()), "rows outside the column block were written"
    dw, db = dw[c0:c0 + n].double(), db[c0:c0 + n].double()
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    g64, x64 = gz.double(), x.double()          # the same views: strided cases compare with the reference of the view
    want_w, want_b = g64.T @ x64, g64.sum(0)
    bound_w = C_WGRAD * U * math.sqrt(rows) * (g64.abs().T @ x64.abs())
    bound_b = C_WGRAD * U * math.sqrt(rows) * g64.abs().sum(0)
    ratio_w = float(((dw - want_w).abs() / bound_w).max())
    ratio_b = float(((db - want_b).abs() / bound_b).max())
    # the reference without the last row against the full one: the error of a kernel that dropped it
    drop_w = float((torch.outer(g64[-1], x64[-1]).abs() / bound_w).max())
    drop_b = float((g64[-1].abs() / bound_b).max())
    print(f"RATIO {kv.wgrad_case_id(case)} dW={ratio_w:.3f} db={ratio_b:.3f} dropped_row={drop_w:.1f} dropped_row_db={drop_b:.1f}")
    assert ratio_w <= 1.0, f"dW: error {ratio_w:.2f} x the bound"
    assert ratio_b <= 1.0, f"db: error {ratio_b:.2f} x the bound"
    assert drop_w > 1.0 and drop_b > 1.0, f"the bound does not tell a dropped row from the kernel's result ({drop_w:.2f}, {drop_b:.2f})"


# ---- recorded library calls -------------------------------------------------------------------------------------------------------------
PACK, AS, WGRAD, PRELU, PRELU_GRAD = "mcp_linear_pack", "mcp_linear_as", "mcp_linear_wgrad", "mcp_prelu_dropout", "mcp_prelu_dropout_grad"
STREAMING = {AS, WGRAD, PRELU, PRELU_GRAD, "mcp_mlp2", "mcp_linear_narrow"}


@pytest.fixture
def calls(monkeypatch):
    """The names of the library calls made through ops._call, in order."""
    seen, real = [], ops._call

    def recording(name, *a):
        seen.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops, "_call", recording)
    return seen


# ---- dx = gz W through ops._tall_matmul -----------------------------------------------------------------------------------------------
# (rows, n, k, the kernel of the product or None for the library's GEMM).  8200 x 64 -> 32 has two K chunks: below the split-K
# kernel's four, it runs the main kernel on 4-wave workgroups; the 128 -> 64 product is the split-K one.
DX_CASES = [
    (8200, 64, 32, "linear_kernel<1, 1, 4>"),
    (8200, 128, 64, "linear_splitk_kernel<2>"),     # four K chunks below 16384 rows
    (16390, 64, 32, "linear_kernel<1, 1, 4>"),
    (8200, 64, 256, "linear_kernel<8, 1, 4>"),      # wide outputs (cout -> hidden = 256)
    (16390, 128, 512, "linear_kernel<4, 2, 4>"),    # column blocks of 128 (cout -> hidden = 512)
    (8200, 3, 256, None),                           # the kernel declines K = 3
    (8191, 64, 32, None),                           # below the threshold
]


@pytest.mark.parametrize("rows,n,k,kernel", DX_CASES, ids=[f"{r}x{n}->{k}:{kn or 'library'}" for r, n, k, kn in DX_CASES])
def test_input_gradient_product_matches_float64(rows, n, k, kernel, calls):
    """ops._tall_matmul(gz, w): (rows, n) @ (n, k), the forward kernel on w^T where it takes the shape."""
    if kernel is not None:
        assert kv.expected_kernel("linear", rows=rows, ks=(n,), n=k) == kernel
    g = torch.Generator().manual_seed(rows + 5 * n + k)
    gz, wt, _ = positive_mean_data(g, rows, n, k)      # wt (k, n): the product is gz @ wt^T
    zero = torch.zeros(k)
    gzd, wd = gz.to(DEV), wt.t().contiguous().to(DEV)
    got = ops._tall_matmul(gzd, wd)
    assert [c for c in calls if c in STREAMING] == ([AS] if kernel else [])
    if kernel:
        assert torch.equal(ops._tall_matmul(gzd, wd), got), "not bit-reproducible"
    got = got.cpu()
    ratio = linear_ratio(got, gz, wt, zero, 1.0, None)
    sub = slice(0, min(rows, SELF_ROWS))
    ratio2 = linear_ratio(got[sub], gz[sub], wt, zero, 1.0, None, operand=two_term)
    print(f"RATIO dx[{rows}x{n}->{k},{kernel or 'library'}] kernel={ratio:.3f} two_term={ratio2:.2f}")
    assert ratio <= 1.0, f"error {ratio:.2f} x the bound"
    assert ratio2 > 1.0, f"the bound does not tell a two-term split from three terms ({ratio2:.2f})"


# ---- the composed backward functions ------------------------------------------------------------------------------------------------------
def _leaf(t, dt):
    return None if t is None else t.detach().to(DEV, dt).clone().requires_grad_(True)


def check_grads(label, fn_hip, fn_ref, tensors, names, mask_of, calls, want_calls):
    """out = fn(*leaves) on both sides (float32 through the HIP path, float64 through the plain formula on the device); loss =
    <out, g> with a fixed random g whose entries are zeroed by mask_of(float64 leaves) -> bool tensor broadcastable to out (entries
    whose activation input is within KINK of zero); every gradient within 2e-4 of its largest float64 entry + 2e-5.  The backward's
    library calls are exactly want_calls."""
    l64 = [_leaf(t, torch.float64) for t in tensors]
    out64 = fn_ref(*l64)
    g = torch.randn(out64.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
    with torch.no_grad():
        g = g * mask_of(*l64).to(g.dtype)
    live = [t for t in l64 if t is not None]
    want = torch.autograd.grad(out64, live, g.double())
    l32 = [_leaf(t, torch.float32) for t in tensors]
    out = fn_hip(*l32)
    assert out.requires_grad
    torch.testing.assert_close(out.detach().double(), out64.detach(), rtol=5e-5, atol=5e-5)
    del calls[:]
    got = torch.autograd.grad(out, [t for t in l32 if t is not None], g)
    assert list(calls) == want_calls, calls
    for name, a, b in zip([nm for nm, t in zip(names, tensors) if t is not None], got, want):
        scale = float(b.abs().max())
        err = float((a.double() - b).abs().max())
        print(f"GRAD {label} {name}: max err {err:.2e}, gradient scale {scale:.2e}, bound {2e-4 * scale + 2e-5:.2e}")
        assert torch.isfinite(a).all(), name
        assert err <= 2e-4 * scale + 2e-5, f"grad {name}: max err {err:.2e}, gradient scale {scale:.2e}"


def _mlp2_ref(x, res, w1, b1, w2, b2, slope):
    hid = x @ w1.T if b1 is None else x @ w1.T + b1
    out = torch.where(hid > 0, hid, hid * slope) @ w2.T + b2
    return out if res is None else out + res


def _mlp2_mask(x, res, w1, b1, w2, b2, slope):
    hid = x @ w1.T if b1 is None else x @ w1.T + b1
    return (hid.abs().amin(dim=-1, keepdim=True) >= KINK)      # a row with a hidden unit on the kink: no upstream gradient


def _mlp2_data(rows, cin, hidden, cout, res, b1):
    g = torch.Generator().manual_seed(rows + cin + hidden + cout)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    return [r(rows, cin), r(rows, cout) if res else None, r(hidden, cin, scale=cin ** -0.5), r(hidden, scale=0.1) if b1 else None,
            r(cout, hidden, scale=hidden ** -0.5), r(cout, scale=0.1), torch.tensor([0.25])]


MLP2_NAMES = ["x", "res", "w1", "b1", "w2", "b2", "slope"]
# the backward of _Mlp2Fn: the hidden activation again (forward kernel), g_act = gy W2 (forward kernel on W2^T where the kernel reads
# gy: cout a multiple of 4), act and (g_hid, dslope) in one pass each, dW2 / db2, dW1 / db1 (hidden = 512: two column blocks), dx
MLP2_CALLS = {
    (64, 256, 64): [PACK, AS, PACK, AS, PRELU, PRELU_GRAD, WGRAD, WGRAD, PACK, AS],
    (128, 512, 3): [PACK, AS, PRELU, PRELU_GRAD, WGRAD, WGRAD, WGRAD, PACK, AS],
}


@pytest.mark.parametrize("rows", [8200, 16390])
@pytest.mark.parametrize("cin,hidden,cout,res,b1", [(64, 256, 64, True, True), (128, 512, 3, False, True), (128, 512, 3, False, False)],
                         ids=["64-256-64+res", "128-512-3", "128-512-3,b1=None"])
def test_mlp2_backward_on_the_streaming_route_matches_float64(rows, cin, hidden, cout, res, b1, calls):
    be = ops.backend()
    data = _mlp2_data(rows, cin, hidden, cout, res, b1)
    label = f"mlp2[{rows}x{cin}-{hidden}-{cout}{',res' if res else ''}{'' if b1 else ',b1=None'}]"
    check_grads(label, lambda x, r, w1, b1_, w2, b2, sl: be.mlp2(x, w1, b1_, w2, b2, sl, res=r), _mlp2_ref, data, MLP2_NAMES, _mlp2_mask, calls,
                MLP2_CALLS[(cin, hidden, cout)])


def test_mlp2_backward_at_600_rows_reaches_no_streaming_kernel(calls):
    """What test_grad_gpu.test_mlp2_gradients covers: below 2048 rows every product of the backward is a library GEMM; only the
    one-pass PReLU kernels are the workload's."""
    be = ops.backend()
    data = _mlp2_data(600, 64, 256, 64, True, True)
    check_grads("mlp2[600x64-256-64,res]", lambda x, r, w1, b1_, w2, b2, sl: be.mlp2(x, w1, b1_, w2, b2, sl, res=r), _mlp2_ref, data, MLP2_NAMES, _mlp2_mask,
                calls, [PRELU, PRELU_GRAD])
    assert not {AS, WGRAD} & set(calls)


def _linear_ref(slope):
    def ref(x, res, w, b):
        z = x @ w.T + b
        y = torch.where(z > 0, z, z * slope) if slope != 1.0 else z
        return y if res is None else y + res
    return ref


def _linear_mask(slope):
    return lambda x, res, w, b: (x @ w.T + b).abs() >= (KINK if slope != 1.0 else -1.0)


# (rows, piece widths, the backward's calls): a single tensor always takes _LinearFn; pieces that want a gradient are concatenated and
# take it from 16384 rows (below, the layer is the library's, forward and backward: no streaming call at all)
LINEAR_CASES = [
    (8200, (64,), [PACK, AS, WGRAD]),
    (8200, (36, 36, 36), []),
    (16390, (36, 36, 36), [PACK, AS, WGRAD]),
]


@pytest.mark.parametrize("slope", [0.1, 0.0, 1.0])
@pytest.mark.parametrize("rows,ks,want", LINEAR_CASES, ids=[f"{r}x{'+'.join(map(str, ks))}" for r, ks, _ in LINEAR_CASES])
def test_linear_backward_on_the_streaming_route_matches_float64(rows, ks, want, slope, calls):
    be = ops.backend()
    n, K = 64, sum(ks)
    g = torch.Generator().manual_seed(rows + K)
    data = [torch.randn(rows, K, generator=g), torch.randn(rows, n, generator=g), torch.randn(n, K, generator=g) * K ** -0.5, torch.randn(n, generator=g) * 0.1]
    offs = [sum(ks[:i]) for i in range(len(ks))]

    def hip(x, res, w, b):
        xs = x if len(ks) == 1 else [x[:, o:o + kk].contiguous() for o, kk in zip(offs, ks)]   # the pieces: copies whose gradients autograd joins again
        return be.linear(xs, w, b, slope, res)
    check_grads(f"linear[{rows}x{'+'.join(map(str, ks))}->{n},slope={slope},res]", hip, _linear_ref(slope), data, ["x", "res", "w", "b"], _linear_mask(slope), calls, want)


# the 3 -> 32 lift: dx = gz W runs the forward kernel (K = 32 -> 3 outputs); the 32 -> 3 head: gz has 3 columns, the kernel cannot
# read it, dx is the library's
@pytest.mark.parametrize("k,n,slope,want", [(3, 32, 0.1, [PACK, AS, WGRAD]), (32, 3, 1.0, [WGRAD])], ids=["3->32,slope=0.1", "32->3,slope=1"])
def test_plain_linear_backward_matches_float64(k, n, slope, want, calls):
    rows = 8200
    g = torch.Generator().manual_seed(rows + k + n)
    data = [torch.randn(rows, k, generator=g), None, torch.randn(n, k, generator=g) * k ** -0.5, torch.randn(n, generator=g) * 0.1]
    check_grads(f"plain_linear[{rows}x{k}->{n},slope={slope}]", lambda x, res, w, b: ops.plain_linear(x, w, b, slope), _linear_ref(slope), data,
                ["x", "res", "w", "b"], _linear_mask(slope), calls, want)
