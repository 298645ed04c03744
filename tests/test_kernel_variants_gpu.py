"""-m gpu: every template instantiation of the dense-layer kernels (csrc/linear.hip, mlp.hip, attention.hip) against a float64
reference of the same operation, at the shapes where such kernels go wrong: ragged row tails, output widths inside a tile, pieces
whose width is not a multiple of 32, partial key tiles, dead query lanes, unequal key-stage counts per wave, large logits.
tests/kernel_variants.py names the variant each case reaches; test_kernel_variants_cpu.py checks that the cases reach them all.

Tolerances follow the arithmetic.  An element of a K-long product computed in fp32 (the bf16 three-way split of mfma_split.h
drops only terms below 2^-20 of each product) is within

    c * 2^-24 * sqrt(K) * (|W| @ |x| + |b|)   (+ c * 2^-24 * |res| for the rounded residual add)

of the exact value, with one constant c per family.  The linear and mlp2 tests also show that the bound is tight enough to matter:
the same product with both operands cut to the first TWO split terms (a kernel that lost the third, mfma_split.h) fails it on the
same data.  That needs a product whose terms do not cancel on average -- truncation errors all point towards zero, so they add up
where the products share a sign -- hence inputs and weights with a positive mean (and a negative bias, so that the activation
sees both signs)."""
import math

import pytest
import torch

from mocopci_amd import ops
from tests import kernel_variants as kv
from tests.dense_reference import BLOCK, C_LINEAR, SELF_ROWS, U, act, linear_ratio, positive_mean_data, two_term  # shared with the backward products

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_MLP2 = 2.0     # mlp2_kernel (both layers)
C_ATTN = 8.0     # attention_small / wide / wide_ksplit


# ---- linear_kernel / linear_splitk_kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kv.cases("linear"), ids=kv.case_id)
def test_linear_variant_matches_float64(case):
    rows, ks, n, slope = case["rows"], case["ks"], case["n"], case["slope"]
    K = sum(ks)
    g = torch.Generator().manual_seed(rows * 7 + K * 3 + n)
    x, w, b = positive_mean_data(g, rows, K, n)
    res = torch.randn(rows, n, generator=g) if case["res"] else None
    be = ops.backend()
    xd, k0 = x.to(DEV), ks[0]
    if case["strided"]:   # the first piece is a column slice of a wider tensor (row stride k0 + 12)
        wide = torch.zeros(rows, k0 + 12, device=DEV)
        wide[:, 4:4 + k0] = xd[:, :k0]
        first = wide[:, 4:4 + k0]
    else:
        first = xd[:, :k0].contiguous()
    offs = [sum(ks[:i]) for i in range(len(ks))]
    pieces = [first] + [xd[:, o:o + k].contiguous() for o, k in zip(offs[1:], ks[1:])]
    del xd
    arg = pieces if len(pieces) > 1 else pieces[0]
    wd, bd = w.to(DEV), b.to(DEV)
    rd = None if res is None else res.to(DEV)
    call = lambda: be.linear(arg, wd, bd, slope, rd, policy_rows=case["policy_rows"])
    got = call()
    assert torch.equal(call(), got), "not bit-reproducible"
    got = got.cpu()
    ratio = linear_ratio(got, x, w, b, slope, res)
    sub = slice(0, min(rows, SELF_ROWS))
    ratio2 = linear_ratio(got[sub], x[sub], w, b, slope, None if res is None else res[sub], operand=two_term)
    print(f"RATIO {kv.case_id(case)} kernel={ratio:.3f} two_term={ratio2:.2f}")
    assert ratio <= 1.0, f"{kv.expected_kernel(**case)}: error {ratio:.2f} x the bound"
    assert ratio2 > 1.0, f"the bound does not tell a two-term split from the kernel's three terms ({ratio2:.2f})"


def test_linear_declines_output_widths_it_is_not_built_for():
    # 129..160 and 193..224 columns (5 and 7 tiles) and wide outputs that are not whole 128-column blocks
    be = ops.backend()
    for n in (130, 200, 300):
        with pytest.raises(ValueError):
            kv.expected_kernel("linear", rows=20000, ks=(64,), n=n)
        with pytest.raises(RuntimeError):
            be.linear_pack(torch.zeros(n, 64, device=DEV), None, [64])


# ---- linear_narrow_kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kv.cases("linear_narrow"), ids=kv.case_id)
def test_linear_narrow_variant_matches_float64(case):
    rows, k, n = case["rows"], case["k"], case["n"]
    g = torch.Generator().manual_seed(rows + k + n)
    x = torch.randn(rows, k, generator=g)
    w, b = torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g) * 0.1
    be = ops.backend()
    wide = torch.zeros(rows, k + 8, device=DEV)
    wide[:, 4:4 + k] = x.to(DEV)
    call = lambda: be.linear_narrow(wide[:, 4:4 + k], w.to(DEV), b.to(DEV), 0.25)
    got = call()
    assert torch.equal(call(), got)
    # act on the input, then the K-long fp32 sum (plain FMAs): the same bound with x -> act(x)
    ratio = linear_ratio(got.cpu(), act(x, 0.25), w, b, 1.0, None)
    print(f"RATIO {kv.case_id(case)} kernel={ratio:.3f}")
    assert ratio <= 1.0, f"error {ratio:.2f} x the bound"


# ---- mlp2_kernel ---------------------------------------------------------------------------------------------------------------
def mlp2_ratio(got, x, w1, b1, w2, b2, slope, res, operand=None):
    """As linear_ratio for both layers (operand=two_term: x, W1, the fp32 hidden activation and W2 cut to two split terms)."""
    cin, hidden = w1.shape[1], w1.shape[0]
    cut = (lambda t: t) if operand is None else operand
    w1o, w2o = cut(w1).double(), cut(w2).double()
    w1a, w2a = w1.double().abs(), w2.double().abs()
    worst = 0.0
    for r0 in range(0, x.shape[0], BLOCK):
        xb = x[r0:r0 + BLOCK]
        h = act(cut(xb).double() @ w1o.T + b1.double(), slope)
        y = (h if operand is None else operand(h.float()).double()) @ w2o.T + b2.double()
        # hidden error (first layer, passed through the activation: |act'| <= 1) carried through |W2|, plus the second layer's own
        e_h = math.sqrt(cin) * (xb.double().abs() @ w1a.T + b1.double().abs())
        bound = math.sqrt(hidden) * (h.abs() @ w2a.T + b2.double().abs()) + e_h @ w2a.T
        if res is not None:
            y = y + res[r0:r0 + BLOCK].double()
            bound = bound + res[r0:r0 + BLOCK].double().abs()
        worst = max(worst, ((got[r0:r0 + BLOCK].double() - y).abs() / (C_MLP2 * U * bound)).max().item())
    return worst


@pytest.mark.parametrize("case", kv.cases("mlp2"), ids=kv.case_id)
def test_mlp2_variant_matches_float64(case):
    rows, cin, hidden, cout = case["rows"], case["cin"], case["hidden"], case["cout"]
    g = torch.Generator().manual_seed(rows + cin * 5 + hidden * 3 + cout)
    x, w1, b1 = positive_mean_data(g, rows, cin, hidden)
    w2 = (torch.randn(cout, hidden, generator=g) + 1.0) / hidden
    b2 = torch.randn(cout, generator=g) * 0.1
    res = torch.randn(rows, cout, generator=g) if case["res"] else None
    slope = 0.25
    be = ops.backend()
    if case["strided"]:   # x read through a row stride (a column slice of a wider tensor)
        wide = torch.zeros(rows, cin + 8, device=DEV)
        wide[:, :cin] = x.to(DEV)
        xd = wide[:, :cin]
    else:
        xd = x.to(DEV)
    dw = [t.to(DEV) for t in (w1, b1, w2, b2)]
    rd = None if res is None else res.to(DEV)
    call = lambda: be.mlp2(xd, *dw, slope, res=rd)
    got = call()
    assert torch.equal(call(), got), "not bit-reproducible"
    got = got.cpu()
    ratio = mlp2_ratio(got, x, w1, b1, w2, b2, slope, res)
    sub = slice(0, min(rows, SELF_ROWS))
    ratio2 = mlp2_ratio(got[sub], x[sub], w1, b1, w2, b2, slope, None if res is None else res[sub], operand=two_term)
    print(f"RATIO {kv.case_id(case)} kernel={ratio:.3f} two_term={ratio2:.2f}")
    assert ratio <= 1.0, f"{kv.expected_kernel(**case)}: error {ratio:.2f} x the bound"
    assert ratio2 > 1.0, f"the bound does not tell a two-term split from the kernel's three terms ({ratio2:.2f})"


# ---- attention_small / attention_wide / attention_wide_ksplit -----------------------------------------------------------------
def attention_ratio(got, q, k, v, heads, shift, scale):
    """Against softmax(q k^T scale) v in float64, batch b reading keys / values of batch (b + shift) mod BF.  Bound per element:
    c 2^-24 (sqrt(nk) + S) (P @ |V|), S = max over keys of (|q| @ |k|) scale -- the score error relative to the largest
    logit's magnitude (the exponent's argument) plus the nk-long P.V sum."""
    BF, nq, C = q.shape
    nk, hd = k.shape[1], C // heads
    sp = lambda t, n: t.double().reshape(BF, n, heads, hd).permute(0, 2, 1, 3)
    qh = sp(q, nq)
    kh, vh = sp(torch.roll(k, -shift, 0), nk), sp(torch.roll(v, -shift, 0), nk)
    s = qh @ kh.transpose(-1, -2) * scale
    p = torch.softmax(s, dim=-1)
    want = p @ vh
    S = (qh.abs() @ kh.abs().transpose(-1, -2)).amax(-1, keepdim=True) * scale
    bound = C_ATTN * U * (math.sqrt(nk) + S) * (p @ vh.abs())
    gh = got.double().reshape(BF, nq, heads, hd).permute(0, 2, 1, 3)
    return ((gh - want).abs() / bound).max().item()


@pytest.mark.parametrize("case", kv.cases("attention"), ids=kv.case_id)
def test_attention_variant_matches_float64(case):
    bf, nq, nk, heads, hd, shift = case["bf"], case["nq"], case["nk"], case["heads"], case["hd"], case["shift"]
    C = heads * hd
    g = torch.Generator().manual_seed(bf * 1000 + nq * 7 + nk * 3 + hd + heads)
    q, k, v = torch.randn(bf, nq, C, generator=g), torch.randn(bf, nk, C, generator=g), torch.randn(bf, nk, C, generator=g)
    scale = hd ** -0.5
    if case["same_keys"]:      # every key of head 0 identical: a uniform softmax, the output is the mean of v
        k[:, :, :hd] = k[:, :1, :hd]
    if case["logits"]:         # max |q.k| * scale about `logits`: exp without max subtraction overflows
        kr = torch.roll(k, -(shift or 0), 0)
        qk = torch.einsum("bihd,bjhd->bhij", q.double().reshape(bf, nq, heads, hd), kr.double().reshape(bf, nk, heads, hd))
        q = q * float(case["logits"] / (qk.abs().max().item() * scale))
    be = ops.backend()
    kvd = torch.cat([k, v], dim=-1).to(DEV)   # [k | v] per row, as the kv projection writes it
    qd = q.to(DEV)
    if shift is None:
        call = lambda: be.attention(qd, kvd, heads)
    else:
        call = lambda: be.attention_rot(qd, kvd[..., :C], kvd[..., C:], heads, shift)
    got = call()
    assert torch.equal(call(), got), "not bit-reproducible"
    got = got.cpu()
    assert torch.isfinite(got).all()
    ratio = attention_ratio(got, q, k, v, heads, shift or 0, scale)
    print(f"RATIO {kv.case_id(case)} kernel={ratio:.3f}")
    assert ratio <= 1.0, f"{kv.expected_kernel(**case)}: error {ratio:.2f} x the bound"


# ---- policy_rows: a subset of a tall product's rows, computed as the tall product -------------------------------------------
@pytest.mark.parametrize("R,sub,k,n", [(196608, 6000, 536, 64), (20000, 3000, 128, 96)])
def test_policy_rows_subset_is_bit_identical_to_the_full_product(R, sub, k, n):
    """model.lin / qkv_projection (model.py) compute some rows of a tall product on their own with policy_rows = the full row count
    and rely on the same bits as those rows of the full product: 196608 rows run 8-wave workgroups, 6000 rows 4-wave ones; 20000
    rows run the tall kernel, 3000 rows alone would run split-K."""
    g = torch.Generator().manual_seed(R + sub)
    x, w, b = positive_mean_data(g, R, k, n)
    sel = torch.randperm(R, generator=g)[:sub].sort().values.to(DEV)
    be = ops.backend()
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    full = be.linear(xd, wd, bd, 0.1)
    part = be.linear(xd[sel], wd, bd, 0.1, policy_rows=R)
    assert torch.equal(part, full[sel])


# ---- pieces that want a gradient, with a kept pack ------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [(36, 36), (64, 64, 64)])
def test_linear_pieces_with_gradient_and_kept_pack(ks):
    """be.linear(pieces, ..., packed=linear_pack(w, b, widths)) where the pieces require a gradient: the pieces are concatenated for
    the explicit backward, so the kernel must run on the image of the concatenation -- [36, 36] pads to 4 chunks, [72] has 3.
    Forward and input gradients against float64 autograd."""
    rows, n, slope = 16384 + 100, 64, 0.1
    K = sum(ks)
    g = torch.Generator().manual_seed(K)
    x, w, b = positive_mean_data(g, rows, K, n)
    gy = torch.randn(rows, n, generator=g)
    x64 = x.double().requires_grad_()
    z64 = x64 @ w.double().T + b.double()
    gy[z64.detach().abs() < 1e-5] = 0.0   # the activation's derivative is not defined at fp32 precision there
    y64 = act(z64, slope)
    y64.backward(gy.double())
    be = ops.backend()
    wd, bd = w.to(DEV), b.to(DEV)
    offs = [sum(ks[:i]) for i in range(len(ks))]
    pieces = [x[:, o:o + kk].contiguous().to(DEV).requires_grad_() for o, kk in zip(offs, ks)]
    out = be.linear(pieces, wd, bd, slope, packed=be.linear_pack(wd, bd, list(ks)))
    out.backward(gy.to(DEV))
    ratio = linear_ratio(out.detach().cpu(), x, w, b, slope, None)
    assert ratio <= 1.0, f"forward: error {ratio:.2f} x the bound"
    # dx = gz W: an n-long product (the forward kernel on W^T) of the masked upstream gradient
    gz = torch.where(z64.detach() > 0, gy.double(), gy.double() * slope)
    dx = torch.cat([p.grad.cpu() for p in pieces], dim=1).double()
    bound = C_LINEAR * U * math.sqrt(n) * (gz.abs() @ w.double().abs())
    gratio = ((dx - x64.grad).abs() / bound).max().item()
    assert gratio <= 1.0, f"input gradient: error {gratio:.2f} x the bound"
