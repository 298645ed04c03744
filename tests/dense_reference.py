"""What the float64 tests of the dense layers share (test_kernel_variants_gpu.py: the forward kernels; test_linear_grad_edges_gpu.py:
the same kernels as backward products): the data, the error bound of an fp32-accurate K-long product and the two-term self-check.

An element of a K-long product computed in fp32 (the bf16 three-way split of mfma_split.h drops only terms below 2^-20 of each
product) is within

    c * 2^-24 * sqrt(K) * (|W| @ |x| + |b|)   (+ c * 2^-24 * |res| for the rounded residual add)

of the exact value, with one constant c per family.  The same product with both operands cut to the first TWO split terms (a kernel
that lost the third) fails that bound where the products do not cancel on average -- truncation errors all point towards zero, so
they add up where the products share a sign -- hence inputs and weights with a positive mean (and a negative bias, so that an
activation sees both signs).  A plain module, imported by the tests."""
import math

import torch

U = 2.0 ** -24
C_LINEAR = 2.0   # linear_kernel, linear_splitk_kernel, linear_narrow_kernel
BLOCK = 32768    # rows per float64 block of the CPU references
SELF_ROWS = 8192  # rows of the two-term self-check


def _trunc16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def two_term(t):
    """fp32 values cut to the first two bf16 pieces of mfma_split.h's exact split (x1 = top 16 bits, x2 = top 16 bits of the rest):
    what a kernel that dropped the third piece would multiply."""
    t = t.float()
    a1 = _trunc16(t)
    return a1 + _trunc16(t - a1)


def act(z, slope):
    return torch.where(z > 0, z, z * slope)


def positive_mean_data(g, rows, k, n):
    """x ~ N(0.5, 1), W ~ (N(0, 1) + 1) / K, b ~ N(-0.5, 0.1): the output straddles zero, products mostly share a sign."""
    x = torch.randn(rows, k, generator=g) + 0.5
    w = (torch.randn(n, k, generator=g) + 1.0) / k
    b = torch.randn(n, generator=g) * 0.1 - 0.5
    return x, w, b


def linear_ratio(got, x, w, b, slope, res, c=C_LINEAR, operand=lambda t: t):
    """max over elements of |got - exact| / bound, with exact = act(W x + b) + res in float64 (operands through `operand` first:
    two_term for the self-check), computed in row blocks."""
    K = x.shape[1]
    w64, b64 = operand(w).double(), b.double()
    wa, ba = w.double().abs(), b.double().abs()
    worst = 0.0
    for r0 in range(0, x.shape[0], BLOCK):
        xb = x[r0:r0 + BLOCK]
        z = operand(xb).double() @ w64.T + b64
        y = act(z, slope)
        bound = math.sqrt(K) * (xb.double().abs() @ wa.T + ba)
        if res is not None:
            y = y + res[r0:r0 + BLOCK].double()
            bound = bound + res[r0:r0 + BLOCK].double().abs()
        worst = max(worst, ((got[r0:r0 + BLOCK].double() - y).abs() / (c * U * bound)).max().item())
    return worst
