"""-m "not gpu": PointConv with centre lengths, what can be held without a device.

  * The new unit emits exactly the length forms of the dense units' kernels -- one per form of the dense dispatch, so every case of
    test_pointconv_lengths_gpu.py has a kernel and no kernel is without a case --, and the dense units still emit what
    test_kernel_variants_cpu.py pins (the length forms live in pointconv_lengths.hip alone).
  * The three entry points are declared in the header with `const int *qlen` behind idx and carry the dense signature plus one
    pointer in _lib.SIGNATURES.
  * grad.pointconv_agg_lengths_twin, the masked torch formulation that shapes without a backward kernel take: on a padded batch
    with NaN padding and out-of-range list rows it gives, per element, what grad.pointconv_agg_twin gives on the live prefix alone
    (float32 sums of 32 terms in another association: 1e-5 relative to the largest magnitude), zeros on padded rows, finite
    gradients that are zero on padded centres and equal the per-element gradients.
  * grad.spread_padded_rows keeps live rows and gives padded centre i the row i mod n."""
import os
import re

import torch

from mocopci_amd import _lib, grad
from tests.test_kernel_variants_cpu import emitted_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_unit_emits_the_length_forms_and_nothing_else():
    dense = emitted_kernels(("pointconv",))
    assert emitted_kernels(("pointconv_lengths",)) == {k[:-1] + ", PcLengths>" for k in dense} | {"pointconv_agg_grad_lengths_kernel",
                                                                                                "pointconv_grad_reduce_kernel"}
    assert emitted_kernels(("pointconv_grad",)) == {"pointconv_agg_grad_kernel", "pointconv_grad_reduce_kernel"}
    assert not any("PcLengths" in k for k in dense)


def test_entry_points_are_declared_with_qlen_behind_idx():
    header = open(os.path.join(ROOT, "include", "mocopci_hip.h")).read()
    for name in ("mcp_pointconv_agg", "mcp_pointconv_linear", "mcp_pointconv_agg_grad"):
        plain = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        lens = re.search(rf"\bint {name}_lengths\((.*?)\);", header, re.S).group(1)
        norm = lambda s: re.sub(r"\s+", " ", s).strip()
        assert norm(lens) == norm(plain).replace("const int *idx,", "const int *idx, const int *qlen,")
        sig, sig_len = _lib.SIGNATURES[name], _lib.SIGNATURES[name + "_lengths"]
        assert len(sig_len) == len(sig) + 1 and sig_len[:9] == sig[:9] and sig_len[10:] == sig[9:]


def _gather(points, idx):
    return points[torch.arange(points.shape[0]).view(-1, 1, 1), idx.long()]


def test_masked_twin_is_the_dense_twin_on_the_live_prefix():
    g = torch.Generator().manual_seed(3)
    r = lambda *shape, scale=1.0: (torch.rand(*shape, generator=g) * 2 - 1) * scale
    B, N, S, D = 3, 40, 21, 5
    lens = torch.tensor([0, 21, 9])
    s_xyz, s_points, new_xyz = r(B, N, 3), r(B, N, D), r(B, S, 3)
    idx = torch.randint(0, N, (B, S, 32), generator=g, dtype=torch.int32)
    wn = [r(8, 3, scale=0.8), r(8, scale=0.3), r(8, 8, scale=0.6), r(8, scale=0.3), r(8, 8, scale=0.6), r(8, scale=0.3)]
    gout = r(B, S, (D + 3) * 8)
    live = torch.arange(S).view(1, S) < lens.view(B, 1)
    dirty_xyz, dirty_idx, dirty_g = new_xyz.clone(), idx.clone(), gout.clone()
    dirty_xyz[~live], dirty_g[~live], dirty_idx[~live] = float("nan"), float("nan"), 1 << 30

    leaves = [t.clone().requires_grad_(True) for t in (s_xyz, dirty_xyz, s_points, *wn)]
    out = grad.pointconv_agg_lengths_twin(_gather, leaves[0], leaves[1], leaves[2], dirty_idx, *leaves[3:], lens)
    assert (out[~live] == 0).all()
    grads = torch.autograd.grad(out, leaves, torch.where(live.unsqueeze(-1), dirty_g, torch.zeros(())))
    assert all(torch.isfinite(t).all() for t in grads)
    assert (grads[1][~live] == 0).all()

    want = [torch.zeros_like(t) for t in leaves]
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        one = [s_xyz[b:b + 1], new_xyz[b:b + 1, :n], s_points[b:b + 1]] + list(wn)
        one = [t.clone().requires_grad_(True) for t in one]
        o = grad.pointconv_agg_twin(_gather, one[0], one[1], one[2], idx[b:b + 1, :n], *one[3:])
        tol = 1e-5 * float(o.detach().abs().max())
        assert (out[b, :n] - o[0]).abs().max() <= tol
        gs = torch.autograd.grad(o, one, gout[b:b + 1, :n])
        want[0][b], want[2][b] = gs[0][0], gs[2][0]
        want[1][b, :n] = gs[1][0]
        for w, gw in zip(want[3:], gs[3:]):
            w += gw
    for got, w in zip(grads, want):
        assert (got - w).abs().max() <= 1e-5 * max(1.0, float(w.abs().max()))


def test_padded_rows_are_spread_over_the_sources():
    idx = torch.randint(0, 7, (2, 20, 4), dtype=torch.int32)
    live = torch.arange(20).view(1, 20) < torch.tensor([[3], [20]])
    out = grad.spread_padded_rows(idx, live, 7)
    assert torch.equal(out[live], idx[live]) and out.dtype == idx.dtype
    assert torch.equal(out[0, 3:], (torch.arange(3, 20, dtype=torch.int32) % 7).view(-1, 1).expand(-1, 4))
