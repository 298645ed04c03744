"""Float64 reference of attention over a padded batch with per-element lengths (helper of test_attention_lengths_cpu.py and
test_attention_lengths_gpu.py; runs on whatever device its inputs live on).

The masked dense formulation: with ql, kl the lengths of an element (clamped to the padded sizes),
    rows i <  ql   softmax_{j < kl}(q_i . k_j scale) (* keep) v_j,  lse = log2-sum-exp of that row's scores;
    rows i >= ql   zeros (out and lse);      kl = 0   every row zero.
Padding is replaced by zeros before any product, so whatever it holds (NaN, inf) reaches neither a result nor a gradient."""
import math

import torch

U = 2.0 ** -24    # unit roundoff of fp32
C_ATTN = 8.0      # the project's constant for the attention kernels (tests/test_kernel_variants_gpu.py)
M32 = 0xFFFFFFFF
LN2 = 0.6931471805599453


def keep_mask(seed, bf, heads, nq, nk, p, device):
    """The kernels' dropout mask in torch (restated from tests/test_attention_wide_grad_gpu.py): a hash of (seed, row = (bf * heads +
    head) * nq + query, key) over the PADDED shape -> (bf, heads, nq, nk) bool."""
    row = torch.arange(bf * heads * nq, device=device, dtype=torch.int64).view(bf, heads, nq, 1)
    key = torch.arange(nk, device=device, dtype=torch.int64).view(1, 1, 1, nk)
    x = (seed ^ ((row * 0x9E3779B1) & M32) ^ ((key * 0x85EBCA77) & M32)) & M32
    x = x ^ (x >> 16); x = (x * 0x7FEB352D) & M32; x = x ^ (x >> 15); x = (x * 0x846CA68B) & M32; x = x ^ (x >> 16)
    return x >= int(p * 4294967296.0)


def spans(lens, bf, limit, device):
    """(bf,) int64 lengths as the kernels see them: None = full, clamped to [0, limit]."""
    if lens is None:
        return torch.full((bf,), limit, dtype=torch.int64, device=device)
    return torch.as_tensor(lens, device=device).to(torch.int64).reshape(bf).clamp(0, limit)


def _heads(q, k, v, heads, qlen, klen, kv_shift):
    bf, nq, C = q.shape
    nk, hd = k.shape[1], C // heads
    dev = q.device
    ql, kl = spans(qlen, bf, nq, dev), spans(klen, bf, nk, dev)
    # keys / values of element (b + kv_shift) mod bf, with THAT element's length
    k, v, kl = torch.roll(k, -kv_shift, 0), torch.roll(v, -kv_shift, 0), torch.roll(kl, -kv_shift, 0)
    qm = torch.arange(nq, device=dev).view(1, nq) < ql.view(bf, 1)
    km = torch.arange(nk, device=dev).view(1, nk) < kl.view(bf, 1)
    zero = q.new_zeros(())
    sp = lambda t, n, m: torch.where(m.unsqueeze(-1), t, zero).reshape(bf, n, heads, hd).permute(0, 2, 1, 3)
    return sp(q, nq, qm), sp(k, nk, km), sp(v, nk, km), qm.view(bf, 1, nq, 1), km.view(bf, 1, 1, nk), kl


def masked_attention(q, k, v, heads, qlen=None, klen=None, scale=None, keep=None, kv_shift=0):
    """(out (bf,nq,C), lse (bf,heads,nq) in the log2 domain) in the dtype of the inputs, differentiable.  q (bf,nq,C), k / v (bf,nk,C);
    keep: (bf,heads,nq,nk) factor on P in P.V (a dropout mask already scaled by 1 / (1 - p)), or None."""
    bf, nq, C = q.shape
    hd = C // heads
    scale = hd ** -0.5 if scale is None else scale
    qh, kh, vh, qm, km, kl = _heads(q, k, v, heads, qlen, klen, kv_shift)
    some = (kl > 0).view(bf, 1, 1, 1)
    s = qh @ kh.transpose(-1, -2) * scale
    s = s.masked_fill(~km & some, float("-inf"))     # an element without keys keeps finite scores; its P is dropped below
    p = torch.where(km, torch.softmax(s, dim=-1), s.new_zeros(()))
    lse = torch.where(qm.squeeze(-1) & some.squeeze(-1), torch.logsumexp(s, dim=-1) / LN2, s.new_zeros(()))
    if keep is not None:
        p = p * keep
    out = torch.where(qm, p @ vh, s.new_zeros(()))
    return out.permute(0, 2, 1, 3).reshape(bf, nq, C), lse


def split_kv(kv):
    C = kv.shape[-1] // 2
    return kv[..., :C], kv[..., C:]


def reference(q, kv, heads, qlen, klen, grad_out=None, scale=None, keep=None):
    """float64 (out, lse, grad_q, grad_kv) of the layer's calling convention: q (bf,nq,C), kv (bf,nk,2C) = [k | v]; the gradients are
    None without grad_out.  Padding of grad_out is ignored (the output's padded rows do not depend on anything)."""
    ql, kvl = (t.detach().double().clone().requires_grad_(True) for t in (q, kv))
    out, lse = masked_attention(ql, *split_kv(kvl), heads, qlen, klen, scale, keep)
    if grad_out is None:
        return out.detach(), lse.detach(), None, None
    bf, nq, _ = q.shape
    live = torch.arange(nq, device=q.device).view(1, nq, 1) < spans(qlen, bf, nq, q.device).view(bf, 1, 1)
    g = torch.where(live, grad_out.double(), grad_out.new_zeros((), dtype=torch.float64))
    gq, gkv = torch.autograd.grad(out, (ql, kvl), g)
    return out.detach(), lse.detach(), gq, gkv


def forward_ratio(got, q, k, v, heads, qlen=None, klen=None, scale=None, kv_shift=0):
    """max over live rows of |got - f64| / bound, the bound of tests/test_kernel_variants_gpu.py::attention_ratio with each element's
    own kl in place of nk:  C_ATTN 2^-24 (sqrt(kl) + S) (P @ |V|),  S = max over the live keys of (|q| @ |k|) scale.  Elements without
    a live row or a live key do not enter (their rows are checked for exact zeros elsewhere)."""
    bf, nq, C = q.shape
    hd = C // heads
    scale = hd ** -0.5 if scale is None else scale
    qd, kd, vd = q.double(), k.double(), v.double()
    want, _ = masked_attention(qd, kd, vd, heads, qlen, klen, scale, None, kv_shift)
    qh, kh, vh, qm, km, kl = _heads(qd, kd, vd, heads, qlen, klen, kv_shift)
    s = (qh @ kh.transpose(-1, -2) * scale).masked_fill(~km, float("-inf"))
    p = torch.where(km, torch.softmax(s, dim=-1), s.new_zeros(()))
    S = (qh.abs() @ kh.abs().transpose(-1, -2)).masked_fill(~km, 0.0).amax(-1, keepdim=True) * scale
    bound = C_ATTN * U * (kl.double().sqrt().view(bf, 1, 1, 1) + S) * (p @ vh.abs())
    gh = got.double().reshape(bf, nq, heads, hd).permute(0, 2, 1, 3)
    wh = want.reshape(bf, nq, heads, hd).permute(0, 2, 1, 3)
    live = (qm & (kl > 0).view(bf, 1, 1, 1)).expand_as(gh)
    if not bool(live.any()):
        return 0.0
    ratio = (gh - wh).abs() / bound
    return float(ratio[live].max())


def grad_bound(want):
    """The project's bound on a gradient tensor: 1e-4 max|f64| + 1e-6 (tests/test_grad_gpu.py, tests/test_attention_wide_grad_gpu.py)."""
    return 1e-4 * float(want.abs().max()) + 1e-6


assert math.isclose(LN2, math.log(2.0))
