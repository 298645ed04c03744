"""EMD metric with the reference's names (models/EMD/emd.py:26-45, models/utils.py:223-235) on the HIP kernels, differentiable.

EarthMoverDistanceFunction is the reference's autograd function (emd.py:5-21) without the (B,M,N) match matrix: when a
gradient is wanted the forward (mcp_emd_keep) keeps each level's ratios, B*10*(N+M) floats, and the backward (mcp_emd_grad)
rebuilds the match pair by pair from them.  Without a gradient the forward is mcp_emd alone.  The match is held constant in
the backward, as the reference's matchcostgrad1 / matchcostgrad2 do.  approxmatch_forward / matchcost_forward /
matchcost_backward are the reference's explicit-match emd_cuda API (emd.cpp:24-26).

Per-cloud lengths (lengths1 / lengths2 of earth_mover_distance, approxmatch_forward and EMD): element b of a padded batch is the
metric of its prefixes xyz1[b, :lengths1[b]] and xyz2[b, :lengths2[b]] (mcp_emd_lengths / mcp_emd_keep_lengths /
mcp_emd_grad_lengths), bit for bit the length-free result on the sliced clouds; an element with an empty side costs 0.  The
padding is never read, the gradient rows beyond a length are exact zeros, and no length is read on the host."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _check(name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        what = f"{t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"EMD: {name} must be a float32 CUDA tensor, got {what}")


def _check_clouds(xyz1, xyz2):
    _check("xyz1", xyz1)
    _check("xyz2", xyz2)
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz1.shape[0] != xyz2.shape[0]:
        raise RuntimeError(f"EMD: expected xyz1 (B,N,3) and xyz2 (B,M,3), got {tuple(xyz1.shape)} and {tuple(xyz2.shape)}")


def _check_match(match, B, N, M):
    _check("match", match)
    if tuple(match.shape) != (B, M, N):
        raise RuntimeError(f"EMD: expected match of shape {(B, M, N)}, got {tuple(match.shape)}")


def _lengths(xyz1, xyz2, lengths1, lengths2):
    """lengths1 / lengths2 as (B,) int32 device arrays, or None (ops.lengths_tensor: host values are validated, device tensors
    are trusted and clamped in the kernels)."""
    from . import ops
    B, N, M = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    return ops.lengths_tensor(lengths1, B, N, xyz1.device), ops.lengths_tensor(lengths2, B, M, xyz1.device)


def _iptr(t):
    return None if t is None else _lib.iptr(t)


def _emd(xyz1, xyz2, want_match, keep_levels=False, len1=None, len2=None):
    """len1 / len2: (B,) int32 device arrays or None; both None is the length-free call."""
    xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
    B, N, _ = xyz1.shape
    M = xyz2.shape[1]
    plain = len1 is None and len2 is None
    cost = torch.empty((B,), dtype=torch.float32, device=xyz1.device)
    ws = torch.empty((B * (3 * N + 2 * M),), dtype=torch.float32, device=xyz1.device)
    match = torch.empty((B, M, N), dtype=torch.float32, device=xyz1.device) if want_match else None
    lib = _lib.load()
    levels = None
    with torch.cuda.device(xyz1.device):
        if keep_levels:
            levels = torch.empty((lib.mcp_emd_levels_floats(B, N, M),), dtype=torch.float32, device=xyz1.device)
        if not plain:
            if keep_levels:
                _lib.check(lib.mcp_emd_keep_lengths(B, N, M, _lib.fptr(xyz1), _lib.fptr(xyz2), _iptr(len1), _iptr(len2), _lib.fptr(cost),
                                                    _lib.fptr(levels), _lib.fptr(ws), _lib.stream()))
            else:
                _lib.check(lib.mcp_emd_lengths(B, N, M, _lib.fptr(xyz1), _lib.fptr(xyz2), _iptr(len1), _iptr(len2),
                                               _lib.fptr(match) if want_match else None, _lib.fptr(cost), _lib.fptr(ws), _lib.stream()))
        elif keep_levels:
            _lib.check(lib.mcp_emd_keep(B, N, M, _lib.fptr(xyz1), _lib.fptr(xyz2), _lib.fptr(cost), _lib.fptr(levels), _lib.fptr(ws),
                                        _lib.stream()))
        else:
            _lib.check(lib.mcp_emd(B, N, M, _lib.fptr(xyz1), _lib.fptr(xyz2), _lib.fptr(match) if want_match else None, _lib.fptr(cost),
                                   _lib.fptr(ws), _lib.stream()))
    return cost, match, levels


class EarthMoverDistanceFunction(torch.autograd.Function):
    """emd.py:5-21: xyz1 (B,N,3), xyz2 (B,M,3) -> cost (B); backward through the kept levels (no match matrix)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        _check_clouds(xyz1, xyz2)
        xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
        if any(ctx.needs_input_grad[:2]):
            cost, _, levels = _emd(xyz1, xyz2, False, keep_levels=True)
            ctx.save_for_backward(xyz1, xyz2, levels)
        else:
            cost = _emd(xyz1, xyz2, False)[0]
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_cost):
        xyz1, xyz2, levels = ctx.saved_tensors
        grad_cost = grad_cost.contiguous()
        B, N, M = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
        want1, want2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g1 = torch.empty((B, N, 3), dtype=torch.float32, device=xyz1.device) if want1 else None
        g2 = torch.empty((B, M, 3), dtype=torch.float32, device=xyz1.device) if want2 else None
        with torch.cuda.device(xyz1.device):
            _lib.check(_lib.load().mcp_emd_grad(B, N, M, _lib.fptr(grad_cost), _lib.fptr(xyz1), _lib.fptr(xyz2), _lib.fptr(levels),
                                                _lib.fptr(g1) if want1 else None, _lib.fptr(g2) if want2 else None, _lib.stream()))
        return g1, g2


class EarthMoverDistanceLengthsFunction(torch.autograd.Function):
    """EarthMoverDistanceFunction over the valid prefixes of a padded batch: len1 / len2 (B,) int32 device arrays or None.
    Gradient rows beyond a length, and every row of an element with an empty side, are exact zeros."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, len1, len2):
        _check_clouds(xyz1, xyz2)
        xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
        if any(ctx.needs_input_grad[:2]):
            cost, _, levels = _emd(xyz1, xyz2, False, keep_levels=True, len1=len1, len2=len2)
            ctx.has_lens = (len1 is not None, len2 is not None)
            ctx.save_for_backward(xyz1, xyz2, levels, *[t for t in (len1, len2) if t is not None])
        else:
            cost = _emd(xyz1, xyz2, False, len1=len1, len2=len2)[0]
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_cost):
        xyz1, xyz2, levels, *lens = ctx.saved_tensors   # the lengths are saved tensors: an in-place change before backward is an error
        len1 = lens.pop(0) if ctx.has_lens[0] else None
        len2 = lens.pop(0) if ctx.has_lens[1] else None
        grad_cost = grad_cost.contiguous()
        B, N, M = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
        want1, want2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g1 = torch.empty((B, N, 3), dtype=torch.float32, device=xyz1.device) if want1 else None
        g2 = torch.empty((B, M, 3), dtype=torch.float32, device=xyz1.device) if want2 else None
        with torch.cuda.device(xyz1.device):
            _lib.check(_lib.load().mcp_emd_grad_lengths(B, N, M, _lib.fptr(grad_cost), _lib.fptr(xyz1), _lib.fptr(xyz2), _iptr(len1),
                                                        _iptr(len2), _lib.fptr(levels), _lib.fptr(g1) if want1 else None,
                                                        _lib.fptr(g2) if want2 else None, _lib.stream()))
        return g1, g2, None, None


def approxmatch_forward(xyz1, xyz2, lengths1=None, lengths2=None):
    """emd_cuda.approxmatch_forward: (B,N,3),(B,M,3) -> match (B,M,N).  With lengths, block [:lengths2[b], :lengths1[b]] of
    match[b] is the match of the two prefixes and everything else is zero."""
    _check_clouds(xyz1, xyz2)
    len1, len2 = _lengths(xyz1, xyz2, lengths1, lengths2)
    return _emd(xyz1, xyz2, True, len1=len1, len2=len2)[1]


def matchcost_forward(xyz1, xyz2, match):
    """emd_cuda.matchcost_forward: (B,N,3),(B,M,3), match (B,M,N) -> cost (B) = sum match * squared distance."""
    _check_clouds(xyz1, xyz2)
    B, N, M = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    _check_match(match, B, N, M)
    xyz1, xyz2, match = xyz1.contiguous(), xyz2.contiguous(), match.contiguous()
    cost = torch.empty((B,), dtype=torch.float32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        _lib.check(_lib.load().mcp_matchcost(B, N, M, _lib.fptr(xyz1), _lib.fptr(xyz2), _lib.fptr(match), _lib.fptr(cost), _lib.stream()))
    return cost


def matchcost_backward(grad_cost, xyz1, xyz2, match):
    """emd_cuda.matchcost_backward: grad_cost (B), (B,N,3),(B,M,3), match (B,M,N) -> [grad1 (B,N,3), grad2 (B,M,3)]."""
    _check_clouds(xyz1, xyz2)
    _check("grad_cost", grad_cost)
    B, N, M = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    _check_match(match, B, N, M)
    if grad_cost.numel() != B:
        raise RuntimeError(f"EMD: expected grad_cost of {B} elements, got {tuple(grad_cost.shape)}")
    grad_cost, xyz1, xyz2, match = grad_cost.contiguous(), xyz1.contiguous(), xyz2.contiguous(), match.contiguous()
    g1 = torch.empty((B, N, 3), dtype=torch.float32, device=xyz1.device)
    g2 = torch.empty((B, M, 3), dtype=torch.float32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        _lib.check(_lib.load().mcp_matchcost_grad(B, N, M, _lib.fptr(grad_cost), _lib.fptr(xyz1), _lib.fptr(xyz2), _lib.fptr(match),
                                                  _lib.fptr(g1), _lib.fptr(g2), _lib.stream()))
    return [g1, g2]


def earth_mover_distance(xyz1, xyz2, transpose=True, lengths1=None, lengths2=None):
    """models/EMD/emd.py:26-45: (b,3,n) inputs when transpose=True, (b,n,3) otherwise -> cost (b).
    lengths1 / lengths2: per-cloud point counts of a padded batch (a sequence, a CPU tensor or a device tensor; None = every point
    of that side): cost[b] is the EMD of the first lengths1[b] points of xyz1[b] and the first lengths2[b] points of xyz2[b]."""
    if xyz1.dim() == 2:
        xyz1 = xyz1.unsqueeze(0)
    if xyz2.dim() == 2:
        xyz2 = xyz2.unsqueeze(0)
    if transpose:
        xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
    if lengths1 is not None or lengths2 is not None:
        _check_clouds(xyz1, xyz2)
        len1, len2 = _lengths(xyz1, xyz2, lengths1, lengths2)
        if torch.is_grad_enabled() and (xyz1.requires_grad or xyz2.requires_grad):
            return EarthMoverDistanceLengthsFunction.apply(xyz1, xyz2, len1, len2)
        return _emd(xyz1, xyz2, False, len1=len1, len2=len2)[0]
    if torch.is_grad_enabled() and (xyz1.requires_grad or xyz2.requires_grad):
        return EarthMoverDistanceFunction.apply(xyz1, xyz2)
    # no graph to record (the function's forward cannot see the grad mode): mcp_emd alone, no level buffer
    _check_clouds(xyz1, xyz2)
    return _emd(xyz1, xyz2, False)[0]


def EMD(pc1, pc2, lengths1=None, lengths2=None):
    """models/utils.py:223-235: pc1, pc2 (B,3,M) -> mean(cost) / M.  With lengths: mean_b(cost_b / max(lengths1_b, 1)), the
    same per-point normalisation on each element's own point count."""
    x, y = pc1.permute(0, 2, 1).contiguous(), pc2.permute(0, 2, 1).contiguous()
    if lengths1 is None and lengths2 is None:
        return torch.mean(earth_mover_distance(x, y, transpose=False)) / pc1.shape[2]
    _check_clouds(x, y)
    len1, len2 = _lengths(x, y, lengths1, lengths2)
    d = earth_mover_distance(x, y, transpose=False, lengths1=len1, lengths2=len2)
    count = pc1.shape[2] if len1 is None else len1.clamp(1, pc1.shape[2]).to(d.dtype)
    return torch.mean(d / count)
