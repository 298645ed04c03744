"""Operator API of the reference's pointnet2/pointnet2_utils.py (and its duplicate
models/pointnet2/pointnet2_utils.py) on top of the MI355X kernels: same public
names, argument order, dtypes (int32 indices), shapes and autograd contract
(index-producing ops return None grads; gather/group/interpolate backward is a
scatter-add).  Reference lines are cited per class."""
from typing import Tuple

import torch
import torch.nn as nn
from torch.autograd import Function

from . import pointnet2_cuda as pointnet2


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _i32(shape, like):
    return torch.empty(shape, dtype=torch.int32, device=like.device)


class FurthestPointSampling(Function):
    """pointnet2_utils.py:10-33."""

    @staticmethod
    def forward(ctx, xyz: torch.Tensor, npoint: int) -> torch.Tensor:
        assert xyz.is_contiguous()
        B, N, _ = xyz.size()
        output = _i32((B, npoint), xyz)
        temp = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
        pointnet2.furthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output)
        ctx.mark_non_differentiable(output)
        return output

    @staticmethod
    def backward(ctx, a=None):
        return None, None


furthest_point_sample = FurthestPointSampling.apply


class GatherOperation(Function):
    """pointnet2_utils.py:39-70."""

    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        assert features.is_contiguous()
        assert idx.is_contiguous()
        B, npoint = idx.size()
        _, C, N = features.size()
        output = _f32((B, C, npoint), features)
        pointnet2.gather_points_wrapper(B, C, N, npoint, features, idx, output)
        ctx.for_backwards = (idx, C, N)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        idx, C, N = ctx.for_backwards
        B, npoint = idx.size()
        grad_features = torch.empty((B, C, N), dtype=torch.float32, device=grad_out.device)
        pointnet2.gather_points_grad_wrapper(B, C, N, npoint, grad_out.contiguous(), idx, grad_features, accumulate=False)
        return grad_features, None


gather_operation = GatherOperation.apply


class ThreeNN(Function):
    """pointnet2_utils.py:76-102: returns (sqrt(dist2), idx)."""

    @staticmethod
    def forward(ctx, unknown: torch.Tensor, known: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        assert unknown.is_contiguous()
        assert known.is_contiguous()
        B, N, _ = unknown.size()
        m = known.size(1)
        dist2 = _f32((B, N, 3), unknown)
        idx = _i32((B, N, 3), unknown)
        pointnet2.three_nn_wrapper(B, N, m, unknown, known, dist2, idx)
        ctx.mark_non_differentiable(idx)
        return torch.sqrt(dist2), idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


def three_nn(unknown: torch.Tensor, known: torch.Tensor, unknown_lengths=None, known_lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ThreeNN.apply(unknown, known); with per-cloud lengths (forms: ops.lengths_tensor) on a padded batch: element b searches
    known[b, :known_lengths[b]] for unknown[b, :unknown_lengths[b]] and a live row holds what three_nn returns for the two prefixes
    on their own -- with fewer than three known points the positions k >= known_lengths[b] hold distance +inf and index 0, as the
    reference's untouched accumulators do.  Padded unknown rows hold distance 0 and index 0; rows beyond a length are never read.
    The search is the package's K = 3 neighbour search in its direct distance form under the lengths (HipBackend.knn: exhaustive or
    pruned by the padded sizes, the same bits), whose own rule for short clouds -- repeat the last entry -- is overwritten here."""
    if unknown_lengths is None and known_lengths is None:
        return ThreeNN.apply(unknown, known)
    from . import ops
    assert unknown.is_contiguous() and known.is_contiguous()
    B, N, _ = unknown.size()
    m = known.size(1)
    ul, kl = ops.lengths_tensor(unknown_lengths, B, N, unknown.device), ops.lengths_tensor(known_lengths, B, m, unknown.device)
    idx, dist2 = ops.backend().knn(unknown, known, 3, mode=ops.MCP_DIST_DIRECT, return_dist=True, query_lengths=ul, ref_lengths=kl)
    if kl is not None:
        tail = torch.arange(3, device=unknown.device).view(1, 1, 3) >= kl.clamp(0, m).view(B, 1, 1)
        if ul is not None:
            tail = tail & (torch.arange(N, device=unknown.device).view(1, N, 1) < ul.clamp(0, N).view(B, 1, 1))
        dist2, idx = dist2.masked_fill(tail, float("inf")), idx.masked_fill(tail, 0)
    return torch.sqrt(dist2), idx


class ThreeInterpolate(Function):
    """pointnet2_utils.py:108-150."""

    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
        assert features.is_contiguous()
        assert idx.is_contiguous()
        assert weight.is_contiguous()
        B, c, m = features.size()
        n = idx.size(1)
        ctx.three_interpolate_for_backward = (idx, weight, m)
        output = _f32((B, c, n), features)
        pointnet2.three_interpolate_wrapper(B, c, m, n, features, idx, weight, output)
        return output

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        idx, weight, m = ctx.three_interpolate_for_backward
        B, c, n = grad_out.size()
        grad_features = torch.empty((B, c, m), dtype=torch.float32, device=grad_out.device)
        pointnet2.three_interpolate_grad_wrapper(B, c, n, m, grad_out.contiguous(), idx, weight, grad_features, accumulate=False)
        return grad_features, None, None


three_interpolate = ThreeInterpolate.apply


class GroupingOperation(Function):
    """pointnet2_utils.py:156-194."""

    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        assert features.is_contiguous()
        assert idx.is_contiguous()
        B, nfeatures, nsample = idx.size()
        _, C, N = features.size()
        output = _f32((B, C, nfeatures, nsample), features)
        pointnet2.group_points_wrapper(B, C, N, nfeatures, nsample, features, idx, output)
        ctx.for_backwards = (idx, N)
        return output

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        idx, N = ctx.for_backwards
        B, C, npoint, nsample = grad_out.size()
        grad_features = torch.empty((B, C, N), dtype=torch.float32, device=grad_out.device)
        pointnet2.group_points_grad_wrapper(B, C, N, npoint, nsample, grad_out.contiguous(), idx, grad_features, accumulate=False)
        return grad_features, None


grouping_operation = GroupingOperation.apply


class BallQuery(Function):
    """pointnet2_utils.py:200-225."""

    @staticmethod
    def forward(ctx, radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor) -> torch.Tensor:
        assert new_xyz.is_contiguous()
        assert xyz.is_contiguous()
        B, N, _ = xyz.size()
        npoint = new_xyz.size(1)
        idx = torch.zeros((B, npoint, nsample), dtype=torch.int32, device=xyz.device)
        pointnet2.ball_query_wrapper(B, N, npoint, radius, nsample, new_xyz, xyz, idx)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None


class BallQueryLengths(Function):
    """BallQuery on a padded batch of clouds of different sizes (HipBackend.ball_query): idx (B,npoint,nsample) int32, every slot
    written by the kernel."""

    @staticmethod
    def forward(ctx, radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor, xyz_lengths, new_xyz_lengths) -> torch.Tensor:
        assert new_xyz.is_contiguous()
        assert xyz.is_contiguous()
        from . import ops
        idx = ops.backend().ball_query(xyz, new_xyz, radius, nsample, xyz_lengths=xyz_lengths, new_xyz_lengths=new_xyz_lengths)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None, None, None


def ball_query(radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor, xyz_lengths=None, new_xyz_lengths=None) -> torch.Tensor:
    """BallQuery.apply(radius, nsample, xyz, new_xyz) -- the reference's call, route and launch.  With per-cloud lengths (forms:
    ops.lengths_tensor): element b is xyz[b, :xyz_lengths[b]] with the centres new_xyz[b, :new_xyz_lengths[b]]; a live centre gets
    the reference's row for the two prefixes, a padded centre zeros, and rows at or beyond a length are never read."""
    if xyz_lengths is None and new_xyz_lengths is None:
        return BallQuery.apply(radius, nsample, xyz, new_xyz)
    return BallQueryLengths.apply(radius, nsample, xyz, new_xyz, xyz_lengths, new_xyz_lengths)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class QueryAndGroup(nn.Module):
    """Ball query + grouping of coordinates (relative to the centre) and features: the module of pointnet2/pointnet2_utils.py:231-264.
    xyz (B,N,3), new_xyz (B,npoint,3), features (B,C,N) or None -> (B, 3+C | C | 3, npoint, nsample).
    Inference takes ONE launch (mcp_query_and_group: the hits of a centre never leave the compute unit, no transposed copy of the
    cloud, no concatenation); when a gradient is wanted the result is composed from the differentiable functions above."""

    def __init__(self, radius: float, nsample: int, use_xyz: bool = True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz: torch.Tensor, new_xyz: torch.Tensor, features: torch.Tensor = None, xyz_lengths=None, new_xyz_lengths=None):
        """xyz_lengths / new_xyz_lengths (forms: ops.lengths_tensor): element b is xyz[b, :xyz_lengths[b]] (and the same columns of
        features) with the centres new_xyz[b, :new_xyz_lengths[b]].  A live centre gets the module's output for the two prefixes (no
        hit: point 0, which is live); a padded centre, and every centre of an element without a point, gets zeros in every channel.
        Rows and feature columns at or beyond a length are never read, and get no gradient."""
        if features is None and not self.use_xyz:
            raise AssertionError("QueryAndGroup without features needs use_xyz=True: there would be nothing to group")
        with_xyz = self.use_xyz or features is None
        with_lengths = xyz_lengths is not None or new_xyz_lengths is not None
        B, N, _ = xyz.shape
        M = new_xyz.shape[1]
        if with_lengths:
            from . import ops
            rl, ql = ops.lengths_tensor(xyz_lengths, B, N, xyz.device), ops.lengths_tensor(new_xyz_lengths, B, M, xyz.device)
        if self.nsample <= 64 and not _wants_grad(xyz, new_xyz, features):
            from . import _lib
            xyz, new_xyz = xyz.detach().contiguous(), new_xyz.detach().contiguous()
            feats = None if features is None else features.detach().contiguous()
            C = 0 if feats is None else feats.shape[1]
            out = torch.empty((B, (3 if with_xyz else 0) + C, M, self.nsample), dtype=torch.float32, device=xyz.device)
            head = (B, N, M, C, float(self.radius), int(self.nsample), int(bool(self.use_xyz)), _lib.fptr(xyz), _lib.fptr(new_xyz),
                    None if feats is None else _lib.fptr(feats))
            stream = torch.cuda.current_stream(xyz.device).cuda_stream
            with torch.cuda.device(xyz.device):
                if with_lengths:
                    _lib.check(_lib.load().mcp_query_and_group_lengths(*head, None if rl is None else _lib.iptr(rl),
                                                                       None if ql is None else _lib.iptr(ql), _lib.fptr(out), stream))
                else:
                    _lib.check(_lib.load().mcp_query_and_group(*head, _lib.fptr(out), stream))
            return out
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz, rl, ql) if with_lengths else ball_query(self.radius, self.nsample, xyz, new_xyz)
        parts = []
        if with_xyz:  # neighbour coordinates relative to their centre, channel-major as grouping_operation returns them
            parts.append(grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1))
        if features is not None:
            parts.append(grouping_operation(features, idx))
        out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        if with_lengths:  # padded centres, and elements without a point (whose index 0 is padding): exact zeros, whatever was gathered
            live = torch.ones((B, M), dtype=torch.bool, device=xyz.device)
            if ql is not None:
                live = live & (torch.arange(M, device=xyz.device).view(1, M) < ql.clamp(0, M).view(B, 1))
            if rl is not None:
                live = live & (rl > 0).view(B, 1)
            out = torch.where(live.view(B, 1, M, 1), out, out.new_zeros(()))
        return out


class GroupAll(nn.Module):
    """The whole cloud as one group (pointnet2/pointnet2_utils.py:267-290): (B, 3+C | C | 3, 1, N); new_xyz is ignored."""

    def __init__(self, use_xyz: bool = True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz: torch.Tensor, new_xyz: torch.Tensor, features: torch.Tensor = None):
        parts = [xyz.transpose(1, 2).unsqueeze(2)] if (self.use_xyz or features is None) else []
        if features is not None:
            parts.append(features.unsqueeze(2))
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
