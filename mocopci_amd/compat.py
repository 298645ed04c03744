"""Drop-in installation for an unmodified checkout of the reference.

The reference reaches its extension through two import roots, both ending in `import pointnet2_cuda`
(pointnet2/pointnet2_utils.py:7; models/pointnet2/pointnet2_utils.py:7 via mocopci.py:8), its EMD metric through
`import emd_cuda` (models/EMD/emd.py:2), and
models/layers.py:15 expects a `models.common` module that the repository does not ship.
`install()` registers this package's implementations under those names BEFORE the reference's
modules are imported:

    import mocopci_amd.compat as compat; compat.install()
    from models.m_models.mocopci import MoCoPCI      # the reference's own file, unmodified

`install(patch_helpers=True)` additionally rebinds the module-level helpers the reference defines in
Python (knn_point, knn_point_cosine, index_points_group, index_points_gather in pointconv_util and the
local copies in mocopci.py:1130-1215) to the fused kernels, keeping their signatures and int64 results.
"""
import sys
import types

import torch

from . import emd_cuda, ops, pointnet2_cuda, pointnet2_utils


def _common_module():
    """`models.common` as implied by the call sites in models/layers.py:35,37,62,64,162,170."""
    m = types.ModuleType("models.common")
    m.fps = pointnet2_utils.furthest_point_sample                     # fps(xyz (B,N,3), npoint) -> (B,npoint) int32
    m.gather_points = pointnet2_utils.gather_operation                # gather_points(features (B,C,N), idx) -> (B,C,npoint)
    m.ball_query = pointnet2_utils.ball_query                         # ball_query(radius, nsample, xyz, new_xyz)
    m.three_nn = pointnet2_utils.three_nn
    m.three_interpolate = pointnet2_utils.three_interpolate
    m.group_points = pointnet2_utils.grouping_operation
    return m


# ---- reference-signature helpers on the fused kernels (channel-last in, like the reference's) ----
def knn_point(nsample, xyz, new_xyz):
    """mocopci.py:1158-1169: xyz (B,N,3) refs, new_xyz (B,S,3) queries -> (B,S,nsample) int64."""
    return ops.backend().knn(new_xyz.contiguous(), xyz.contiguous(), nsample).long()


def knn_point_cosine(nsample, xyz, new_xyz, lengths=None, new_lengths=None):
    """pointconv_util.py:142-153 on (B,N,C) features.  lengths (B,) belongs to xyz, the references, and new_lengths (B,) to
    new_xyz, the queries (forms: ops.lengths_tensor): rows beyond them are padding, see ops.HipBackend.knn_cosine."""
    return ops.backend().knn_cosine(new_xyz.contiguous(), xyz.contiguous(), nsample, query_lengths=new_lengths, ref_lengths=lengths).long()


def index_points_group(points, knn_idx):
    """mocopci.py:1204-1215: (B,N,C), (B,S,K) -> (B,S,K,C)."""
    return ops.backend().group_rows(points.contiguous(), knn_idx.int())


def index_points_gather(points, fps_idx):
    """mocopci.py:1190-1201: (B,N,C), (B,S) -> (B,S,C)."""
    return ops.backend().group_rows(points.contiguous(), fps_idx.int())


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, return_nn=False, **_):
    """pytorch3d.ops.knn_points as called at pointconv_util.py:910 and models/layers.py:205,287: returns (dists, idx, nn).
    lengths1 / lengths2 (B,): only p1[b, :lengths1[b]] are queries and only p2[b, :lengths2[b]] are searched.  As in pytorch3d,
    rows >= lengths1[b] and positions k >= lengths2[b] are zero in dists and idx (the library's own rule for fewer than K
    references, "repeat the last valid entry", is overwritten here).  return_nn: nn = p2 gathered through idx, (B,P1,K,3);
    otherwise None.  Every other keyword of pytorch3d's signature is accepted and ignored."""
    be = ops.backend()
    p1, p2 = p1.contiguous(), p2.contiguous()
    if lengths1 is None and lengths2 is None:
        idx, dist = be.knn(p1, p2, K, mode=ops.MCP_DIST_DIRECT, return_dist=True)
    else:
        B, P2 = p2.shape[0], p2.shape[1]
        l1, l2 = ops.lengths_tensor(lengths1, B, p1.shape[1], p1.device), ops.lengths_tensor(lengths2, B, P2, p1.device)
        idx, dist = be.knn(p1, p2, K, mode=ops.MCP_DIST_DIRECT, return_dist=True, query_lengths=l1, ref_lengths=l2)
        if l2 is not None:
            pad = torch.arange(K, device=p1.device).view(1, 1, K) >= l2.clamp(0, P2).view(B, 1, 1)
            idx, dist = idx.masked_fill(pad, 0), dist.masked_fill(pad, 0.0)
    nn = be.group_rows(p2, idx) if return_nn else None
    return dist, idx.long(), nn


def ball_query(p1, p2, lengths1=None, lengths2=None, K=500, radius=0.2, return_nn=True):
    """pytorch3d.ops.ball_query: for every point of p1 (B,P1,3) the first K points of p2 (B,P2,3), in index order, closer than
    `radius` -> (dists, idx, nn).  lengths1 / lengths2 (B,): only p1[b, :lengths1[b]] are centres and only p2[b, :lengths2[b]] are
    searched.  idx (B,P1,K) int64 holds -1 behind a centre's hits and in rows >= lengths1[b] (pytorch3d's padding; the library's
    own, "repeat the first hit", is overwritten from the hit counts); dists (B,P1,K) are the SQUARED distances and nn (B,P1,K,3) the
    gathered points (None without return_nn), both zero where idx is -1."""
    be = ops.backend()
    p1, p2 = p1.contiguous(), p2.contiguous()
    idx, cnt = be.ball_query(p2, p1, radius, K, xyz_lengths=lengths2, new_xyz_lengths=lengths1, return_count=True)
    pad = torch.arange(K, device=p1.device).view(1, 1, K) >= cnt.unsqueeze(-1)
    nn = be.group_rows(p2.detach(), idx.masked_fill(pad, 0)).masked_fill(pad.unsqueeze(-1), 0.0)
    diff = (nn - p1.detach().unsqueeze(2)).masked_fill(pad.unsqueeze(-1), 0.0)
    dists = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
    return dists, idx.long().masked_fill(pad, -1), nn if return_nn else None


def chamfer_distance(x, y, x_lengths=None, y_lengths=None):
    """pytorch3d.loss.chamfer_distance as called at models/utils.py:44 (default reductions, no normals): (loss, None)."""
    if x_lengths is None and y_lengths is None:
        return ops.backend().chamfer(x.contiguous(), y.contiguous()), None
    return ops.backend().chamfer(x.contiguous(), y.contiguous(), x_lengths=x_lengths, y_lengths=y_lengths), None


def sample_farthest_points(points, lengths=None, K=50, random_start_point=False):
    """pytorch3d.ops.sample_farthest_points: points (B,P,3), lengths (B,) -> (sampled (B,K,3), idx (B,K) int64).  Element b samples
    min(lengths[b], K) points of points[b, :lengths[b]], starting from row 0; as pytorch3d pads, positions j >= lengths[b] hold index
    -1 and coordinates 0.  One launch of the length-aware sampler (HipBackend.fps(lengths=)); rows beyond a length are never read.
    Among points at equal distance the tie rule is this library's -- the reference sampling kernel's (csrc/fps.hip) -- not
    pytorch3d's first-index rule, so on clouds with exact ties the selections can differ from pytorch3d's.  K is one integer;
    random_start_point=True is not supported (the sampler is deterministic) and raises."""
    if random_start_point:
        raise NotImplementedError("sample_farthest_points: random_start_point=True is not supported; the start point is row 0")
    points = points.contiguous()
    B, P = points.shape[0], points.shape[1]
    if lengths is None:
        idx, sampled = ops.backend().fps(points, K, with_points=True)
        lens = None
    else:
        lens = ops.lengths_tensor(lengths, B, P, points.device)
        idx, sampled = ops.backend().fps(points, K, with_points=True, lengths=lens)
    pad = torch.arange(K, device=points.device).view(1, K) >= (P if lens is None else lens.clamp(0, P).view(B, 1))
    return sampled.masked_fill(pad.unsqueeze(-1), 0.0), idx.long().masked_fill(pad, -1)


def install(patch_helpers=False):
    sys.modules["pointnet2_cuda"] = pointnet2_cuda
    sys.modules["emd_cuda"] = emd_cuda                                # models/EMD/emd.py:2
    for name in ("pointnet2.pointnet2_utils", "models.pointnet2.pointnet2_utils"):
        sys.modules[name] = pointnet2_utils
    for pkg in ("pointnet2", "models.pointnet2"):
        if pkg in sys.modules:
            setattr(sys.modules[pkg], "pointnet2_utils", pointnet2_utils)
    sys.modules.setdefault("models.common", _common_module())
    if patch_helpers:
        for modname in ("models.pointconv_util", "models.m_models.mocopci"):
            mod = sys.modules.get(modname)
            if mod is None:
                continue
            for fn in (knn_point, knn_point_cosine, index_points_group, index_points_gather):
                if hasattr(mod, fn.__name__):
                    setattr(mod, fn.__name__, fn)
            if hasattr(mod, "knn_points"):
                mod.knn_points = knn_points
            if hasattr(mod, "sample_farthest_points"):
                mod.sample_farthest_points = sample_farthest_points
