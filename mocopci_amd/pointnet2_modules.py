"""Set-abstraction and feature-propagation modules of pointnet2 (the reference's pointnet2/pointnet2_modules.py:
PointnetSAModuleMSG, PointnetSAModule, PointnetFPModule) on the MI355X kernels.  Same constructor arguments, tensor layouts (xyz
(B,N,3), features (B,C,N) -> new_xyz (B,npoint,3), (B, sum of the scales' last widths, npoint)) and parameter names, so a state_dict
of the reference classes loads strictly (tests/golden/pointnet2_sa_state_keys.json lists the names of one two-scale module,
pointnet2_fp_state_keys.json those of a feature-propagation module).

Two routes give the same layer:
  * the composition -- QueryAndGroup, the shared Conv2d / BatchNorm2d / ReLU stack, the pool over the neighbours -- is the definition
    and carries the gradient;
  * the fused route -- sampling, one ball query per scale, one mcp_group_mlp launch per scale (ops.HipBackend.group_mlp) -- writes
    nothing but the pooled features.  It is taken only under no-grad, in eval(), for a shape the kernel supports, and for a shape
    class that the measurement of tools/group_mlp_times.py found faster (ops.GROUP_MLP_FUSED_CLASSES; `route` overrides it).
    When a gradient is wanted a scale's fused route is the differentiable layer ops.HipBackend.group_mlp_layer (mcp_group_mlp
    forward, mcp_group_mlp_grad backward: the ball query on detached coordinates, gradients for xyz, new_xyz, the features and the
    stack's parameters through ops.fold_conv_bn_grad), taken in eval() or without BatchNorm for a class of
    ops.GROUP_MLP_GRAD_FUSED_CLASSES (tools/group_mlp_grad_times.py; `grad_route` overrides it).
    Under train() with BatchNorm a scale has a third route: the layer with batch statistics, ops.HipBackend.group_mlp_bn_layer
    (mcp_group_mlp_bn_forward / mcp_group_mlp_bn_backward), after which the module updates every BatchNorm2d's running statistics as
    torch does -- taken with or without a wanted gradient, never with lengths or with npoint=None, for a class of
    ops.GROUP_MLP_BN_FUSED_CLASSES (tools/group_mlp_bn_times.py; `bn_route` overrides it).
PointnetFPModule has the same two routes: the composition -- three_nn, the weights in torch, three_interpolate, cat, the shared
stack -- and one mcp_fp_mlp launch after the three-neighbour search (ops.HipBackend.fp_mlp; ops.FP_MLP_FUSED_CLASSES from
tools/fp_mlp_times.py).  When a gradient is wanted its fused route is the differentiable layer ops.HipBackend.fp_mlp_layer
(mcp_fp_mlp_grad backward), taken in eval() or without BatchNorm for a class of ops.FP_MLP_GRAD_FUSED_CLASSES
(tools/fp_mlp_grad_times.py; `grad_route` overrides it).  Under train() with BatchNorm it has a third route of its own: the layer
with batch statistics, ops.HipBackend.fp_mlp_bn_layer (mcp_fp_mlp_bn_forward / mcp_fp_mlp_bn_backward), after which the module
updates every BatchNorm2d's running statistics as torch does -- taken with or without a wanted gradient, never with lengths, for a
class of ops.FP_MLP_BN_FUSED_CLASSES (tools/fp_mlp_bn_times.py; `bn_route` overrides it)."""
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, pointnet2_utils as pu


def _conv_unit(cin, cout, bn, instance_norm):
    """One layer of the shared MLP under the reference's names: conv, bn.bn, activation, in."""
    unit = nn.Sequential()
    conv = nn.Conv2d(cin, cout, kernel_size=(1, 1), bias=not bn)
    nn.init.kaiming_normal_(conv.weight)
    if conv.bias is not None:
        nn.init.zeros_(conv.bias)
    unit.add_module("conv", conv)
    if bn:
        norm = nn.Sequential()
        norm.add_module("bn", nn.BatchNorm2d(cout))
        unit.add_module("bn", norm)
    unit.add_module("activation", nn.ReLU(inplace=True))
    if instance_norm and not bn:
        unit.add_module("in", nn.InstanceNorm2d(cout, affine=False, track_running_stats=False))
    return unit


def _track(bn, mean, var, rows):
    """nn.BatchNorm2d's update of its running statistics from the batch mean and the biased batch variance over `rows` rows."""
    if not bn.track_running_stats or bn.running_mean is None:
        return
    with torch.no_grad():
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked += 1
        f = bn.momentum if bn.momentum is not None else 1.0 / bn.num_batches_tracked.to(torch.float32)
        bn.running_mean.mul_(1.0 - f).add_(f * mean)
        bn.running_var.mul_(1.0 - f).add_(f * (var * (rows / (rows - 1.0))))


def _shared_mlp(spec, bn, instance_norm):
    mlp = nn.Sequential()
    for j in range(len(spec) - 1):
        mlp.add_module(f"layer{j}", _conv_unit(spec[j], spec[j + 1], bn, instance_norm))
    return mlp


class PointnetSAModuleMSG(nn.Module):
    """Set abstraction with multi-scale grouping: npoint centres by furthest point sampling, per scale a ball of radii[i] with
    nsamples[i] slots, the shared MLP mlps[i] (its first entry counts the feature channels; 3 is added with use_xyz) and the pool.
    npoint=None groups the whole cloud (GroupAll).  route: "measured" (default), "always" or "never" for the fused route when no
    gradient is wanted; grad_route: the same three values, independently, for the fused differentiable route (mcp_group_mlp forward,
    mcp_group_mlp_grad backward) when one is -- eligible in eval() or with bn=False.  bn_route: the same three values,
    independently, for the route with batch statistics (mcp_group_mlp_bn_forward / mcp_group_mlp_bn_backward) under train() with
    bn=True, with or without a wanted gradient; a call with lengths keeps the composition there (its batch statistics count the
    padded rows, the kernel's do not), and so does npoint=None."""

    def __init__(self, *, npoint: int, radii: List[float], nsamples: List[int], mlps: List[List[int]], bn: bool = True, use_xyz: bool = True,
                 pool_method="max_pool", instance_norm=False):
        super().__init__()
        if not (len(radii) == len(nsamples) == len(mlps)):
            raise ValueError("radii, nsamples and mlps need one entry per scale")
        if pool_method not in ("max_pool", "avg_pool"):
            raise NotImplementedError(pool_method)
        self.npoint, self.use_xyz, self.pool_method, self.bn, self.instance_norm = npoint, use_xyz, pool_method, bn, instance_norm
        self.route = "measured"
        self.grad_route = "measured"
        self.bn_route = "measured"
        self.groupers, self.mlps = nn.ModuleList(), nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(pu.QueryAndGroup(radius, nsample, use_xyz=use_xyz) if npoint is not None else pu.GroupAll(use_xyz))
            spec = [spec[0] + (3 if use_xyz else 0), *spec[1:]]
            self.mlps.append(_shared_mlp(spec, bn, instance_norm))
        self.__dict__["_packed"] = {}

    # ---- fused route -----------------------------------------------------------------------------------------------------------
    def _layers(self, i):
        units = list(self.mlps[i].children())
        return [u.conv for u in units], [u.bn.bn if self.bn else None for u in units]

    def _packed_weights(self, i):
        """(packed, widths) of scale i, kept until one of its parameters or buffers is written or replaced."""
        state = [*self.mlps[i].parameters(), *self.mlps[i].buffers()]
        key = tuple((id(t), t._version, t.device) for t in state)
        hit = self.__dict__["_packed"].get(i)
        if hit is None or hit[0] != key:
            hit = self.__dict__["_packed"][i] = (key, ops.group_mlp_pack(*self._layers(i), use_xyz=self.use_xyz))
        return hit[1]

    def fused_scale(self, i, channels, centres):
        """Whether scale i of a call with `channels` feature channels and `centres` = B * npoint centres takes the fused route."""
        if self.training or self.npoint is None or self.route == "never" or (self.instance_norm and not self.bn):
            return False
        g = self.groupers[i]
        widths = [u.conv.out_channels for u in self.mlps[i].children()]
        if not ops.group_mlp_supported(channels, widths, g.nsample, self.use_xyz):
            return False
        return self.route == "always" or ops.group_mlp_routes_fused(channels, widths, g.nsample, centres)

    def fused_scale_grad(self, i, channels, centres):
        """Whether scale i of a call that wants a gradient takes the fused differentiable route: BatchNorm folded (eval mode) or
        absent."""
        if (self.training and self.bn) or self.npoint is None or self.grad_route == "never" or (self.instance_norm and not self.bn):
            return False
        g = self.groupers[i]
        widths = [u.conv.out_channels for u in self.mlps[i].children()]
        if not ops.group_mlp_grad_supported(channels, widths, g.nsample, self.use_xyz):
            return False
        return self.grad_route == "always" or ops.group_mlp_grad_routes_fused(channels, widths, g.nsample, centres)

    def fused_scale_bn(self, i, channels, centres, with_lengths=False):
        """Whether scale i of a call under train() with BatchNorm takes the fused route with batch statistics (a batch of one pair is
        left to torch, which refuses it)."""
        if not (self.training and self.bn) or self.npoint is None or with_lengths or self.bn_route == "never":
            return False
        g = self.groupers[i]
        widths = [u.conv.out_channels for u in self.mlps[i].children()]
        if centres * g.nsample < 2 or not ops.group_mlp_bn_supported(channels, widths, g.nsample, self.use_xyz):
            return False
        return self.bn_route == "always" or ops.group_mlp_bn_routes_fused(channels, widths, g.nsample, centres)

    def forward(self, xyz: torch.Tensor, features: torch.Tensor = None, new_xyz=None, xyz_lengths=None, new_xyz_lengths=None):
        """xyz (B,N,3), features (B,C,N) or None, new_xyz (B,npoint,3) or None (sampled here) -> new_xyz, (B, sum C_out, npoint).
        xyz_lengths / new_xyz_lengths (forms: ops.lengths_tensor): element b is its first xyz_lengths[b] points with the centres
        new_xyz[b, :new_xyz_lengths[b]]; padded centres, and every centre of an element without a point, give zeros."""
        be = ops.backend()
        B, N, _ = xyz.shape
        if new_xyz is None and self.npoint is not None:
            picked = be.fps(xyz.contiguous(), self.npoint, lengths=xyz_lengths)
            new_xyz = pu.gather_operation(xyz.transpose(1, 2).contiguous(), picked).transpose(1, 2).contiguous()
        wants_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (xyz, features, new_xyz, *self.parameters()))
        M = 1 if self.npoint is None else new_xyz.shape[1]
        C = 0 if features is None else features.shape[1]
        with_lengths = self.npoint is not None and (xyz_lengths is not None or new_xyz_lengths is not None)
        rl = ql = live = None
        if with_lengths:
            rl, ql = ops.lengths_tensor(xyz_lengths, B, N, xyz.device), ops.lengths_tensor(new_xyz_lengths, B, M, xyz.device)
            count = torch.full((B,), M, dtype=torch.int32, device=xyz.device) if ql is None else ql.clamp(0, M)
            if rl is not None:
                count = torch.where(rl > 0, count, torch.zeros_like(count))
            live = torch.arange(M, device=xyz.device).view(1, M) < count.view(B, 1)
        rows = None  # features channel-last, made once for the fused scales
        rows_grad = None  # the same, attached to the graph, for the differentiable fused scales
        outs = []
        for i, grouper in enumerate(self.groupers):
            if self.fused_scale_bn(i, C, B * M, with_lengths):
                if features is not None and rows_grad is None:
                    rows_grad = features.transpose(1, 2).contiguous()
                # the neighbour list is a constant of the layer: no gradient reaches the search
                idx = be.ball_query(xyz.detach().contiguous(), new_xyz.detach().contiguous(), grouper.radius, grouper.nsample)
                convs, bns = self._layers(i)
                layers = [(c.weight.flatten(1), c.bias, b.weight, b.bias, b.eps) for c, b in zip(convs, bns)]
                pooled, stats, _ = be.group_mlp_bn_layer(xyz.contiguous(), new_xyz.contiguous(), rows_grad, idx, layers, pool=self.pool_method,
                                                         use_xyz=self.use_xyz)
                for b, (mean, var) in zip(bns, stats):
                    _track(b, mean, var, B * M * grouper.nsample)
                outs.append(pooled.transpose(1, 2))
                continue
            if not wants_grad and self.fused_scale(i, C, B * M):
                packed, widths = self._packed_weights(i)
                x, c = xyz.detach().contiguous(), new_xyz.detach().contiguous()
                if features is not None and rows is None:
                    rows = features.detach().transpose(1, 2).contiguous()
                idx = be.ball_query(x, c, grouper.radius, grouper.nsample, xyz_lengths=rl, new_xyz_lengths=ql)
                pooled = be.group_mlp(x, c, rows, idx, packed, widths, pool=self.pool_method, use_xyz=self.use_xyz,
                                      new_xyz_lengths=count if with_lengths else None)
                outs.append(pooled.transpose(1, 2))
                continue
            if wants_grad and self.fused_scale_grad(i, C, B * M):
                if features is not None and rows_grad is None:
                    rows_grad = features.transpose(1, 2).contiguous()
                # the neighbour list is a constant of the layer: no gradient reaches the search
                idx = be.ball_query(xyz.detach().contiguous(), new_xyz.detach().contiguous(), grouper.radius, grouper.nsample, xyz_lengths=rl,
                                    new_xyz_lengths=ql)
                folded = [ops.fold_conv_bn_grad(c, b) for c, b in zip(*self._layers(i))]
                pooled = be.group_mlp_layer(xyz.contiguous(), new_xyz.contiguous(), rows_grad, idx, folded, pool=self.pool_method, use_xyz=self.use_xyz,
                                            new_xyz_lengths=count if with_lengths else None)
                outs.append(pooled.transpose(1, 2))
                continue
            grouped = grouper(xyz, new_xyz, features, rl, ql) if with_lengths else grouper(xyz, new_xyz, features)
            h = self.mlps[i](grouped)
            pool = F.max_pool2d if self.pool_method == "max_pool" else F.avg_pool2d
            h = pool(h, kernel_size=[1, h.size(3)]).squeeze(-1)
            if live is not None:
                h = torch.where(live.view(B, 1, M), h, h.new_zeros(()))
            outs.append(h)
        return new_xyz, torch.cat(outs, dim=1)


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction with one scale."""

    def __init__(self, *, mlp: List[int], npoint: int = None, radius: float = None, nsample: int = None, bn: bool = True, use_xyz: bool = True,
                 pool_method="max_pool", instance_norm=False):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz, pool_method=pool_method,
                         instance_norm=instance_norm)


class PointnetFPModule(nn.Module):
    """Feature propagation: the features of the `known` points are blended onto the `unknown` points from their three nearest
    known points, concatenated with the unknown points' own (skip) features and sent through the shared MLP `mlp` (its first entry
    counts C2 + C1).  weighting: "pointnet2" (weights 1 / (dist + 1e-8), normalised; the reference class) or "flownet3d"
    (1 / max(dist^2, 1e-10), normalised; FeaturePropagation of models/layers.py).  route: "measured" (default), "always" or "never"
    for the fused route when no gradient is wanted; grad_route: the same three values, independently, for the fused differentiable
    route (mcp_fp_mlp forward, mcp_fp_mlp_grad backward) when one is -- eligible in eval() or with bn=False.  bn_route: the same
    three values, independently, for the route with batch statistics (mcp_fp_mlp_bn_forward / mcp_fp_mlp_bn_backward) under train()
    with bn=True, with or without a wanted gradient; a call with lengths keeps the composition there (its batch statistics count the
    padded rows, the kernel's do not)."""

    def __init__(self, *, mlp: List[int], bn: bool = True):
        super().__init__()
        self.bn = bn
        self.weighting = "pointnet2"
        self.route = "measured"
        self.grad_route = "measured"
        self.bn_route = "measured"
        self.mlp = _shared_mlp(list(mlp), bn, False)
        self.__dict__["_packed"] = None

    # ---- fused route -----------------------------------------------------------------------------------------------------------
    def _layers(self):
        units = list(self.mlp.children())
        return [u.conv for u in units], [u.bn.bn if self.bn else None for u in units]

    def _packed_weights(self, c2):
        """(packed, widths) for c2 interpolated channels, kept until a parameter or buffer of the stack is written or replaced."""
        state = [*self.mlp.parameters(), *self.mlp.buffers()]
        key = (c2, *((id(t), t._version, t.device) for t in state))
        hit = self.__dict__["_packed"]
        if hit is None or hit[0] != key:
            hit = self.__dict__["_packed"] = (key, ops.fp_mlp_pack(*self._layers(), c2=c2))
        return hit[1]

    def fused(self, c2, c1, rows):
        """Whether a call with c2 known and c1 skip channels over `rows` = B * n unknown points takes the fused route."""
        if self.training or self.route == "never" or self.weighting not in ("pointnet2", "flownet3d"):
            return False
        convs = self._layers()[0]
        widths = [c.out_channels for c in convs]
        if not convs or convs[0].in_channels != c2 + c1 or not ops.fp_mlp_supported(c2, c1, widths):
            return False
        return self.route == "always" or ops.fp_mlp_routes_fused(c2, c1, widths, rows)

    def fused_grad(self, c2, c1, rows):
        """Whether a call that wants a gradient takes the fused differentiable route: BatchNorm folded (eval mode) or absent."""
        if (self.training and self.bn) or self.grad_route == "never" or self.weighting not in ("pointnet2", "flownet3d"):
            return False
        convs = self._layers()[0]
        widths = [c.out_channels for c in convs]
        if not convs or convs[0].in_channels != c2 + c1 or not ops.fp_mlp_grad_supported(c2, c1, widths):
            return False
        return self.grad_route == "always" or ops.fp_mlp_grad_routes_fused(c2, c1, widths, rows)

    def fused_bn(self, c2, c1, rows, with_lengths=False):
        """Whether a call under train() with BatchNorm takes the fused route with batch statistics (a batch of one row is left to
        torch, which refuses it)."""
        if not (self.training and self.bn) or with_lengths or rows < 2 or self.bn_route == "never" or self.weighting not in ("pointnet2", "flownet3d"):
            return False
        convs = self._layers()[0]
        widths = [c.out_channels for c in convs]
        if not convs or convs[0].in_channels != c2 + c1 or not ops.fp_mlp_bn_supported(c2, c1, widths):
            return False
        return self.bn_route == "always" or ops.fp_mlp_bn_routes_fused(c2, c1, widths, rows)

    def weights(self, dist):
        """(B,n,3) interpolation weights of three_nn's distances under `weighting`; a row without a finite distance gets zeros."""
        if self.weighting == "pointnet2":
            recip = 1.0 / (dist + 1e-8)
        elif self.weighting == "flownet3d":
            recip = 1.0 / (dist * dist).clamp_min(1e-10)
        else:
            raise NotImplementedError(self.weighting)
        norm = torch.sum(recip, dim=2, keepdim=True)
        return recip / torch.where(norm > 0, norm, torch.ones_like(norm))

    def forward(self, unknown: torch.Tensor, known: torch.Tensor, unknow_feats: torch.Tensor, known_feats: torch.Tensor, unknown_lengths=None,
                known_lengths=None) -> torch.Tensor:
        """unknown (B,n,3), known (B,m,3) or None, unknow_feats (B,C1,n) or None, known_feats (B,C2,m) -> (B, mlp[-1], n).  known=None
        broadcasts known_feats (B,C2,1) to every unknown point.  unknown_lengths / known_lengths (forms: ops.lengths_tensor):
        element b is its first unknown_lengths[b] unknown and known_lengths[b] known points; padded rows give zeros, and an element
        without a known point gets a zero interpolated part."""
        B, n = unknown.shape[0], unknown.shape[1]
        C2 = known_feats.shape[1]
        C1 = 0 if unknow_feats is None else unknow_feats.shape[1]
        with_lengths = known is not None and (unknown_lengths is not None or known_lengths is not None)
        ul = kl = None
        if with_lengths:
            ul = ops.lengths_tensor(unknown_lengths, B, n, unknown.device)
            kl = ops.lengths_tensor(known_lengths, B, known.shape[1], unknown.device)
        wants_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (unknown, known, unknow_feats, known_feats,
                                                                                                 *self.parameters()))
        if known is not None and self.fused_bn(C2, C1, B * n, with_lengths):
            dist, idx = pu.three_nn(unknown.detach().contiguous(), known.detach().contiguous())   # no gradient reaches the coordinates
            rows = known_feats.transpose(1, 2).contiguous()
            skip = None if unknow_feats is None else unknow_feats.transpose(1, 2).contiguous()
            convs, bns = self._layers()
            layers = [(c.weight.flatten(1), c.bias, b.weight, b.bias, b.eps) for c, b in zip(convs, bns)]
            out, stats, _ = ops.backend().fp_mlp_bn_layer(rows, skip, idx, dist, layers, rule=self.weighting)
            for b, (mean, var) in zip(bns, stats):
                _track(b, mean, var, B * n)
            return out.transpose(1, 2)
        if known is not None and not wants_grad and self.fused(C2, C1, B * n):
            packed, widths = self._packed_weights(C2)
            dist, idx = pu.three_nn(unknown.detach().contiguous(), known.detach().contiguous(), ul, kl)
            rows = known_feats.detach().transpose(1, 2).contiguous()
            skip = None if unknow_feats is None else unknow_feats.detach().transpose(1, 2).contiguous()
            out = ops.backend().fp_mlp(rows, skip, idx, dist, packed, widths, rule=self.weighting, unknown_lengths=ul)
            return out.transpose(1, 2)
        if known is not None and wants_grad and self.fused_grad(C2, C1, B * n):
            dist, idx = pu.three_nn(unknown.detach().contiguous(), known.detach().contiguous(), ul, kl)   # no gradient reaches the coordinates
            rows = known_feats.transpose(1, 2).contiguous()
            skip = None if unknow_feats is None else unknow_feats.transpose(1, 2).contiguous()
            folded = [ops.fold_conv_bn_grad(c, b) for c, b in zip(*self._layers())]
            out = ops.backend().fp_mlp_layer(rows, skip, idx, dist, folded, rule=self.weighting, unknown_lengths=ul)
            return out.transpose(1, 2)
        if known is not None:
            dist, idx = pu.three_nn(unknown.contiguous(), known.contiguous(), ul, kl)
            interpolated = pu.three_interpolate(known_feats.contiguous(), idx, self.weights(dist).contiguous())
        else:
            interpolated = known_feats.expand(*known_feats.size()[0:2], n)
        new_features = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
        h = self.mlp(new_features.unsqueeze(-1)).squeeze(-1)
        if ul is not None:
            live = torch.arange(n, device=h.device).view(1, n) < ul.clamp(0, n).view(B, 1)
            h = torch.where(live.view(B, 1, n), h, h.new_zeros(()))
        return h
