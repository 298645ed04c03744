"""Float64 statements of the fused point layers (csrc/fusion.hip, cross.hip, pointconv.hip, ptblock.hip), written from the layer
definitions, each with a running error bound computed beside the value.  A plain module: test_fused_reference_cpu.py checks the
statements against the fp32 oracle, test_fused_variants_gpu.py checks the kernels against them.

Every reference returns (exact, bound) for the selected points, both float64 of shape (points, channels).  `bound` is in units of
2^-24 (one fp32 rounding of a value of magnitude 1): a correct fp32 evaluation of the layer is within c * 2^-24 * bound of `exact`
with a small constant c per kernel family.  The rules, applied stage by stage:

  * a coordinate difference carries one rounding of its own magnitude;
  * a product stage of length K, z = W x + b, adds sqrt(K) * (|W| @ |x| + |b|) and pushes the incoming bound through |W|
    (product_stage) -- the form of test_kernel_variants_gpu.py; the aggregation of PointConv is the same with both operands
    uncertain;
  * ReLU, LeakyReLU and maxima are 1-Lipschitz: they pass the bound on (a maximum: the largest bound among its arguments);
  * sums of two or three fp32 terms add one rounding of each partial sum's magnitude;
  * a softmax-weighted sum out = sum_j a_j v_j moves by sum_j a_j (v_j - out) d_j when logit j moves by d_j, so a logit bound e_j
    adds sum_j a_j e_j |v_j - out| -- never more than max(e) times twice the weighted magnitude sum_j a_j |v_j|, and much less where
    the values share a large offset, as neighbour coordinates do --, to which come the values' own bounds, the rounding of
    logit - max and of exp (|logit - max| + 2 units on e_j) and the J-long sum with its product and division (sqrt(J) + 2 units of
    the weighted magnitude) (softmax_sum).

cut: None, or a function on fp32 tensors applied to every multiplicand of a product stage (weights and activations) before the
product -- test_kernel_variants_gpu.two_term gives what a kernel that lost the third term of the bf16 split would compute.
sel: flat indices (batch * points + point) of the points wanted, default all; the work is done in row blocks.

The *_inputs functions build the test data of a case (CPU fp32 tensors): clustered clouds whose neighbour lists are real
neighbours, so that relative coordinates come from a cancellation, and features and weights with a positive mean, so that the
truncation errors of a two-term split add up instead of cancelling (see the docstring of test_kernel_variants_gpu.py).  A case's
optional "seed" is added to the seed its shape gives (the backward cases choose it, see fused_grad_reference.py)."""
import math

import torch

U = 2.0 ** -24
CLOUD_EXTENT = (40.0, 40.0, 3.0)   # tests/test_ops_gpu.cloud


def _op(cut, t):
    return t.double() if cut is None else cut(t.float()).double()


def leaky(z, slope):
    return torch.where(z > 0, z, z * slope)


def product_stage(x, xb, w, b, cut=None):
    """z = W x + b over the last axis of x (..., K) with w (n, K), b (n,); xb is the bound x arrives with."""
    wa, ba = w.double().abs(), b.double().abs()
    z = _op(cut, x) @ _op(cut, w).T + b.double()
    zb = math.sqrt(w.shape[1]) * (x.abs() @ wa.T + ba) + xb @ wa.T
    return z, zb


def softmax_sum(s, sb, v, vb):
    """sum_j softmax_j(s) v over axis 1: s, sb (P, J, C or 1) logits and their bound, v, vb (P, J, C) values and their bound."""
    eps = sb + (s - s.amax(1, keepdim=True)).abs() + 2.0
    a = torch.softmax(s, 1)
    out = (a * v).sum(1)
    bound = (a * eps * (v - out[:, None]).abs()).sum(1) + (a * vb).sum(1) + (math.sqrt(s.shape[1]) + 2.0) * (a * v.abs()).sum(1)
    return out, bound


def _blocks(total, sel, block):
    sel = torch.arange(total) if sel is None else torch.as_tensor(sel, dtype=torch.long)
    for r0 in range(0, sel.numel(), block):
        yield sel[r0:r0 + block]


def _run(block_fn, total, n, sel, block):
    """block_fn(batch ids, point ids) -> (exact, bound) over the flat points `sel` of (B, n) in blocks."""
    outs = [block_fn(s // n, s % n) for s in _blocks(total, sel, block)]
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


def _whole(idx):
    return torch.cat(list(idx), dim=-1) if isinstance(idx, (tuple, list)) else idx


# ---- fusion (mocopci.py:803-819, BatchNorm folded): MLP 4 -> 64 -> 64 -> 128 on [p2_j - p1_i, |p2_j - p1_i|], channel max,
# softmax over the 64 neighbours, blend of the neighbour coordinates -------------------------------------------------------------
def fusion_reference(p1, p2, idx, w1, b1, w2, b2, w3, b3, sel=None, cut=None, block=1024):
    B, N, _ = p1.shape
    idx = _whole(idx)

    def blk(b, i):
        nb = p2[b[:, None], idx[b, i].long()].double()                   # (P, 64, 3)
        resi = nb - p1[b, i].double()[:, None]
        dist = resi.square().sum(-1, keepdim=True).sqrt()
        # |d dist| <= |resi . d resi| / dist <= |d resi| (Cauchy-Schwarz) = one unit of dist, plus the squares, the sums and the root
        x, xb = torch.cat([resi, dist], -1), torch.cat([resi.abs(), 4.0 * dist], -1)
        for w, bias in ((w1, b1), (w2, b2), (w3, b3)):
            z, xb = product_stage(x, xb, w, bias, cut)
            x = torch.relu(z)
        return softmax_sum(x.amax(-1, keepdim=True), xb.amax(-1, keepdim=True), nb, torch.zeros_like(nb))

    return _run(blk, B * N, N, sel, block)


# ---- cross volume (pointconv_util.py:765-781, one mlp layer): leaky(points2_j + points1_i + Wpos (xyz2_j - xyz1_i) + bpos), a D x D
# Linear with LeakyReLU, maximum over the 32 neighbours --------------------------------------------------------------------------------
def cross_reference(xyz1, xyz2, points1, points2, idx, wpos, bpos, wmlp, bmlp, sel=None, cut=None, block=512):
    B, N1, _ = xyz1.shape
    idx = _whole(idx)

    def blk(b, i):
        j = idx[b, i].long()
        d = xyz2[b[:, None], j].double() - xyz1[b, i].double()[:, None]
        pos, posb = product_stage(d, d.abs(), wpos, bpos, cut)           # (P, 32, D)
        f1, g2 = points1[b, i].double()[:, None], points2[b[:, None], j].double()
        x0 = (f1 + pos) + g2
        # three-term sum in either order (the kernel starts the K = 4 product from the points1 row): partial sums stay below |f1| + |g2|
        x0b = posb + 2.0 * (f1.abs() + g2.abs()) + x0.abs()
        z, zb = product_stage(leaky(x0, 0.1), x0b, wmlp, bmlp, cut)
        return leaky(z, 0.1).amax(1), zb.amax(1)

    return _run(blk, B * N1, N1, sel, block)


# ---- PointConv (mocopci.py:1218-1266, :1289-1300, :1330-1342): WeightNet 3 -> 8 -> 8 -> 8 on the relative coordinates, the (3 + D) x 8
# aggregate over the 32 neighbours, optionally Linear + LeakyReLU --------------------------------------------------------------------
def pointconv_agg_reference(s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, sel=None, cut=None, block=1024):
    B, S, _ = new_xyz.shape

    def blk(b, i):
        j = idx[b, i].long()
        g = s_xyz[b[:, None], j].double() - new_xyz[b, i].double()[:, None]      # (P, 32, 3)
        w, wb = g, g.abs()
        for ww, bias in ((w0, b0), (w1, b1), (w2, b2)):
            z, wb = product_stage(w, wb, ww, bias, cut)
            w = torch.relu(z)
        f = s_points[b[:, None], j].double()
        x, xb = torch.cat([g, f], -1), torch.cat([g.abs(), torch.zeros_like(f)], -1)   # (P, 32, 3 + D)
        xa, wa = x.abs().transpose(1, 2), w.abs()
        agg = _op(cut, x).transpose(1, 2) @ _op(cut, w)                                 # (P, 3 + D, 8): a 32-long product stage
        aggb = math.sqrt(x.shape[1]) * (xa @ wa) + xb.transpose(1, 2) @ wa + xa @ wb
        return agg.flatten(1), aggb.flatten(1)

    return _run(blk, B * S, S, sel, block)


def pointconv_linear_reference(s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, w, b, slope, sel=None, cut=None, block=1024):
    B, S, _ = new_xyz.shape
    outs = []
    for s in _blocks(B * S, sel, block):
        agg, aggb = pointconv_agg_reference(s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, sel=s, cut=cut, block=block)
        z, zb = product_stage(agg, aggb, w, b, cut)
        outs.append((leaky(z, slope), zb))
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


# ---- vector attention of the Point-Transformer block (pointT_layer2.py:64-75): delta_j = fc_delta(xyz_i - xyz_j),
# attn_j = fc_gamma(q_i - k_j + delta_j), per-channel softmax of attn / 8 over the 16 neighbours, blend of v_j + delta_j -------------------
def ptblock_reference(xyz, q, k, v, idx, wd1, bd1, wd2, bd2, wg1, bg1, wg2, bg2, sel=None, cut=None, block=2048):
    B, N, _ = xyz.shape

    def blk(b, i):
        j = idx[b, i].long()
        rel = xyz[b, i].double()[:, None] - xyz[b[:, None], j].double()          # (P, 16, 3)
        z, zb = product_stage(rel, rel.abs(), wd1, bd1, cut)
        delta, deltab = product_stage(torch.relu(z), zb, wd2, bd2, cut)
        qk = q[b, i].double()[:, None] - k[b[:, None], j].double()
        g = qk + delta
        z, zb = product_stage(g, deltab + qk.abs() + g.abs(), wg1, bg1, cut)
        attn, attnb = product_stage(torch.relu(z), zb, wg2, bg2, cut)
        logit = attn / 8.0                                               # the kernel multiplies by a rounded log2(e) / 8: two roundings
        val = v[b[:, None], j].double() + delta
        return softmax_sum(logit, attnb / 8.0 + 2.0 * logit.abs(), val, deltab + val.abs())

    return _run(blk, B * N, N, sel, block)


# ---- test data ---------------------------------------------------------------------------------------------------------------------
def clustered_cloud(g, b, n, size, extent=False, spread=0.5):
    """(b, n, 3): points i // size * size .. + size - 1 form one cluster of radius ~spread around a centre drawn from the extent of
    test_ops_gpu.cloud (extent=True) or from +-2."""
    ext = torch.tensor(CLOUD_EXTENT if extent else (2.0, 2.0, 2.0))
    centres = (torch.rand(b, (n + size - 1) // size, 3, generator=g) * 2 - 1) * ext
    return (centres.repeat_interleave(size, 1)[:, :n] + spread * torch.randn(b, n, 3, generator=g)).contiguous()


def cluster_neighbours(g, b, nq, nref, k, size, home=None):
    """(b, nq, k) int32: k members of the cluster of reference point home[i] (default i * nref // nq), starting at a random member;
    k > cluster size (or a cloud smaller than a cluster) repeats members."""
    home = torch.arange(nq) * nref // nq if home is None else home
    base = (home // size * size)[None, :, None]
    start = torch.randint(0, size, (b, nq, 1), generator=g)
    return ((base + (start + torch.arange(k)) % size) % nref).int().contiguous()


def positive_weights(g, n, k, gain=1.0, bias=0.0):
    """W ~ gain (N(0, 1) + 1) / K, b ~ N(bias, 0.1)."""
    return gain * (torch.randn(n, k, generator=g) + 1.0) / k, torch.randn(n, generator=g) * 0.1 + bias


def fusion_inputs(case):
    """p1, p2 (b, n, 3), (ia, ib) two (b, n, 32) lists, [w1, b1, w2, b2, w3, b3].  same: p2 is p1, so every list holds its own point
    (a zero-length vector); dup: the second list repeats the first."""
    b, n = case["b"], case["n"]
    g = torch.Generator().manual_seed(1000 * b + n + case.get("seed", 0))
    p1 = clustered_cloud(g, b, n, 64, case.get("extent", False))
    p2 = p1.clone() if case.get("same") else (p1 + 0.2 * torch.randn(b, n, 3, generator=g)).contiguous()
    ia = cluster_neighbours(g, b, n, n, 32, 64)
    ib = ia.clone() if case.get("dup") else cluster_neighbours(g, b, n, n, 32, 64)
    # scales chosen so that the scores of a point's neighbours differ by about one: a saturated softmax would hide the scores' errors
    ws = [*positive_weights(g, 64, 4, 2.0, -0.2), *positive_weights(g, 64, 64, 1.0, -0.1), *positive_weights(g, 128, 64, 2.0, -0.2)]
    return p1, p2, (ia, ib), ws


def cross_inputs(case):
    """xyz1 (b, n1, 3), xyz2 (b, n2, 3), points1, points2, (ia, ib) two (b, n1, 16) lists into cloud 2, [wpos, bpos, wmlp, bmlp]."""
    b, n1, n2, d = case["b"], case["n1"], case["n2"], case["d"]
    g = torch.Generator().manual_seed(b * 7919 + n1 * 31 + n2 + d + case.get("seed", 0))
    xyz2 = clustered_cloud(g, b, n2, 32, case.get("extent", False))
    home = torch.arange(n1) * n2 // n1
    xyz1 = (xyz2[:, home] + 0.2 * torch.randn(b, n1, 3, generator=g)).contiguous()
    p1, p2 = torch.randn(b, n1, d, generator=g) + 0.5, torch.randn(b, n2, d, generator=g) + 0.5
    ia, ib = (cluster_neighbours(g, b, n1, n2, 16, 32, home) for _ in range(2))
    return xyz1, xyz2, p1, p2, (ia, ib), [*positive_weights(g, d, 3, 1.0, 0.1), *positive_weights(g, d, d, 1.0, -0.5)]


def pointconv_inputs(case):
    """s_xyz (b, n, 3), new_xyz (b, s, 3) (points of s_xyz), s_points (b, n, d), idx (b, s, 32), the six WeightNet tensors and, with
    c_out, [w, b] of the Linear."""
    b, n, s, d = case["b"], case["n"], case["s"], case["d"]
    g = torch.Generator().manual_seed(b * 7919 + n * 31 + s + d + case.get("seed", 0))
    s_xyz = clustered_cloud(g, b, n, 32, case.get("extent", False))
    home = torch.arange(s) * n // s
    new_xyz = s_xyz[:, home].contiguous()
    pts = torch.randn(b, n, d, generator=g) + 0.5
    idx = cluster_neighbours(g, b, s, n, 32, 32, home)
    wn = [*positive_weights(g, 8, 3, 1.0, 0.2), *positive_weights(g, 8, 8, 2.0, 0.0), *positive_weights(g, 8, 8, 2.0, 0.0)]
    lin = []
    if case.get("c_out"):
        lin = list(positive_weights(g, case["c_out"], (d + 3) * 8, 1.0, -15.0))   # the product's median is about 17: both signs reach the LeakyReLU
    return s_xyz, new_xyz, pts, idx, wn, lin


def ptblock_inputs(case):
    """xyz (b, n, 3), q, k, v (b, n, 64), idx (b, n, 16), the eight weights.  same: the 16 neighbours of a point are one point;
    logits: fc_gamma's last layer scaled so that the largest |attn| / 8 is about this."""
    b, n = case["b"], case["n"]
    g = torch.Generator().manual_seed(b * 7919 + n + case.get("seed", 0))
    xyz = clustered_cloud(g, b, n, 16, case.get("extent", False))
    q, k, v = (torch.randn(b, n, 64, generator=g) + 0.5 for _ in range(3))
    idx = cluster_neighbours(g, b, n, n, 16, 16)
    if case.get("same"):
        idx = idx[..., :1].expand(b, n, 16).contiguous()
    ws = [*positive_weights(g, 64, 3, 1.0, 0.2), *positive_weights(g, 64, 64, 2.0, 0.0), *positive_weights(g, 64, 64, 2.0, 0.0),
          *positive_weights(g, 64, 64, 8.0, 0.0)]
    if case.get("logits"):
        attn = ptblock_logits(xyz, q, k, v, idx, *ws)
        f = float(case["logits"]) / attn.abs().max().item()
        ws[6], ws[7] = ws[6] * f, ws[7] * f
    return xyz, q, k, v, idx, ws


def ptblock_logits(xyz, q, k, v, idx, wd1, bd1, wd2, bd2, wg1, bg1, wg2, bg2):
    """attn / 8 of the block in fp32 (for scaling the data only)."""
    F = torch.nn.functional
    bi = torch.arange(xyz.shape[0])[:, None, None]
    j = idx.long()
    delta = F.linear(torch.relu(F.linear(xyz[:, :, None] - xyz[bi, j], wd1, bd1)), wd2, bd2)
    return F.linear(torch.relu(F.linear(q[:, :, None] - k[bi, j] + delta, wg1, bg1)), wg2, bg2) / 8.0
