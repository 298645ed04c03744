"""Ball query under per-cloud lengths -- mcp_ball_query_lengths, mcp_query_and_group_lengths (csrc/pointnet2_ops.hip) and the
box-pruned mcp_ball_query_pruned (csrc/ball_query_pruned.hip) -- and three_nn with lengths, against the CPU oracle run on every
element's prefixes on their own.  Row 0 of every cloud lies far away, so point 0 is never a hit and a row of zeros means "no hit".
The padding is hostile: padded reference rows are copies of live centres (an unmasked kernel returns them as hits) and padded
centres hold 1e30; a second filling (-5e29 / NaN) must not move a single output bit.  Every ball-query case asserts that the oracle
alone yields all three kinds of centre: no hit, fewer than nsample hits, at least nsample hits."""
import functools
import math

import pytest
import torch

from mocopci_amd import _lib, compat, ops
from mocopci_amd import pointnet2_utils as pu
from oracle import pointset as orc
from tests.test_knn_lengths_gpu import cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAR = 1e4

A = (3, 130, 200, (130, 64, 3), (200, 65, 1))        # a partial tile, a one-point cloud, 4 waves per workgroup, the last one ragged
B_ = (2, 300, 2048, (300, 129), (2048, 1000))        # 32 tiles, a live prefix that ends inside a tile
C = (2, 64, 20000, (64, 40), (20000, 16500))         # the multi-step cloud builder beyond 16384
D = (1, 64, 65536, (64,), (65000,))                  # the largest supported cloud


def fill_padding(xyz, centres, qlen, rlen, filling):
    """filling 0: padded reference rows are copies of live centres, padded centres 1e30.  filling 1: -5e29 / NaN."""
    xyz, centres = xyz.clone(), centres.clone()
    for b in range(xyz.shape[0]):
        ql, rl = qlen[b], rlen[b]
        if filling == 0:
            xyz[b, rl:] = centres[b, torch.arange(xyz.shape[1] - rl) % ql] if ql else 0.0
            centres[b, ql:] = 1e30
        else:
            xyz[b, rl:] = -5e29
            centres[b, ql:] = float("nan")
    return xyz.contiguous(), centres.contiguous()


@functools.lru_cache(maxsize=None)
def clouds(B, M, N, qlen, rlen, filling=0):
    xyz, centres = cloud(2000 + N, B, N), cloud(1000 + M, B, M)
    xyz[:, 0] = FAR
    return fill_padding(xyz, centres, qlen, rlen, filling)


LATTICE_LENGTHS = ((230, 230), (1025, 700))


@functools.lru_cache(maxsize=None)
def lattice(filling=0):
    """The 16 x 16 x 4 integer lattice shuffled with seed 5, behind a far row 0 (1025 rows), twice: element 0 whole, element 1 its
    first 700 rows.  Centres: 100 lattice points, 100 lattice points + 0.5, 30 lattice points + 100."""
    g = torch.Generator().manual_seed(5)
    pts = torch.stack(torch.meshgrid(torch.arange(16.), torch.arange(16.), torch.arange(4.), indexing="ij"), -1).reshape(-1, 3)
    pts = pts[torch.randperm(1024, generator=g)]
    xyz = torch.cat([torch.full((1, 3), FAR), pts]).unsqueeze(0).repeat(2, 1, 1)
    centres = torch.cat([pts[:100], pts[100:200] + 0.5, pts[200:230] + 100.0]).unsqueeze(0).repeat(2, 1, 1)
    return fill_padding(xyz, centres, *LATTICE_LENGTHS, filling)


def counts_of(idx):
    """min(hits, nsample) from a reference row, given that point 0 is never a hit: zeros = no hit; otherwise the hits ascend and
    the tail repeats the first (smallest) one."""
    if idx.shape[-1] == 1:
        return (idx[..., 0] != 0).int()
    rising = (idx[..., 1:] > idx[..., :-1]).sum(-1) + 1
    return torch.where(idx[..., 0] != 0, rising, torch.zeros_like(rising)).int()


def oracle_rows(xyz, centres, qlen, rlen, r, ns):
    """(idx, cnt, kinds): the oracle on each element's prefixes, zeros elsewhere; kinds = (none, partial, full) per element."""
    B, M = centres.shape[:2]
    idx = torch.zeros(B, M, ns, dtype=torch.int32)
    for b in range(B):
        if qlen[b] and rlen[b]:
            idx[b, :qlen[b]] = orc.ball_query(r, ns, xyz[b:b + 1, :rlen[b]], centres[b:b + 1, :qlen[b]])[0]
    cnt = counts_of(idx)
    kinds = [(int((cnt[b, :qlen[b]] == 0).sum()), int(((cnt[b, :qlen[b]] > 0) & (cnt[b, :qlen[b]] < ns)).sum()), int((cnt[b, :qlen[b]] == ns).sum()))
             for b in range(B)]
    return idx, cnt, kinds


@functools.lru_cache(maxsize=None)
def expected(case, r, ns):
    B, M, N, qlen, rlen = case
    return oracle_rows(*clouds(B, M, N, qlen, rlen), qlen, rlen, r, ns)


def assert_all_kinds(kinds):
    total = [sum(k[i] for k in kinds) for i in range(3)]
    assert all(total), f"the case lacks a kind of centre (none, partial, full): {kinds}"


def dev_lengths(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def run_exhaustive(xyz, centres, qlen, rlen, r, ns):
    """mcp_ball_query_lengths, called directly; outputs pre-filled so that an unwritten slot shows."""
    B, N, _ = xyz.shape
    M = centres.shape[1]
    xd, cd = xyz.to(DEV), centres.to(DEV)
    idx, cnt = torch.full((B, M, ns), -77, dtype=torch.int32, device=DEV), torch.full((B, M), -77, dtype=torch.int32, device=DEV)
    ql, rl = (None if v is None else dev_lengths(v) for v in (qlen, rlen))
    ops._call("mcp_ball_query_lengths", xd, B, N, M, float(r), ns, _lib.fptr(cd), _lib.fptr(xd), None if ql is None else _lib.iptr(ql),
              None if rl is None else _lib.iptr(rl), _lib.iptr(idx), _lib.iptr(cnt))
    return idx.cpu(), cnt.cpu()


def run_pruned(xyz, centres, qlen, rlen, r, ns):
    """mcp_ball_query_pruned on a cloud built under the same lengths; outputs pre-filled."""
    B, N, _ = xyz.shape
    M = centres.shape[1]
    xd, cd = xyz.to(DEV), centres.to(DEV)
    ql, rl = (None if v is None else dev_lengths(v) for v in (qlen, rlen))
    rs, rperm, boxes = ops.backend()._build_cloud(xd, rl)
    idx, cnt = torch.full((B, M, ns), -77, dtype=torch.int32, device=DEV), torch.full((B, M), -77, dtype=torch.int32, device=DEV)
    ops._call("mcp_ball_query_pruned", xd, B, N, M, float(r), ns, _lib.fptr(cd), _lib.fptr(rs), _lib.iptr(rperm), _lib.fptr(boxes),
              None if ql is None else _lib.iptr(ql), None if rl is None else _lib.iptr(rl), _lib.iptr(idx), _lib.iptr(cnt))
    return idx.cpu(), cnt.cpu()


BOTH = (run_exhaustive, run_pruned)

CASES = {
    "A": (A, ((8.0, 16, [(1, 129, 0), (17, 47, 0), (3, 0, 0)]), (20.0, 8, [(0, 0, 130), (0, 16, 48), (3, 0, 0)]))),
    "B": (B_, ((1.0, 16, [(244, 56, 0), (120, 9, 0)]), (6.0, 32, [(0, 199, 101), (0, 129, 0)]),
               (12.0, 64, [(0, 9, 291), (0, 59, 70)]))),   # r = 12: more hits than slots, spread over many tiles -- catches a wrong merge
    "C": (C, ((0.5, 16, [(44, 20, 0), (34, 6, 0)]), (3.0, 16, [(0, 0, 64), (0, 0, 40)]))),
    "D": (D, ((0.3, 8, [(51, 13, 0)]), (2.0, 32, [(0, 5, 59)]))),
}


@pytest.mark.parametrize("name", list(CASES))
def test_both_searches_equal_the_oracle_on_prefixes(name):
    case, settings = CASES[name]
    B, M, N, qlen, rlen = case
    seen = []
    for r, ns, kinds in settings:
        want_i, want_c, got_kinds = expected(case, r, ns)
        assert got_kinds == kinds, (r, ns, got_kinds)
        seen += got_kinds
        for run in BOTH:
            for filling in (0, 1):
                idx, cnt = run(*clouds(B, M, N, qlen, rlen, filling), qlen, rlen, r, ns)
                assert torch.equal(idx, want_i) and torch.equal(cnt, want_c), (r, ns, run.__name__, filling)
    assert_all_kinds(seen)


def test_more_slots_than_a_wave_runs_exhaustively_and_the_pruned_entry_refuses():
    B, M, N, qlen, rlen = A
    want_i, want_c, kinds = expected(A, 20.0, 70)
    for filling in (0, 1):
        idx, cnt = run_exhaustive(*clouds(B, M, N, qlen, rlen, filling), qlen, rlen, 20.0, 70)
        assert torch.equal(idx, want_i) and torch.equal(cnt, want_c)
    assert any(k[1] for k in kinds) and any(k[0] for k in kinds)
    with pytest.raises(_lib.Unsupported):
        run_pruned(*clouds(B, M, N, qlen, rlen), qlen, rlen, 20.0, 70)
    # through the backend: the rule keeps nsample > 64 off the pruned route whatever the thresholds
    xyz, centres = (t.to(DEV) for t in clouds(B, M, N, qlen, rlen))
    idx, cnt = ops.backend().ball_query(xyz, centres, 20.0, 70, xyz_lengths=list(rlen), new_xyz_lengths=list(qlen), return_count=True)
    assert torch.equal(idx.cpu(), want_i) and torch.equal(cnt.cpu(), want_c)


def test_lattice_points_and_box_faces_at_exactly_r_are_excluded():
    """Integer coordinates: every distance is exact, many points lie at exactly r (r = 2; r = float32(sqrt 3), where the host-side
    float product r * r decides, for every route alike, whether 3 < r * r) and tile-box faces lie at exactly r from lattice
    centres.  Strict < and the slack-free box bound."""
    qlen, rlen = LATTICE_LENGTHS
    seen = []
    for r, ns, kinds in ((2.0, 16, [(30, 38, 162), (30, 111, 89)]), (2.0, 32, [(30, 185, 15), None]),
                         (float(torch.tensor(3.0).sqrt()), 32, [None, None])):
        want_i, want_c, got = oracle_rows(*lattice(), qlen, rlen, r, ns)
        assert all(k is None or k == g for k, g in zip(kinds, got)), (r, ns, got)
        seen += got
        for run in BOTH:
            for filling in (0, 1):
                idx, cnt = run(*lattice(filling), qlen, rlen, r, ns)
                assert torch.equal(idx, want_i) and torch.equal(cnt, want_c), (r, ns, run.__name__, filling)
    assert_all_kinds(seen)


def test_empty_sides():
    B, M, N, qlen, rlen = 2, 70, 100, (0, 70), (100, 0)
    for run in BOTH:
        for filling in (0, 1):
            idx, cnt = run(*clouds(B, M, N, qlen, rlen, filling), qlen, rlen, 8.0, 16)
            assert not idx.any() and not cnt.any(), (run.__name__, filling)
    xyz, centres = (t.to(DEV) for t in clouds(B, M, N, qlen, rlen))
    feats = torch.full((B, 4, N), float("nan"), device=DEV)
    out = pu.QueryAndGroup(8.0, 16)(xyz, centres, feats, xyz_lengths=list(rlen), new_xyz_lengths=list(qlen))
    assert out.shape == (B, 7, M, 16) and not out.any()
    feats.requires_grad_(True)   # the composed route: what index 0 gathers there is padding, and is masked to exact zeros
    out = pu.QueryAndGroup(8.0, 16)(xyz, centres, feats, xyz_lengths=list(rlen), new_xyz_lengths=list(qlen))
    out.sum().backward()
    assert out.shape == (B, 7, M, 16) and not out.any() and not feats.grad.any()


def test_null_and_full_lengths_equal_the_length_free_ball_query():
    B, M, N = 2, 130, 2100
    xyz, centres = clouds(B, M, N, (M, M), (N, N))
    want = pu.ball_query(6.0, 16, xyz.to(DEV), centres.to(DEV)).cpu()
    assert torch.equal(want, orc.ball_query(6.0, 16, xyz, centres))
    want_c = counts_of(want)
    assert (want_c == 16).any() and (want_c < 16).any()
    for run in BOTH:
        for ql, rl in ((None, None), ((M, M), (N, N)), (None, (N, N)), ((M, M), None)):
            idx, cnt = run(xyz, centres, ql, rl, 6.0, 16)
            assert torch.equal(idx, want) and torch.equal(cnt, want_c), (run.__name__, ql, rl)


# ---- QueryAndGroup -------------------------------------------------------------------------------------------------------------
def composed(xyz, centres, feats, idx, qlen, rlen, use_xyz):
    """The module's definition from the oracle's grouping on a given idx, zeros for padded centres and point-less elements."""
    parts = []
    if use_xyz or feats is None:
        parts.append(orc.grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - centres.transpose(1, 2).unsqueeze(-1))
    if feats is not None:
        parts.append(orc.grouping_operation(feats, idx))
    out = torch.cat(parts, dim=1)
    for b in range(xyz.shape[0]):
        out[b, :, qlen[b]:] = 0.0
        if rlen[b] == 0:
            out[b] = 0.0
    return out


@pytest.mark.parametrize("r,ns", [(8.0, 16), (20.0, 8), (20.0, 70)])
@pytest.mark.parametrize("C_,use_xyz", [(0, True), (5, True), (5, False)])
def test_query_and_group_with_lengths(r, ns, C_, use_xyz):
    """One launch (ns <= 64) or the composition (ns = 70) against the composed definition; padded feature columns are NaN or huge."""
    B, M, N, qlen, rlen = A
    want_i = expected(A, r, ns)[0]
    outs = []
    for filling in (0, 1):
        xyz, centres = clouds(B, M, N, qlen, rlen, filling)
        feats = None
        if C_:
            feats = torch.randn(B, C_, N, generator=torch.Generator().manual_seed(3))
            for b in range(B):
                feats[b, :, rlen[b]:] = float("nan") if filling else 3e38
        want = composed(xyz, centres, feats, want_i, qlen, rlen, use_xyz)   # live rows gather live rows only; the rest is overwritten
        module = pu.QueryAndGroup(r, ns, use_xyz=use_xyz)
        out = module(xyz.to(DEV), centres.to(DEV), None if feats is None else feats.to(DEV), xyz_lengths=list(rlen), new_xyz_lengths=list(qlen)).cpu()
        assert torch.equal(out, want), filling
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def test_query_and_group_gradient_equals_the_length_free_module_on_slices():
    B, M, N, qlen, rlen = A
    xyz, centres = (t.to(DEV) for t in clouds(B, M, N, qlen, rlen, 1))
    base = torch.randn(B, 5, N, generator=torch.Generator().manual_seed(4)).to(DEV)
    for b in range(B):
        base[b, :, rlen[b]:] = float("nan")
    feats = base.clone().requires_grad_(True)
    module = pu.QueryAndGroup(8.0, 16)
    out = module(xyz, centres, feats, xyz_lengths=list(rlen), new_xyz_lengths=list(qlen))
    weight = torch.randn(out.shape, generator=torch.Generator().manual_seed(6)).to(DEV)
    (out * weight).sum().backward()
    for b in range(B):
        ql, rl = qlen[b], rlen[b]
        fb = base[b:b + 1, :, :rl].clone().contiguous().requires_grad_(True)
        ob = module(xyz[b:b + 1, :rl].contiguous(), centres[b:b + 1, :ql].contiguous(), fb)
        assert torch.equal(out[b:b + 1, :, :ql].detach(), ob.detach())
        (ob * weight[b:b + 1, :, :ql]).sum().backward()
        assert torch.equal(feats.grad[b, :, :rl], fb.grad[0]), b
        assert not feats.grad[b, :, rl:].any(), b


# ---- three_nn ------------------------------------------------------------------------------------------------------------------
def three_nn_expected(unknown, known, ulen, klen):
    B, n = unknown.shape[:2]
    dist, idx = torch.zeros(B, n, 3), torch.zeros(B, n, 3, dtype=torch.int32)
    for b in range(B):
        if ulen[b] and klen[b]:
            dist[b, :ulen[b]], idx[b, :ulen[b]] = (t[0] for t in orc.three_nn(unknown[b:b + 1, :ulen[b]], known[b:b + 1, :klen[b]]))
        elif ulen[b]:
            dist[b, :ulen[b]] = float("inf")
    return dist, idx


@pytest.mark.parametrize("case", [A, B_])
def test_three_nn_with_lengths(case, monkeypatch):
    """Both routes of the K = 3 search (the padded sizes forced over the pruned KNN thresholds by the class attributes) against the
    oracle on prefixes, with the +inf / 0 tail where fewer than three points are known (A: one point).  Indices and the kernels'
    squared distances are exact; three_nn's own distances pass through the device's sqrt, which may differ from the host's by an
    ulp (2^-23 relative), so they are held to rtol 2e-7 against the oracle -- and to equal bits between fillings and routes."""
    B, M, N, ulen, klen = case
    want_d, want_i = three_nn_expected(*reversed(clouds(B, M, N, ulen, klen)), ulen, klen)
    if case is A:
        assert math.isinf(want_d[2, 0, 1]) and math.isinf(want_d[2, 0, 2]) and want_i[2, 0].tolist() == [0, 0, 0] and not math.isinf(want_d[2, 0, 0])
    got = []
    for pruned_route in (False, True):
        monkeypatch.setattr(ops.HipBackend, "PRUNE_LENGTHS_MIN_REFS", 1 if pruned_route else 1 << 30)
        monkeypatch.setattr(ops.HipBackend, "PRUNE_LENGTHS_MIN_QUERIES", 1)
        assert ops.HipBackend.prunes_with_lengths(M, N, 3) == pruned_route
        for filling in (0, 1):
            known, unknown = (t.to(DEV) for t in clouds(B, M, N, ulen, klen, filling))
            dist, idx = pu.three_nn(unknown, known, list(ulen), list(klen))
            assert idx.dtype == torch.int32 and torch.equal(idx.cpu(), want_i), (pruned_route, filling)
            torch.testing.assert_close(dist.cpu(), want_d, rtol=2e-7, atol=0)
            _, d2 = ops.backend().knn(unknown, known, 3, mode=ops.MCP_DIST_DIRECT, return_dist=True, query_lengths=list(ulen), ref_lengths=list(klen))
            for b in range(B):   # the squared distances of the live entries, through the host's sqrt: the oracle's bits
                k = min(3, klen[b])
                assert torch.equal(torch.sqrt(d2[b, :ulen[b], :k].cpu()), want_d[b, :ulen[b], :k]), (pruned_route, filling, b)
            got.append((dist.cpu(), idx.cpu()))
    assert all(torch.equal(g[0], got[0][0]) and torch.equal(g[1], got[0][1]) for g in got)


# ---- the backend's routes --------------------------------------------------------------------------------------------------------
def test_backend_routes_return_equal_bits_and_a_scope_builds_the_cloud_once(monkeypatch):
    B, M, N, qlen, rlen = B_
    xyz, centres = (t.to(DEV) for t in clouds(B, M, N, qlen, rlen))
    ql, rl = dev_lengths(qlen), dev_lengths(rlen)
    be = ops.HipBackend()
    builds = []
    real = be._build_cloud
    monkeypatch.setattr(be, "_build_cloud", lambda *a, **k: (builds.append(1), real(*a, **k))[1])
    calls = []
    real_call = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    got = {}
    for pruned in (False, True):
        monkeypatch.setattr(ops.HipBackend, "BALL_PRUNE_MIN_REFS", 1 if pruned else 1 << 30)
        monkeypatch.setattr(ops.HipBackend, "BALL_PRUNE_MIN_CENTRES", 1)
        assert ops.HipBackend.prunes_ball(M, N, 32) == pruned
        del calls[:]
        got[pruned] = be.ball_query(xyz, centres, 6.0, 32, xyz_lengths=rl, new_xyz_lengths=ql, return_count=True)
        assert ("mcp_ball_query_pruned" in calls) == pruned and ("mcp_ball_query_lengths" in calls) != pruned, calls
    want_i, want_c, _ = expected(B_, 6.0, 32)
    for pruned in (False, True):
        assert torch.equal(got[pruned][0].cpu(), want_i) and torch.equal(got[pruned][1].cpu(), want_c), pruned
    assert len(builds) == 1   # outside a scope: one build per pruned call
    del builds[:]
    with be.cloud_scope():
        a = be.ball_query(xyz, centres, 1.0, 16, xyz_lengths=rl, new_xyz_lengths=ql)
        b = be.ball_query(xyz, centres, 12.0, 64, xyz_lengths=rl, new_xyz_lengths=ql)
        assert len(builds) == 1, builds
    assert torch.equal(a.cpu(), expected(B_, 1.0, 16)[0]) and torch.equal(b.cpu(), expected(B_, 12.0, 64)[0])
    # the operator API takes the same routes: pointnet2_utils.ball_query with lengths
    assert torch.equal(pu.ball_query(6.0, 32, xyz, centres, rl, ql).cpu(), want_i)
    # the shape rule off (no supported cloud reaches the bound): the pruned route is taken where the scope already holds the cloud
    monkeypatch.setattr(ops.HipBackend, "BALL_PRUNE_MIN_REFS", 1 << 30)
    del builds[:], calls[:]
    with be.cloud_scope():
        c = be.ball_query(xyz, centres, 6.0, 32, xyz_lengths=rl, new_xyz_lengths=ql)
        assert calls == ["mcp_ball_query_lengths"] and not builds
        be.prebuild_cloud(xyz, rl)
        d = be.ball_query(xyz, centres, 6.0, 32, xyz_lengths=rl, new_xyz_lengths=ql)
        e = be.ball_query(xyz, centres, 1.0, 16, xyz_lengths=rl, new_xyz_lengths=ql)
        assert calls.count("mcp_ball_query_pruned") == 2 and len(builds) == 1, (calls, builds)
        f = be.ball_query(xyz, centres, 6.0, 32, xyz_lengths=dev_lengths(rlen), new_xyz_lengths=ql)   # other lengths tensor: not held
        assert calls[-1] == "mcp_ball_query_lengths" and len(builds) == 1
    assert all(torch.equal(t.cpu(), want_i) for t in (c, d, f)) and torch.equal(e.cpu(), a.cpu())


def test_compat_ball_query_pads_as_pytorch3d():
    B, M, N, qlen, rlen = A
    r, K = 8.0, 16
    want_i, want_c, _ = expected(A, r, K)
    for filling in (0, 1):
        xyz, centres = clouds(B, M, N, qlen, rlen, filling)
        dists, idx, nn = compat.ball_query(centres.to(DEV), xyz.to(DEV), lengths1=torch.tensor(qlen), lengths2=torch.tensor(rlen), K=K, radius=r)
        assert idx.dtype == torch.int64 and idx.shape == dists.shape == (B, M, K) and nn.shape == (B, M, K, 3)
        pad = torch.arange(K).view(1, 1, K) >= want_c.unsqueeze(-1)
        assert torch.equal(idx.cpu(), torch.where(pad, torch.tensor(-1), want_i.long()))
        want_nn = torch.where(pad.unsqueeze(-1), torch.zeros(()), orc.group_rows(clouds(B, M, N, qlen, rlen)[0], torch.where(pad, 0, want_i)))
        assert torch.equal(nn.cpu(), want_nn)
        live_centres = torch.where(pad.unsqueeze(-1), torch.zeros(()), clouds(B, M, N, qlen, rlen)[1].unsqueeze(2).expand(B, M, K, 3))
        want_d = ((want_nn.double() - live_centres.double()) ** 2).sum(-1)
        # float32 sum of three float32 squares of float32 differences, all terms non-negative: a difference is rounded once and
        # squared (2), the square (1) and the two additions (2) once each -- five roundings of 2^-24, and one more for their products
        torch.testing.assert_close(dists.cpu().double(), want_d, rtol=6 * 2.0 ** -24, atol=0.0)
        assert not dists.cpu()[pad].any() and (dists.cpu()[~pad] < r * r).all()
    assert compat.ball_query(centres.to(DEV), xyz.to(DEV), K=K, radius=r, return_nn=False)[2] is None
