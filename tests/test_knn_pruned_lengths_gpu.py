"""The pruned KNN search and its cloud builder under per-cloud lengths (mcp_build_cloud_lengths, mcp_morton_codes_lengths,
mcp_tile_boxes_lengths, mcp_knn_pruned_lengths in csrc/knn_pruned.hip): the builder against the plain builder run on each element's
prefix, the search against the CPU oracle on the prefixes (the references of tests/test_knn_lengths_gpu.py, computed once for both
files), the routing of HipBackend.knn / chamfer, and bitwise independence of everything from what the padding holds."""
import functools

import pytest
import torch

from mocopci_amd import _lib, compat, ops
from tests.test_knn_lengths_gpu import cloud, expected, padded_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD_CODE = 0x7FFFFFFF


def dev_lengths(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


def tiles_of(n):
    return (n + ops.backend().TILE - 1) // ops.backend().TILE


# ---- the builder ------------------------------------------------------------------------------------------------------------------
def padded_cloud(seed, B, n, lens, filling):
    x = cloud(seed, B, n)
    for b in range(B):
        x[b, lens[b]:] = 1e30 if filling == 0 else float("nan")
    return x.to(DEV)


def build_lengths(xyz, lens):
    """mcp_build_cloud_lengths, called directly; the outputs are pre-filled so that an unwritten row shows."""
    B, n, _ = xyz.shape
    s, perm = torch.full_like(xyz, -3.0), torch.full((B, n), -3, dtype=torch.int32, device=DEV)
    boxes = torch.full((B, tiles_of(n), 6), -3.0, device=DEV)
    ops._call("mcp_build_cloud_lengths", xyz, B, n, _lib.fptr(xyz), _lib.iptr(lens), _lib.fptr(s), _lib.iptr(perm), _lib.fptr(boxes))
    return s, perm, boxes


@pytest.mark.parametrize("B,n,lens", [(3, 200, (200, 65, 1)), (4, 2100, (2100, 1025, 64, 0)), (2, 16384, (16384, 8193))])   # IPT = 1, 4, 16
def test_builder_equals_the_plain_builder_on_each_prefix(B, n, lens):
    be = ops.backend()
    xyz = padded_cloud(300 + n, B, n, lens, 0)
    s, perm, boxes = build_lengths(xyz, dev_lengths(lens))
    for b, ln in enumerate(lens):
        t = tiles_of(ln)
        if ln:
            ws, wperm, wboxes = be._build_cloud(xyz[b:b + 1, :ln].contiguous())
            assert torch.equal(s[b, :ln], ws[0]) and torch.equal(perm[b, :ln], wperm[0]) and torch.equal(boxes[b, :t], wboxes[0]), (b, ln)
        assert torch.equal(perm[b, ln:], torch.arange(ln, n, dtype=torch.int32, device=DEV)), (b, ln)
        assert not s[b, ln:].any() and not boxes[b, t:].any(), f"rows beyond the length of element {b} are not zero"
    # another filling of the padding moves no bit of any output (a box that took a padded row in would show here and nowhere else)
    other = build_lengths(padded_cloud(300 + n, B, n, lens, 1), dev_lengths(lens))
    for a, o in zip((s, perm, boxes), other):
        assert torch.equal(a, o)


def test_builder_without_lengths_and_with_full_lengths_is_the_plain_builder():
    be = ops.backend()
    xyz = cloud(41, 2, 700).to(DEV)
    want = be._build_cloud(xyz)
    for got in (be._build_cloud(xyz, dev_lengths((700, 700))), build_lengths(xyz, dev_lengths((900, 2 ** 31 - 1)))):   # clamped by the kernel
        for a, w in zip(got, want):
            assert torch.equal(a, w)
    s, perm, boxes = (torch.empty_like(t) for t in want)
    ops._call("mcp_build_cloud_lengths", xyz, 2, 700, _lib.fptr(xyz), None, _lib.fptr(s), _lib.iptr(perm), _lib.fptr(boxes))
    assert torch.equal(s, want[0]) and torch.equal(perm, want[1]) and torch.equal(boxes, want[2])


def test_three_step_route_under_lengths():
    """Clouds beyond 16384 points: codes, then a stable sort, then tile boxes -- each against the plain entry point on the prefix."""
    be, B, n, lens = ops.backend(), 2, 20000, (20000, 4097)
    outs = []
    for filling in (0, 1):
        xyz, ld = padded_cloud(77, B, n, lens, filling), dev_lengths(lens)
        box = torch.stack([torch.cat([xyz[b, :ln].amin(0), xyz[b, :ln].amax(0)]) for b, ln in enumerate(lens)]).contiguous()
        codes = torch.full((B, n), -3, dtype=torch.int32, device=DEV)
        ops._call("mcp_morton_codes_lengths", xyz, B, n, _lib.fptr(xyz), _lib.fptr(box), _lib.iptr(ld), _lib.iptr(codes))
        s, perm, boxes = be._build_cloud(xyz, ld)
        outs.append((codes, perm, boxes))
        for b, ln in enumerate(lens):
            pre, t = xyz[b:b + 1, :ln].contiguous(), tiles_of(ln)
            want = torch.empty((1, ln), dtype=torch.int32, device=DEV)
            ops._call("mcp_morton_codes", pre, 1, ln, _lib.fptr(pre), _lib.fptr(box[b:b + 1].contiguous()), _lib.iptr(want))
            assert torch.equal(codes[b, :ln], want[0]) and bool((codes[b, ln:] == PAD_CODE).all()), (b, ln)
            assert bool((want < PAD_CODE).all())
            # the sorted form: a permutation of the prefix in ascending code order, ties in index order; the padding stays in place
            p = perm[b, :ln].long()
            assert torch.equal(p, torch.sort(want[0], stable=True)[1]) and torch.equal(s[b, :ln], xyz[b, p])
            assert torch.equal(perm[b, ln:], torch.arange(ln, n, dtype=torch.int32, device=DEV))
            sp = s[b:b + 1, :ln].contiguous()
            wboxes = torch.empty((1, t, 6), device=DEV)
            ops._call("mcp_tile_boxes", sp, 1, ln, _lib.fptr(sp), _lib.fptr(wboxes))
            assert torch.equal(boxes[b, :t], wboxes[0]) and not boxes[b, t:].any(), (b, ln)
    for a, o in zip(*outs):
        assert torch.equal(a, o), "the padding's contents reached a code, the permutation or a box"


# ---- the search, through the C entry point ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pruned(B, Q, N, K, mode, qlen, rlen, filling=0, null_lengths=False):
    """mcp_knn_pruned_lengths on clouds built under the same lengths; CPU copies of (idx, dist), pre-filled with a sentinel.
    null_lengths: both length arrays NULL (clouds built length-free), so the call lands in mcp_knn_pruned."""
    be = ops.backend()
    query, ref = (t.to(DEV) for t in padded_pair(B, Q, N, qlen, rlen, filling))
    ql, rl = (None, None) if null_lengths else (dev_lengths(qlen), dev_lengths(rlen))
    qs, qperm, _ = be._build_cloud(query, ql)
    rs, rperm, boxes = be._build_cloud(ref, rl)
    idx, dist = torch.full((B, Q, K), -7, dtype=torch.int32, device=DEV), torch.full((B, Q, K), -7.0, device=DEV)
    ops._call("mcp_knn_pruned_lengths", query, B, Q, N, K, mode, _lib.fptr(qs), _lib.iptr(qperm), _lib.fptr(rs), _lib.iptr(rperm),
              _lib.fptr(boxes), None if ql is None else _lib.iptr(ql), None if rl is None else _lib.iptr(rl), _lib.iptr(idx), _lib.fptr(dist))
    return idx.cpu(), dist.cpu()


def check(B, Q, N, K, mode, qlen, rlen):
    idx, dist = pruned(B, Q, N, K, mode, qlen, rlen)
    want_i, want_d = expected(B, Q, N, K, mode, qlen, rlen)
    for b in range(B):
        ql = qlen[b]
        assert torch.equal(idx[b, :ql], want_i[b, :ql]) and torch.equal(dist[b, :ql], want_d[b, :ql]), (b, ql, rlen[b])
        assert not idx[b, ql:].any() and not dist[b, ql:].any(), f"padded rows of element {b} are not zero"
    other = pruned(B, Q, N, K, mode, qlen, rlen, filling=1)
    assert torch.equal(idx, other[0]) and torch.equal(dist, other[1]), "the padding's contents reached an output bit"


FIRST = (3, 130, 200, (130, 64, 3), (200, 65, 1))   # a partial tile, a one-point set, rlen < K, a partial last wave, dead waves


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [1, 4, 16, 32])
def test_both_kernels_against_the_oracle(K, mode):
    B, Q, N, qlen, rlen = FIRST
    check(B, Q, N, K, mode, qlen, rlen)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [1, 16, 32])           # round 3's kernel in its K <= 4 and K <= 16 classes, the walk kernel
@pytest.mark.parametrize("N", [5000, 9000, 20000])   # 2, 4 and 16 tile bounds per lane; 20000 through the external sort
def test_every_tile_count_instantiation(N, K, mode):
    check(2, 130, N, K, mode, (130, 130), (N, N // 2 + 1))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [1, 16, 32])
@pytest.mark.parametrize("N", [5000, 9000, 20000])
def test_every_tile_count_instantiation_without_lengths(N, K, mode):
    """The same shapes with both length arrays NULL: the length-free kernels (mcp_knn_pruned), every row live, against the oracle."""
    B, Q = 2, 130
    idx, dist = pruned(B, Q, N, K, mode, (Q,) * B, (N,) * B, null_lengths=True)
    want_i, want_d = expected(B, Q, N, K, mode, (Q,) * B, (N,) * B)
    assert torch.equal(idx, want_i) and torch.equal(dist, want_d)


@pytest.mark.parametrize("K,mode", [(4, 1), (16, 0), (32, 1)])
def test_no_query_and_nothing_to_search(K, mode):
    check(2, 70, 100, K, mode, (0, 70), (100, 0))


@pytest.mark.parametrize("K", [4, 32])
def test_null_lengths_and_full_lengths_equal_the_plain_pruned_search(K):
    be, B, Q, N = ops.backend(), 2, 130, 300
    query, ref = cloud(51, B, Q).to(DEV), cloud(52, B, N).to(DEV)
    qs, qperm, _ = be._build_cloud(query)
    rs, rperm, boxes = be._build_cloud(ref)
    args = (_lib.fptr(qs), _lib.iptr(qperm), _lib.fptr(rs), _lib.iptr(rperm), _lib.fptr(boxes))
    want = torch.empty((B, Q, K), dtype=torch.int32, device=DEV), torch.empty((B, Q, K), device=DEV)
    ops._call("mcp_knn_pruned", query, B, Q, N, K, 1, *args, _lib.iptr(want[0]), _lib.fptr(want[1]))
    fq, fr = dev_lengths((Q,) * B), dev_lengths((N,) * B)
    for ql, rl in ((None, None), (fq, fr), (fq, None), (None, fr)):
        idx, dist = torch.full_like(want[0], -7), torch.full_like(want[1], -7.0)
        ops._call("mcp_knn_pruned_lengths", query, B, Q, N, K, 1, *args, None if ql is None else _lib.iptr(ql),
                  None if rl is None else _lib.iptr(rl), _lib.iptr(idx), _lib.fptr(dist))
        assert torch.equal(idx, want[0]) and torch.equal(dist, want[1]), (ql, rl)


# ---- routing and the public interface ---------------------------------------------------------------------------------------------
# the smallest shape that takes the pruned route (B = 2, Q = 1024, N = 2048 with lengths (1024, 513) / (2048, 1000) at the size
# rule's first constants; it follows the class attributes)
RB, RQ, RN = 2, ops.HipBackend.PRUNE_LENGTHS_MIN_QUERIES, ops.HipBackend.PRUNE_LENGTHS_MIN_REFS
RQLEN, RRLEN = (RQ, RQ // 2 + 1), (RN, RN * 125 // 256)


@pytest.fixture(scope="module")
def routed():
    query, ref = padded_pair(RB, RQ, RN, RQLEN, RRLEN)
    return query.to(DEV), ref.to(DEV), dev_lengths(RQLEN), dev_lengths(RRLEN)


@pytest.fixture
def calls(monkeypatch):
    names, real = [], ops._call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(ops, "_call", spy)
    return names


@pytest.mark.parametrize("K", [1, 32])
def test_knn_takes_the_pruned_route_and_equals_the_exhaustive_one(routed, calls, K):
    query, ref, ql, rl = routed
    be = ops.backend()
    want = be.knn_bruteforce(query, ref, K, mode=1, return_dist=True, query_lengths=ql, ref_lengths=rl)
    del calls[:]
    got = be.knn(query, ref, K, mode=1, return_dist=True, query_lengths=ql, ref_lengths=rl)
    assert "mcp_knn_pruned_lengths" in calls and "mcp_knn_lengths" not in calls, calls
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # one side without a length: that cloud is built length-free, and every query row is live (so: queries without padding)
    whole = cloud(1000 + RQ, RB, RQ).to(DEV)
    del calls[:]
    got = be.knn(whole, ref, K, mode=1, return_dist=True, ref_lengths=rl)
    want = be.knn_bruteforce(whole, ref, K, mode=1, return_dist=True, ref_lengths=rl)
    assert calls[:3] == ["mcp_build_cloud_lengths", "mcp_build_cloud", "mcp_knn_pruned_lengths"], calls
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_one_step_below_either_threshold_stays_exhaustive(routed, calls):
    query, ref, ql, rl = routed
    be = ops.backend()
    for q, r in ((query[:, :RQ - 1].contiguous(), ref), (query, ref[:, :RN - 1].contiguous())):
        del calls[:]
        be.knn(q, r, 1, mode=1, query_lengths=[RQLEN[1]] * RB, ref_lengths=[RRLEN[1]] * RB)
        assert calls == ["mcp_knn_lengths"], calls


def test_cloud_scope_builds_once_per_tensor_and_lengths_tensor(routed, calls):
    query, ref, ql, rl = routed
    be = ops.backend()
    builds = lambda: [c for c in calls if c.startswith("mcp_build_cloud")]
    with be.cloud_scope():
        a = be.knn(query, ref, 4, query_lengths=ql, ref_lengths=rl)
        assert builds() == ["mcp_build_cloud_lengths"] * 2
        b = be.knn(query, ref, 4, query_lengths=ql, ref_lengths=rl)
        assert builds() == ["mcp_build_cloud_lengths"] * 2 and torch.equal(a, b)            # both clouds served from the scope
        other = rl.clone()
        be.knn(query, ref, 4, query_lengths=ql, ref_lengths=other)
        assert builds() == ["mcp_build_cloud_lengths"] * 3                                   # the reference again, under `other`
        be.knn(query, ref, 4, query_lengths=ql)
        assert builds() == ["mcp_build_cloud_lengths"] * 3 + ["mcp_build_cloud"]             # ... and length-free
        be.knn(query, ref, 4)                                                                # the plain search: the query length-free too
        assert builds() == ["mcp_build_cloud_lengths"] * 3 + ["mcp_build_cloud"] * 2
    # a cloud searched in itself is one cloud only when the lengths are one object
    del calls[:]
    be.knn(ref, ref, 4, query_lengths=rl, ref_lengths=rl)
    assert builds() == ["mcp_build_cloud_lengths"]
    del calls[:]
    be.knn(ref, ref, 4, query_lengths=rl, ref_lengths=rl.clone())
    assert builds() == ["mcp_build_cloud_lengths"] * 2


def test_compat_knn_points_is_what_it_is_without_pruning(routed, calls, monkeypatch):
    query, ref, ql, rl = routed
    got = compat.knn_points(query, ref, lengths1=ql, lengths2=rl, K=4, return_nn=True)
    assert "mcp_knn_pruned_lengths" in calls
    monkeypatch.setattr(ops.HipBackend, "PRUNE_LENGTHS_MIN_REFS", 1 << 30)
    monkeypatch.setattr(ops.HipBackend, "PRUNE_LENGTHS_MIN_QUERIES", 1 << 30)
    del calls[:]
    want = compat.knn_points(query, ref, lengths1=ql, lengths2=rl, K=4, return_nn=True)
    assert "mcp_knn_pruned_lengths" not in calls and "mcp_knn_lengths" in calls
    for g, w in zip(got, want):
        assert torch.equal(g, w)


# ---- Chamfer ----------------------------------------------------------------------------------------------------------------------
# both directions qualify: x (2, 2048, 3) with lengths (2048, 1030), y (2, 3000, 3) with (3000, 1500) at the size rule's first constants
CB, CN = 2, max(ops.HipBackend.PRUNE_LENGTHS_MIN_QUERIES, ops.HipBackend.PRUNE_LENGTHS_MIN_REFS)
CM = CN * 375 // 256
CXLEN, CYLEN = (CN, CN * 515 // 1024), (CM, CM // 2)


def chamfer_results():
    """(no-grad value, differentiable value, d/dx, d/dy) on NaN-padded clouds."""
    x, y = cloud(61, CB, CN), cloud(62, CB, CM)
    for b in range(CB):
        x[b, CXLEN[b]:] = float("nan")
        y[b, CYLEN[b]:] = float("nan")
    be, xl, yl = ops.backend(), dev_lengths(CXLEN), dev_lengths(CYLEN)
    plain = be.chamfer(x.to(DEV), y.to(DEV), per_sample=True, x_lengths=xl, y_lengths=yl)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    v = be.chamfer(xd, yd, per_sample=True, x_lengths=xl, y_lengths=yl)
    gx, gy = torch.autograd.grad(v.mean(), [xd, yd])
    return plain, v.detach(), gx, gy


def test_chamfer_takes_the_pruned_route_with_the_same_bits(calls, monkeypatch):
    got = chamfer_results()
    assert calls.count("mcp_knn_pruned_lengths") == 4 and "mcp_knn_lengths" not in calls and "mcp_chamfer_nn_lengths" not in calls, calls
    assert calls.count("mcp_build_cloud_lengths") == 4, calls   # each cloud once per chamfer call, for its two roles
    monkeypatch.setattr(ops.HipBackend, "PRUNE_LENGTHS_MIN_REFS", 1 << 30)
    monkeypatch.setattr(ops.HipBackend, "PRUNE_LENGTHS_MIN_QUERIES", 1 << 30)
    del calls[:]
    want = chamfer_results()
    assert "mcp_knn_pruned_lengths" not in calls and "mcp_chamfer_nn_lengths" in calls, calls
    for name, g, w in zip(("value", "differentiable value", "d/dx", "d/dy"), got, want):
        assert torch.equal(g, w), name
    assert bool(torch.isfinite(got[0]).all())
    for b in range(CB):
        assert not got[2][b, CXLEN[b]:].any() and not got[3][b, CYLEN[b]:].any(), "gradient rows beyond a length are not exact zeros"
        assert bool(got[2][b, :CXLEN[b]].any()) and bool(got[3][b, :CYLEN[b]].any())
