"""The length-aware exhaustive KNN search (mcp_knn_lengths, csrc/knn.hip) against the CPU oracle run on every element's
valid prefixes on their own.  The padding is hostile: padded reference rows are copies of live query points (an unmasked kernel
returns them at distance 0) and padded query rows hold 1e30; a second filling (NaN / -5e29) must not move a single output bit."""
import ctypes
import functools

import pytest
import torch

from mocopci_amd import _lib, compat, ops
from oracle import pointset as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cloud(seed, b, n, dup=0.05, extent=(40.0, 40.0, 3.0)):
    """tests/test_ops_gpu.py's cloud(): uniform points with 5 % exact duplicates, so the (distance, index) tie rule decides."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(b, n, 3, generator=g) * 2 - 1) * torch.tensor(extent)
    nd = int(n * dup)
    if nd:
        src = torch.randint(0, n - nd, (nd,), generator=g)
        x[:, n - nd:] = x[:, src]
        x = x[:, torch.randperm(n, generator=g)]
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def padded_pair(B, Q, N, qlen, rlen, filling=0):
    """(query (B,Q,3), ref (B,N,3)) whose rows beyond qlen[b] / rlen[b] are padding.  filling 0: padded references are copies of
    live query points, padded queries 1e30.  filling 1: padded references -5e29, padded queries NaN.  Live rows do not depend on it."""
    query, ref = cloud(1000 + Q, B, Q), cloud(2000 + N, B, N)
    for b in range(B):
        ql, rl = qlen[b], rlen[b]
        if filling == 0:
            ref[b, rl:] = query[b, torch.arange(N - rl) % ql] if ql else 0.0
            query[b, ql:] = 1e30
        else:
            ref[b, rl:] = -5e29
            query[b, ql:] = float("nan")
    return query, ref


@functools.lru_cache(maxsize=None)
def expected(B, Q, N, K, mode, qlen, rlen):
    """The oracle on each element's prefixes; zeros in padded rows and where there is nothing to search."""
    query, ref = padded_pair(B, Q, N, qlen, rlen)
    idx, dist = torch.zeros(B, Q, K, dtype=torch.int32), torch.zeros(B, Q, K)
    for b in range(B):
        ql, rl = qlen[b], rlen[b]
        if ql and rl:
            idx[b, :ql], dist[b, :ql] = (t[0] for t in orc.knn(query[b:b + 1, :ql], ref[b:b + 1, :rl], K, mode, return_dist=True))
    return idx, dist


def search(B, Q, N, K, mode, qlen, rlen, filling=0, as_lengths=list):
    query, ref = padded_pair(B, Q, N, qlen, rlen, filling)
    idx, dist = ops.backend().knn(query.to(DEV), ref.to(DEV), K, mode=mode, return_dist=True, query_lengths=as_lengths(qlen),
                                  ref_lengths=as_lengths(rlen))
    assert idx.dtype == torch.int32 and idx.shape == dist.shape == (B, Q, K)
    return idx.cpu(), dist.cpu()


def check(B, Q, N, K, mode, qlen, rlen):
    idx, dist = search(B, Q, N, K, mode, qlen, rlen)
    want_i, want_d = expected(B, Q, N, K, mode, qlen, rlen)
    for b in range(B):
        ql = qlen[b]
        assert torch.equal(idx[b, :ql], want_i[b, :ql]) and torch.equal(dist[b, :ql], want_d[b, :ql]), (b, ql, rlen[b])
        assert not idx[b, ql:].any() and not dist[b, ql:].any(), f"padded rows of element {b} are not zero"


FIRST = (3, 130, 200, (130, 64, 3), (200, 65, 1))   # 4 waves per workgroup; a partial tile, a one-point set, rlen < K


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [1, 4, 16, 32])
def test_every_selection_family(K, mode):
    B, Q, N, qlen, rlen = FIRST
    check(B, Q, N, K, mode, qlen, rlen)


@pytest.mark.parametrize("B,Q,N,K,mode,qlen,rlen", [
    (1, 64, 1024, 32, 0, (64,), (70,)),              # 8 waves per workgroup, six of them own no reference
    (1, 64, 1024, 32, 0, (64,), (5,)),               # ... seven of them
    (1, 64, 1024, 3, 1, (64,), (5,)),                # the same through the register list's merge
    (2, 64, 1024, 16, 1, (1, 64), (1024, 129)),      # full and short elements in one launch
    (1, 64, 70000, 1, 1, (40,), (66000,)),           # a reference set beyond 65536
    (2, 100, 60, 4, 1, (100, 10), (60, 33)),         # one wave per workgroup, one tile
    (2, 100, 60, 16, 0, (100, 10), (60, 33)),
    (2, 70, 150, 32, 1, (70, 65), (150, 64)),        # two waves per workgroup; the second one's slice is empty at rlen = 64
    (2, 70, 100, 4, 1, (0, 70), (100, 0)),           # no query at all / nothing to search
    (2, 70, 100, 16, 0, (0, 70), (100, 0)),
])
def test_split_slices_and_edges(B, Q, N, K, mode, qlen, rlen):
    check(B, Q, N, K, mode, qlen, rlen)


def test_without_lengths_and_with_full_lengths_equal_the_plain_search():
    be = ops.backend()
    query, ref = cloud(7, 2, 70).to(DEV), cloud(8, 2, 300).to(DEV)
    want_i, want_d = be.knn_bruteforce(query, ref, 7, mode=1, return_dist=True)
    for ql, rl in ((None, None), ([70, 70], [300, 300]), ([70, 70], None), (None, [300, 300])):
        idx, dist = be.knn(query, ref, 7, mode=1, return_dist=True, query_lengths=ql, ref_lengths=rl)
        assert torch.equal(idx, want_i) and torch.equal(dist, want_d), (ql, rl)
    assert torch.equal(be.knn(query, ref, 7, mode=1, query_lengths=[70, 70], ref_lengths=[300, 300]), want_i)   # indices only


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [1, 4, 16, 32])
def test_padding_contents_reach_no_output_bit(K, mode):
    B, Q, N, qlen, rlen = FIRST
    a, b = search(B, Q, N, K, mode, qlen, rlen), search(B, Q, N, K, mode, qlen, rlen, filling=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_device_tensor_lengths(dtype):
    B, Q, N, qlen, rlen = FIRST
    a = search(B, Q, N, 16, 1, qlen, rlen)
    b = search(B, Q, N, 16, 1, qlen, rlen, as_lengths=lambda v: torch.tensor(v, dtype=dtype, device=DEV))
    c = search(B, Q, N, 16, 1, qlen, rlen, as_lengths=lambda v: torch.tensor(v, dtype=dtype))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_device_lengths_are_clamped_by_the_kernel():
    """A device tensor is trusted by the host: the kernel clamps it to [0, Q] / [0, N]."""
    B, Q, N = 2, 70, 100
    query, ref = cloud(11, B, Q).to(DEV), cloud(12, B, N).to(DEV)
    be = ops.backend()
    want = be.knn(query, ref, 4, return_dist=True, query_lengths=[Q, 0], ref_lengths=[N, 0])
    got = be.knn(query, ref, 4, return_dist=True, query_lengths=torch.tensor([Q + 1000, -3], device=DEV),
                 ref_lengths=torch.tensor([2 ** 31 - 1, -1], dtype=torch.int32, device=DEV))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[0][0], be.knn_bruteforce(query[:1], ref[:1], 4)[0]) and not got[0][1].any()


def test_abi_contract():
    """k = 33 is MCP_ERR_UNSUPPORTED, a null idx MCP_ERR_BAD_ARG, and neither launches anything: the sentinel survives."""
    lib = _lib.load()
    query, ref = cloud(21, 1, 64).to(DEV), cloud(22, 1, 128).to(DEV)
    lens = torch.tensor([64], dtype=torch.int32, device=DEV)
    idx = torch.full((1, 64, 33), -77, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = (query.data_ptr(), ref.data_ptr(), lens.data_ptr(), lens.data_ptr())
    assert lib.mcp_knn_lengths(1, 64, 128, 33, 1, *args, idx.data_ptr(), None, stream) == 10002
    assert lib.mcp_knn_lengths(1, 64, 128, 4, 1, *args, None, None, stream) == 10001
    assert lib.mcp_knn_lengths(1, 64, 128, 33, 1, query.data_ptr(), ref.data_ptr(), None, None, idx.data_ptr(), None, stream) == 10002
    torch.cuda.synchronize()
    assert bool((idx == -77).all())
    with pytest.raises(RuntimeError):   # host lengths are validated before the call
        ops.backend().knn(query, ref, 4, ref_lengths=[129])


def test_chamfer_nn_lengths_entry_point():
    """mcp_chamfer_nn_lengths: squared nearest distances over the valid prefixes both ways, zeros in padded rows."""
    B, N, M, xlen, ylen = 3, 130, 200, (130, 64, 3), (200, 65, 1)
    x, y = padded_pair(B, N, M, xlen, ylen)
    xd, yd = x.to(DEV), y.to(DEV)
    xl, yl = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in (xlen, ylen))
    dxy, dyx = torch.full((B, N), -1.0, device=DEV), torch.full((B, M), -1.0, device=DEV)
    rc = _lib.load().mcp_chamfer_nn_lengths(B, N, M, xd.data_ptr(), yd.data_ptr(), xl.data_ptr(), yl.data_ptr(), dxy.data_ptr(), dyx.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(dxy.cpu(), expected(B, N, M, 1, 1, xlen, ylen)[1][..., 0])
    for b in range(B):
        want = orc.knn(y[b:b + 1, :ylen[b]], x[b:b + 1, :xlen[b]], 1, 1, return_dist=True)[1][0, :, 0]
        assert torch.equal(dyx[b, :ylen[b]].cpu(), want) and not dyx[b, ylen[b]:].any()


def test_compat_knn_points():
    B, P1, P2, K, l1, l2 = 3, 130, 200, 4, (130, 64, 3), (200, 65, 1)
    p1, p2 = padded_pair(B, P1, P2, l1, l2)
    p1d, p2d = p1.to(DEV), p2.to(DEV)
    d, i, nn = compat.knn_points(p1d, p2d, lengths1=torch.tensor(l1), lengths2=torch.tensor(l2), K=K, return_nn=True, return_sorted=True)
    assert i.dtype == torch.int64 and i.shape == d.shape == (B, P1, K) and nn.shape == (B, P1, K, 3)
    want_i, want_d = expected(B, P1, P2, K, 1, l1, l2)
    for b in range(B):
        live = min(K, l2[b])
        assert torch.equal(i[b, :l1[b], :live].cpu().int(), want_i[b, :l1[b], :live]) and torch.equal(d[b, :l1[b], :live].cpu(), want_d[b, :l1[b], :live])
        assert not i[b, :, live:].any() and not d[b, :, live:].any()     # pytorch3d's zero padding at k >= lengths2[b] ...
        assert not i[b, l1[b]:].any() and not d[b, l1[b]:].any()         # ... and in rows >= lengths1[b]
    assert torch.equal(nn.cpu(), orc.group_rows(p2, i.cpu().int()))
    # the call of tests/test_ops_gpu.py::test_compat_helpers_keep_reference_signatures is what it was
    xyz, new_xyz = cloud(95, 2, 700).to(DEV), cloud(96, 2, 300).to(DEV)
    d, i, none = compat.knn_points(new_xyz, xyz, K=4)
    wi, wd = orc.knn(new_xyz.cpu(), xyz.cpu(), 4, mode=1, return_dist=True)
    assert none is None and torch.equal(i.cpu().int(), wi) and torch.equal(d.cpu(), wd)
    d2, i2, nn2 = compat.knn_points(new_xyz, xyz, K=4, return_nn=True)
    assert torch.equal(i2, i) and torch.equal(d2, d) and torch.equal(nn2.cpu(), orc.group_rows(xyz.cpu(), wi))
