"""The length-aware feature-cosine KNN search (mcp_knn_cosine_lengths, csrc/knn_cosine.hip) against the CPU oracle run on every
element's valid prefixes on their own, bit for bit.  The padding is hostile: padded reference rows are copies of live query rows
of the same element (an unmasked kernel returns them at distance ~ 0) and padded query rows hold 1e30; a second filling (NaN /
-5e29) must not move a single output bit.  The shapes are the smallest that reach each split of the reference range (2, 4 or 8
waves per workgroup, picked from the padded sizes) and each edge of a length against the 32-row tiles and 32-query workgroups."""
import functools

import pytest
import torch

from mocopci_amd import _lib, compat, ops
from oracle import pointset as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def padded_pair(B, Q, N, C, qlen, rlen, filling=0):
    """(qfeat (B,Q,C), rfeat (B,N,C)), torch.randn, whose rows beyond qlen[b] / rlen[b] are padding; the live references end in a few
    exact copies of earlier live rows, so the (distance, index) tie rule decides.  filling 0: padded references are copies of live
    query rows, padded queries 1e30.  filling 1: padded references -5e29, padded queries NaN.  Live rows do not depend on it."""
    g = torch.Generator().manual_seed(1000 * C + 10 * Q + N)
    qf, rf = torch.randn(B, Q, C, generator=g), torch.randn(B, N, C, generator=g)
    for b in range(B):
        ql, rl = qlen[b], rlen[b]
        nd = min(rl // 2, 1 + rl // 16)
        if nd:
            rf[b, rl - nd:rl] = rf[b, torch.randint(0, rl - nd, (nd,), generator=g)]
        if filling == 0:
            rf[b, rl:] = qf[b, torch.arange(N - rl) % ql] if ql else 0.0
            qf[b, ql:] = 1e30
        else:
            rf[b, rl:] = -5e29
            qf[b, ql:] = float("nan")
    return qf, rf


@functools.lru_cache(maxsize=None)
def expected(B, Q, N, C, K, qlen, rlen):
    """The oracle on each element's prefixes with min(K, rlen) neighbours, the last entry repeated up to K; zeros in padded rows and
    where there is nothing to search."""
    qf, rf = padded_pair(B, Q, N, C, qlen, rlen)
    idx, dist = torch.zeros(B, Q, K, dtype=torch.int32), torch.zeros(B, Q, K)
    for b in range(B):
        ql, rl = qlen[b], rlen[b]
        if ql and rl:
            kk = min(K, rl)
            i, d = (t[0] for t in orc.knn_cosine(qf[b:b + 1, :ql], rf[b:b + 1, :rl], kk, return_dist=True))
            idx[b, :ql, :kk], dist[b, :ql, :kk] = i, d
            idx[b, :ql, kk:], dist[b, :ql, kk:] = i[:, -1:], d[:, -1:]
    return idx, dist


def search(B, Q, N, C, K, qlen, rlen, filling=0, as_lengths=list):
    qf, rf = padded_pair(B, Q, N, C, qlen, rlen, filling)
    idx, dist = ops.backend().knn_cosine(qf.to(DEV), rf.to(DEV), K, return_dist=True, query_lengths=as_lengths(qlen),
                                         ref_lengths=as_lengths(rlen))
    assert idx.dtype == torch.int32 and idx.shape == dist.shape == (B, Q, K)
    return idx.cpu(), dist.cpu()


def check(B, Q, N, C, K, qlen, rlen):
    idx, dist = search(B, Q, N, C, K, qlen, rlen)
    want_i, want_d = expected(B, Q, N, C, K, qlen, rlen)
    for b in range(B):
        ql = qlen[b]
        assert torch.equal(idx[b, :ql], want_i[b, :ql]) and torch.equal(dist[b, :ql], want_d[b, :ql]), (b, ql, rlen[b])
        assert not idx[b, ql:].any() and not dist[b, ql:].any(), f"padded rows of element {b} are not zero"


# B, Q, N, C, qlen, rlen (K apart).  Waves per workgroup from the padded sizes: 2 when ceil(N/32) < 4 or 2 * B * ceil(Q/32) >= 2048,
# 4 when ceil(N/32) < 8, 8 otherwise.
FIRST = (3, 130, 200, 64, (130, 64, 3), (200, 65, 1))     # 4 waves; a partial tile; a wave without a tile at 65; rlen < K
SECOND = (2, 70, 300, 128, (70, 33), (300, 31))           # 8 waves, seven of them without a tile in element 1; a query block cut at 33
THIRD = (1, 40, 520, 256, (40,), (257,))                  # 8 waves with the queries in LDS; wave 0 owns two tiles and the others one
FOURTH = (2, 100, 60, (100, 10), (60, 33))                # 2 waves; one or two tiles; three whole query blocks padded in element 1 (C apart)
EMPTY = (2, 70, 100, (0, 70), (100, 0))                   # no query at all / nothing to search (C apart)
LARGE = (8, 4096, 200, 64, (4096, 1, 0, 33, 4095, 64, 2048, 100), (200, 200, 200, 16, 1, 129, 64, 0))   # 2 waves with seven tiles


@pytest.mark.parametrize("K", [1, 5, 16])
def test_partial_tile_idle_wave_and_fewer_references_than_k(K):
    B, Q, N, C, qlen, rlen = FIRST
    check(B, Q, N, C, K, qlen, rlen)


def test_eight_waves_seven_of_them_without_a_tile():
    B, Q, N, C, qlen, rlen = SECOND
    check(B, Q, N, C, 16, qlen, rlen)


def test_queries_in_lds_with_uneven_tile_ownership():
    B, Q, N, C, qlen, rlen = THIRD
    check(B, Q, N, C, 16, qlen, rlen)


@pytest.mark.parametrize("C", [64, 128, 256])
def test_two_waves_and_wholly_padded_query_blocks(C):
    B, Q, N, qlen, rlen = FOURTH
    check(B, Q, N, C, 16, qlen, rlen)


@pytest.mark.parametrize("C", [64, 256])
def test_no_query_and_nothing_to_search(C):
    B, Q, N, qlen, rlen = EMPTY
    check(B, Q, N, C, 4, qlen, rlen)


@pytest.mark.parametrize("rl", [32, 33, 64, 96])
def test_lengths_on_and_next_to_tile_boundaries(rl):
    check(1, 64, 128, 64, 16, (64,), (rl,))


def test_long_and_short_elements_in_one_launch():
    B, Q, N, C, qlen, rlen = LARGE
    check(B, Q, N, C, 16, qlen, rlen)


@pytest.mark.parametrize("case,K", [(FIRST, 5), (FOURTH[:3] + (256,) + FOURTH[3:], 16), (EMPTY[:3] + (64,) + EMPTY[3:], 4)])
def test_padded_rows_are_written_as_zeros_over_a_sentinel(case, K):
    """Through the C ABI, so that the outputs can be pre-filled: every row of idx and dist is written, padded ones with zeros."""
    B, Q, N, C, qlen, rlen = case
    qf, rf = (t.to(DEV) for t in padded_pair(B, Q, N, C, qlen, rlen))
    ql, rl = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in (qlen, rlen))
    idx = torch.full((B, Q, K), -77, dtype=torch.int32, device=DEV)
    dist = torch.full((B, Q, K), -7.0, device=DEV)
    ws = torch.full((B * (Q + N) * C,), 123.0, device=DEV)
    rc = _lib.load().mcp_knn_cosine_lengths(B, Q, N, C, K, qf.data_ptr(), rf.data_ptr(), ql.data_ptr(), rl.data_ptr(), idx.data_ptr(),
                                            dist.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    want_i, want_d = expected(B, Q, N, C, K, qlen, rlen)
    assert torch.equal(idx.cpu(), want_i) and torch.equal(dist.cpu(), want_d)
    # the workspace: live rows hold unit vectors, the rows of padding were not written
    nq, nr = ws[:B * Q * C].view(B, Q, C).cpu(), ws[B * Q * C:].view(B, N, C).cpu()
    for b in range(B):
        assert bool((nq[b, qlen[b]:] == 123.0).all()) and bool((nr[b, rlen[b]:] == 123.0).all()), f"padded workspace rows of element {b} were written"
        assert bool((nq[b, :qlen[b]].abs() <= 1.0).all()) and bool((nr[b, :rlen[b]].abs() <= 1.0).all())
    # without a dist output (NULL) the indices are the same
    idx2 = torch.full((B, Q, K), -77, dtype=torch.int32, device=DEV)
    rc = _lib.load().mcp_knn_cosine_lengths(B, Q, N, C, K, qf.data_ptr(), rf.data_ptr(), ql.data_ptr(), rl.data_ptr(), idx2.data_ptr(),
                                            None, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(idx2.cpu(), want_i)


@pytest.mark.parametrize("case,K", [(FIRST, 1), (FIRST, 5), (FIRST, 16), (SECOND, 16), (FOURTH[:3] + (64,) + FOURTH[3:], 16),
                                    (FOURTH[:3] + (128,) + FOURTH[3:], 16), (FOURTH[:3] + (256,) + FOURTH[3:], 16)])
def test_padding_contents_reach_no_output_bit(case, K):
    B, Q, N, C, qlen, rlen = case
    a, b = search(B, Q, N, C, K, qlen, rlen), search(B, Q, N, C, K, qlen, rlen, filling=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_without_lengths_and_with_full_lengths_equal_the_plain_search():
    be = ops.backend()
    g = torch.Generator().manual_seed(7)
    qf, rf = torch.randn(2, 70, 64, generator=g).to(DEV), torch.randn(2, 300, 64, generator=g).to(DEV)
    want_i, want_d = be.knn_cosine(qf, rf, 7, return_dist=True)
    assert torch.equal(want_i.cpu(), orc.knn_cosine(qf.cpu(), rf.cpu(), 7))
    for ql, rl in ((None, None), ([70, 70], [300, 300]), ([70, 70], None), (None, [300, 300])):
        idx, dist = be.knn_cosine(qf, rf, 7, return_dist=True, query_lengths=ql, ref_lengths=rl)
        assert torch.equal(idx, want_i) and torch.equal(dist, want_d), (ql, rl)
    B, Q, N, C, qlen, rlen = FIRST   # indices only
    qp, rp = (t.to(DEV) for t in padded_pair(B, Q, N, C, qlen, rlen))
    assert torch.equal(be.knn_cosine(qp, rp, 16, query_lengths=list(qlen), ref_lengths=list(rlen)).cpu(), search(B, Q, N, C, 16, qlen, rlen)[0])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_list_cpu_tensor_and_device_tensor_lengths(dtype):
    B, Q, N, C, qlen, rlen = FIRST
    a = search(B, Q, N, C, 16, qlen, rlen)
    b = search(B, Q, N, C, 16, qlen, rlen, as_lengths=lambda v: torch.tensor(v, dtype=dtype, device=DEV))
    c = search(B, Q, N, C, 16, qlen, rlen, as_lengths=lambda v: torch.tensor(v, dtype=dtype))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_device_lengths_are_clamped_by_the_kernel():
    """A device tensor is trusted by the host: the kernels clamp it to [0, Q] / [0, N]."""
    B, Q, N = 2, 70, 100
    g = torch.Generator().manual_seed(11)
    qf, rf = torch.randn(B, Q, 64, generator=g).to(DEV), torch.randn(B, N, 64, generator=g).to(DEV)
    be = ops.backend()
    want = be.knn_cosine(qf, rf, 4, return_dist=True, query_lengths=[Q, 0], ref_lengths=[N, 0])
    got = be.knn_cosine(qf, rf, 4, return_dist=True, query_lengths=torch.tensor([Q + 1000, -3], device=DEV),
                        ref_lengths=torch.tensor([2 ** 31 - 1, -1], dtype=torch.int32, device=DEV))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[0][0], be.knn_cosine(qf[:1], rf[:1], 4)[0]) and not got[0][1].any()


def test_abi_contract():
    """k = 17 and c = 48 are MCP_ERR_UNSUPPORTED, a null idx MCP_ERR_BAD_ARG, and none launches anything: the sentinel survives."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(21)
    qf, rf = torch.randn(1, 64, 64, generator=g).to(DEV), torch.randn(1, 128, 64, generator=g).to(DEV)
    lens = torch.tensor([64], dtype=torch.int32, device=DEV)
    idx = torch.full((1, 64, 17), -77, dtype=torch.int32, device=DEV)
    ws = torch.empty((64 + 128) * 64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for ql, rl in ((lens.data_ptr(), lens.data_ptr()), (None, None)):
        assert lib.mcp_knn_cosine_lengths(1, 64, 128, 64, 17, qf.data_ptr(), rf.data_ptr(), ql, rl, idx.data_ptr(), None, ws.data_ptr(), stream) == 10002
        assert lib.mcp_knn_cosine_lengths(1, 64, 128, 48, 4, qf.data_ptr(), rf.data_ptr(), ql, rl, idx.data_ptr(), None, ws.data_ptr(), stream) == 10002
        assert lib.mcp_knn_cosine_lengths(1, 64, 128, 64, 4, qf.data_ptr(), rf.data_ptr(), ql, rl, None, None, ws.data_ptr(), stream) == 10001
    torch.cuda.synchronize()
    assert bool((idx == -77).all())
    with pytest.raises(RuntimeError):   # host lengths are validated before the call
        ops.backend().knn_cosine(qf, rf, 4, ref_lengths=[129])


def test_compat_knn_point_cosine():
    B, Q, N, C, qlen, rlen = FIRST
    qf, rf = (t.to(DEV) for t in padded_pair(B, Q, N, C, qlen, rlen))
    i = compat.knn_point_cosine(16, rf, qf, lengths=torch.tensor(rlen), new_lengths=torch.tensor(qlen))
    assert i.dtype == torch.int64 and i.shape == (B, Q, 16)
    want_i = expected(B, Q, N, C, 16, qlen, rlen)[0]
    for b in range(B):
        assert torch.equal(i[b, :qlen[b]].cpu().int(), want_i[b, :qlen[b]])
    # the three-argument call is the plain search
    g = torch.Generator().manual_seed(95)
    xyz, new_xyz = torch.randn(2, 300, 64, generator=g), torch.randn(2, 70, 64, generator=g)
    assert torch.equal(compat.knn_point_cosine(8, xyz.to(DEV), new_xyz.to(DEV)).cpu().int(), orc.knn_cosine(new_xyz, xyz, 8))
