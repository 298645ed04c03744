"""The pruned forms of the length-aware furthest point sampling (fps_len_spatial_kernel, fps_len_tiled_kernel: csrc/fps_pruned.h
under FPS_LEN 1) against the CPU oracle run on every element's valid prefix alone, with exact equality, one case per code path of
the two kernels.  The padding is NaN in one filling and 1e30 in another: a kernel that reads it selects it or poisons its
distances.  Every case also asks the unpruned entry point (the resident / streaming forms) for the same bits, checks the sampled
coordinates against a gather of the indices, and names the form the dispatch rule takes for its shape, so a case cannot pass on
another kernel than the one it is about.  The clouds are those of tests/test_fps_lengths_gpu.py (its builders, by import)."""
import functools

import pytest
import torch

import tests.test_fps_lengths_gpu as base
from mocopci_amd import _lib, ops
from oracle import pointset as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESIDENT, SPATIAL, TILED, STREAMING = 0, 1, 2, 3
UNSUPPORTED = 10002


@functools.lru_cache(maxsize=None)
def case(name):
    """(live points (B,n,3), lengths, m, the form the pruned entry point takes with its own workspace figure)"""
    def rows(pts, lens):
        return pts[None].repeat(len(lens), 1, 1).contiguous()
    if name == "spatial_p4_ties":     # 1: P = 4 on the tie-heavy cloud, every length class around the wave / slice / block edges
        lens = (2100, 2049, 2048, 1025, 1024, 1023, 513, 130, 65, 63, 5, 1, 0)
        return rows(base.tie_cloud(2100), lens), lens, 48, SPATIAL
    if name == "spatial_p2":          # 2: P = 2
        return base.cloud(41, 4, 2048), (2048, 1025, 64, 1), 64, SPATIAL
    if name == "spatial_n1024":       # 2: the smallest n of the spatial form
        return base.cloud(42, 2, 1024), (1024, 1), 64, SPATIAL
    if name == "spatial_p8":          # 3: P = 8
        return base.cloud(43, 3, 8192), (8192, 4097, 100), 64, SPATIAL
    if name == "spatial_p16":         # 4: P = 16, the coordinates stay in global memory (LDS_XYZ = false)
        return base.cloud(5, 4, 16384), (16384, 8193, 4097, 1), 64, SPATIAL
    if name == "spatial_no_lds_idx":  # 5: 512 + 12 n + 4 m > 160 KB: the index list goes straight to global memory (lds_idx == 0)
        return base.cloud(44, 2, 13000), (13000, 6000), 2048, SPATIAL
    if name == "tiled_smallest":      # 6: one point in the last tile
        return base.cloud(45, 3, 16385), (16385, 16384, 1), 32, TILED
    if name == "tiled":               # 7
        return base.cloud(6, 6, 20000), (20000, 16385, 16384, 100, 1, 0), 32, TILED
    if name == "tiled_largest":       # 8: the upper n limit
        return base.cloud(46, 2, 65536), (65536, 40000), 64, TILED
    raise KeyError(name)


CASES = ("spatial_p4_ties", "spatial_p2", "spatial_n1024", "spatial_p8", "spatial_p16", "spatial_no_lds_idx", "tiled_smallest", "tiled",
         "tiled_largest")


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle on each element's prefix alone; an all-zero row for the empty element."""
    pts, lens, m, _ = case(name)
    idx = torch.zeros(len(lens), m, dtype=torch.int32)
    for b, l in enumerate(lens):
        if l:
            idx[b] = orc.furthest_point_sample(pts[b:b + 1, :l].contiguous(), m)[0]
    return idx


def filled(pts, lens, filling):
    pts = pts.clone()
    for b, l in enumerate(lens):
        pts[b, l:] = base.FILLINGS[filling]
    return pts


def call(entry, xyz, lens, m, workspace_bytes=None):
    """One call of `entry` on device tensors: (rc, indices, coordinates).  workspace_bytes None: what the entry's own query asks for."""
    lib = _lib.load()
    B, n = xyz.shape[0], xyz.shape[1]
    if workspace_bytes is None:
        query = lib.mcp_fps_lengths_workspace_bytes if entry.endswith("_unpruned") else lib.mcp_fps_lengths_pruned_workspace_bytes
        workspace_bytes = query(B, n, m)
    ws = torch.empty(workspace_bytes, dtype=torch.uint8, device=DEV) if workspace_bytes else None
    idx = torch.full((B, m), -77, dtype=torch.int32, device=DEV)
    pts = torch.full((B, m, 3), float("nan"), dtype=torch.float32, device=DEV)
    lens_d = lens if torch.is_tensor(lens) else torch.tensor(lens, dtype=torch.int32, device=DEV)
    rc = getattr(lib, entry)(B, n, m, xyz.data_ptr(), lens_d.data_ptr(), idx.data_ptr(), pts.data_ptr(), ws.data_ptr() if ws is not None else None,
                             workspace_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, idx.cpu(), pts.cpu()


PRUNED, UNPRUNED = "mcp_furthest_point_sampling_lengths", "mcp_furthest_point_sampling_lengths_unpruned"


@pytest.mark.parametrize("filling", ["nan", "big"])
@pytest.mark.parametrize("name", CASES)
def test_pruned_forms_equal_the_oracle_on_the_prefixes(name, filling):
    live, lens, m, form = case(name)
    B, n = live.shape[0], live.shape[1]
    lib = _lib.load()
    assert lib.mcp_fps_lengths_form(B, n, m, lib.mcp_fps_lengths_pruned_workspace_bytes(B, n, m)) == form
    xyz = filled(live, lens, filling).to(DEV)
    rc, idx, pts = call(PRUNED, xyz, lens, m)
    assert rc == 0
    want = expected(name)
    for b, l in enumerate(lens):
        assert torch.equal(idx[b], want[b]), (name, filling, b, l, int((idx[b] != want[b]).sum()))
    rc_u, idx_u, pts_u = call(UNPRUNED, xyz, lens, m)
    assert rc_u == 0 and torch.equal(idx_u, idx) and torch.equal(pts_u, pts)         # the same bits from the unpruned forms
    gather = base.gathered(live, want)
    for b, l in enumerate(lens):
        if l:
            assert torch.equal(pts[b], gather[b]), (name, b, l)
        else:
            assert not idx[b].any() and not pts[b].any() and not torch.isnan(pts[b]).any()


@pytest.mark.parametrize("filling", ["nan", "big"])
def test_exactly_the_streaming_workspace_still_streams(filling):
    """7, second run: with b*n*4 bytes the call keeps the streaming form and its bits; with less, nothing is launched."""
    live, lens, m, _ = case("tiled")
    B, n = live.shape[0], live.shape[1]
    lib = _lib.load()
    assert lib.mcp_fps_lengths_form(B, n, m, B * n * 4) == STREAMING
    xyz = filled(live, lens, filling).to(DEV)
    rc, idx, pts = call(PRUNED, xyz, lens, m, workspace_bytes=B * n * 4)
    assert rc == 0 and torch.equal(idx, expected("tiled"))
    rc_t, idx_t, pts_t = call(PRUNED, xyz, lens, m)
    assert rc_t == 0 and torch.equal(idx_t, idx) and torch.equal(pts_t, pts)
    rc, idx, _ = call(PRUNED, xyz, lens, m, workspace_bytes=B * n * 4 - 1)
    assert rc == UNSUPPORTED and bool((idx == -77).all())


def test_tiled_form_with_the_index_list_in_global_memory():
    """9: m = 40000 does not fit beside the candidates in LDS (lds_idx == 0).  Against the unpruned entry point only."""
    n, m, lens = 65536, 40000, (65536, 100)
    live = base.cloud(47, 2, n)
    lib = _lib.load()
    assert 512 + (n // 64) * 16 + 4 * m > 160 * 1024
    assert lib.mcp_fps_lengths_form(2, n, m, lib.mcp_fps_lengths_pruned_workspace_bytes(2, n, m)) == TILED
    xyz = filled(live, lens, "nan").to(DEV)
    rc, idx, pts = call(PRUNED, xyz, lens, m)
    rc_u, idx_u, pts_u = call(UNPRUNED, xyz, lens, m)
    assert rc == 0 and rc_u == 0
    assert torch.equal(idx, idx_u) and torch.equal(pts, pts_u)
    assert int(idx[1].max()) < 100 and int(idx.min()) == 0 and len(set(idx[0].tolist())) == m     # m distinct points of the full element
    assert torch.equal(pts, base.gathered(live, idx))


@pytest.mark.parametrize("n", [1024, 4096, 20000])
def test_full_lengths_equal_the_length_free_call(n):
    """10: every len[b] == n: indices and coordinates are the length-free call's, bit for bit."""
    be = ops.backend()
    xyz = base.cloud(50 + n, 2, n).to(DEV)
    m = 128
    want_i, want_p = be.fps(xyz, m, with_points=True)
    rc, idx, pts = call(PRUNED, xyz, (n, n), m)
    assert rc == 0 and torch.equal(idx, want_i.cpu()) and torch.equal(pts, want_p.cpu())
    got_i, got_p = be.fps(xyz, m, with_points=True, lengths=[n, n])              # the backend sizes the workspace for the pruned form
    assert torch.equal(got_i, want_i) and torch.equal(got_p, want_p)
    assert torch.equal(be.fps(xyz, m, lengths=torch.tensor([n, n], device=DEV)), want_i)


@pytest.mark.parametrize("name", ["spatial_p4_ties", "tiled"])
def test_device_lengths_are_clamped_by_both_pruned_forms(name):
    """11: lengths above n, negative, INT_MAX and INT_MIN: clamped to [0, n] in the kernel."""
    live, _, m, form = case(name)
    n = live.shape[1]
    lib = _lib.load()
    assert lib.mcp_fps_lengths_form(4, n, m, lib.mcp_fps_lengths_pruned_workspace_bytes(4, n, m)) == form
    xyz = live[:1].repeat(4, 1, 1).contiguous().to(DEV)
    wild = torch.tensor([n + 1000, -3, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    rc, idx, pts = call(PRUNED, xyz, wild, m)
    rc_w, idx_w, pts_w = call(PRUNED, xyz, (n, 0, n, 0), m)
    assert rc == 0 and rc_w == 0 and torch.equal(idx, idx_w) and torch.equal(pts, pts_w)
    assert torch.equal(idx[0], expected(name)[0]) and torch.equal(idx[2], idx[0])
    assert not idx[1].any() and not pts[1].any() and not idx[3].any() and not pts[3].any()


def test_backend_takes_the_tiled_form_for_whole_scans():
    """HipBackend.fps(lengths=) sizes its workspace with the pruned query; the result is the oracle's either way."""
    live, lens, m, _ = case("tiled")
    idx, pts = ops.backend().fps(filled(live, lens, "nan").to(DEV), m, with_points=True, lengths=list(lens))
    assert torch.equal(idx.cpu(), expected("tiled"))
    gather = base.gathered(live, expected("tiled"))
    for b, l in enumerate(lens):
        assert torch.equal(pts[b].cpu(), gather[b] if l else torch.zeros(m, 3)), (b, l)
