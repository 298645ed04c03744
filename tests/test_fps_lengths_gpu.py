"""The length-aware furthest point sampling (mcp_furthest_point_sampling_lengths, csrc/fps_lengths.hip) against the CPU oracle run
on every element's valid prefix alone, with exact equality.  The padding is NaN in one filling and 1e30 in another: a kernel that
reads it selects it (or poisons its distances), so neither may move an output bit.  The first batch is a tie-heavy cloud (rows
drawn with repetition from a 16 x 16 x 4 integer grid): there the tie order decides most selections, and the oracle on the
zero-padded cloud differs from the oracle on the prefix, so wrong candidates or a wrong tie key cannot pass."""
import functools

import numpy as np
import pytest
import torch

from mocopci_amd import _lib, compat, data, ops
from oracle import pointset as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILLINGS = {"zero": 0.0, "nan": float("nan"), "big": 1e30}


def cloud(seed, b, n, dup=0.05, extent=(40.0, 40.0, 3.0)):
    """tests/test_knn_lengths_gpu.py's cloud(): uniform points with 5 % exact duplicates."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(b, n, 3, generator=g) * 2 - 1) * torch.tensor(extent)
    nd = int(n * dup)
    if nd:
        src = torch.randint(0, n - nd, (nd,), generator=g)
        x[:, n - nd:] = x[:, src]
        x = x[:, torch.randperm(n, generator=g)]
    return x.contiguous()


def tie_cloud(n):
    g = torch.Generator().manual_seed(33)
    return torch.stack([torch.randint(0, 16, (n,), generator=g), torch.randint(0, 16, (n,), generator=g),
                        torch.randint(0, 4, (n,), generator=g)], dim=-1).float()


@functools.lru_cache(maxsize=None)
def case(name):
    """(live points (B,n,3), lengths, m)"""
    if name == "tie":      # three points per reference thread, every block-size class, m > l, the empty element
        lens = (2100, 1024, 1023, 513, 130, 65, 63, 5, 1, 0)
        return tie_cloud(2100)[None].repeat(len(lens), 1, 1).contiguous(), lens, 48
    if name == "dup":      # the widest register form and the slice skipping
        return cloud(5, 4, 16384), (16384, 8193, 4097, 1), 64
    if name == "stream":   # the streaming form
        return cloud(6, 3, 20000), (20000, 16385, 100), 32
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle on each element's prefix alone; an all-zero row for the empty element."""
    pts, lens, m = case(name)
    idx = torch.zeros(len(lens), m, dtype=torch.int32)
    for b, l in enumerate(lens):
        if l:
            idx[b] = orc.furthest_point_sample(pts[b:b + 1, :l].contiguous(), m)[0]
    return idx


@functools.lru_cache(maxsize=None)
def filled(name, filling):
    pts, lens, _ = case(name)
    pts = pts.clone()
    for b, l in enumerate(lens):
        pts[b, l:] = FILLINGS[filling]
    return pts


def sample(name, filling, with_points=False, as_lengths=list):
    _, lens, m = case(name)
    return ops.backend().fps(filled(name, filling).to(DEV), m, with_points=with_points, lengths=as_lengths(lens))


def gathered(pts, idx):
    return torch.gather(pts, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))


def test_tie_cloud_is_not_vacuous():
    """CPU only: on the zero-padded cloud the oracle selects other points than on the prefix, for lengths below 1024."""
    pts, lens, m = case("tie")
    want = expected("tie")
    differing = {}
    for b, l in enumerate(lens):
        if 1 < l < 1024:
            on_padded = orc.furthest_point_sample(filled("tie", "zero")[b:b + 1], m)[0]
            differing[l] = int((on_padded != want[b]).sum())
    print("indices that differ between the zero-padded cloud and the prefix:", differing)
    assert any(v > 0 for v in differing.values()), differing


@pytest.mark.parametrize("filling", ["nan", "big"])
@pytest.mark.parametrize("name", ["tie", "dup", "stream"])
def test_indices_equal_the_oracle_on_the_prefixes(name, filling):
    idx = sample(name, filling)
    _, lens, m = case(name)
    assert idx.dtype == torch.int32 and idx.shape == (len(lens), m)
    got, want = idx.cpu(), expected(name)
    for b, l in enumerate(lens):
        assert torch.equal(got[b], want[b]), (name, filling, b, l, int((got[b] != want[b]).sum()))


def test_streaming_form_needs_its_workspace():
    pts, lens, m = case("stream")
    B, n = pts.shape[0], pts.shape[1]
    lib = _lib.load()
    need = lib.mcp_fps_lengths_workspace_bytes(B, n, m)
    assert need == B * n * 4
    xyz = filled("stream", "nan").to(DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    idx = torch.full((B, m), -77, dtype=torch.int32, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    call = lib.mcp_furthest_point_sampling_lengths
    assert call(B, n, m, xyz.data_ptr(), lens_d.data_ptr(), idx.data_ptr(), None, None, 0, stream) == 10002
    assert call(B, n, m, xyz.data_ptr(), lens_d.data_ptr(), idx.data_ptr(), None, ws.data_ptr(), need - 1, stream) == 10002
    torch.cuda.synchronize()
    assert bool((idx == -77).all())                         # nothing was launched
    assert call(B, n, m, xyz.data_ptr(), lens_d.data_ptr(), idx.data_ptr(), None, ws.data_ptr(), need, stream) == 0
    assert torch.equal(idx.cpu(), expected("stream"))


@pytest.mark.parametrize("n", [1024, 4096, 100])
def test_lengths_that_change_nothing(n):
    be = ops.backend()
    xyz = cloud(40 + n, 2, n).to(DEV)
    m = min(n, 128)
    want_i, want_p = be.fps(xyz, m, with_points=True)
    assert torch.equal(want_i.cpu(), orc.furthest_point_sample(xyz.cpu(), m))
    for lengths in (None, [n, n], torch.tensor([n, n], device=DEV)):
        got_i, got_p = be.fps(xyz, m, with_points=True, lengths=lengths)
        assert torch.equal(got_i, want_i) and torch.equal(got_p, want_p), (n, lengths)
        assert torch.equal(be.fps(xyz, m, lengths=lengths), want_i)
    # the entry point without a length array is the fresh sampling itself
    idx = torch.full((2, m), -1, dtype=torch.int32, device=DEV)
    rc = _lib.load().mcp_furthest_point_sampling_lengths(2, n, m, xyz.data_ptr(), None, idx.data_ptr(), None, None, 0,
                                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(idx, want_i)


@pytest.mark.parametrize("name", ["tie", "stream"])
def test_sampled_xyz_is_the_gather_of_the_indices(name):
    idx, pts = sample(name, "nan", with_points=True)
    _, lens, m = case(name)
    assert pts.shape == (len(lens), m, 3) and torch.equal(idx.cpu(), expected(name))
    want = gathered(case(name)[0], expected(name))
    for b, l in enumerate(lens):
        if l:
            assert torch.equal(pts[b].cpu(), want[b]), (b, l)
        else:
            assert not idx[b].any() and not pts[b].any() and not torch.isnan(pts[b]).any()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_device_tensor_lengths(dtype):
    want = expected("tie")
    assert torch.equal(sample("tie", "big", as_lengths=lambda v: torch.tensor(v, dtype=dtype, device=DEV)).cpu(), want)
    assert torch.equal(sample("tie", "big", as_lengths=lambda v: torch.tensor(v, dtype=dtype)).cpu(), want)


def test_device_lengths_are_clamped_by_the_kernel():
    """A device tensor is trusted by the host: the kernel clamps a length above n to n and treats a negative one as 0."""
    be = ops.backend()
    n, m = 2100, 48
    xyz = tie_cloud(n)[None].repeat(4, 1, 1).contiguous().to(DEV)
    got_i, got_p = be.fps(xyz, m, with_points=True, lengths=torch.tensor([n + 1000, -3, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV))
    want_i, want_p = be.fps(xyz, m, with_points=True, lengths=[n, 0, n, 0])
    assert torch.equal(got_i, want_i) and torch.equal(got_p, want_p)
    assert torch.equal(got_i[0].cpu(), expected("tie")[0]) and not got_i[1].any() and not got_p[1].any()
    with pytest.raises(RuntimeError, match="lengths"):      # host lengths are validated before the call
        be.fps(xyz, m, lengths=[n + 1, 0, 0, 0])


def test_compat_sample_farthest_points():
    pts, lens, K = case("tie")
    B = len(lens)
    xyz = filled("tie", "nan").to(DEV)
    sampled, idx = compat.sample_farthest_points(xyz, lengths=torch.tensor(lens), K=K)
    assert idx.dtype == torch.int64 and idx.shape == (B, K) and sampled.shape == (B, K, 3)
    want = expected("tie")
    for b, l in enumerate(lens):
        live = min(l, K)
        assert torch.equal(idx[b, :live].cpu().int(), want[b, :live]), (b, l)
        assert torch.equal(sampled[b, :live].cpu(), pts[b, want[b, :live].long()])
        assert bool((idx[b, live:] == -1).all()) and not sampled[b, live:].any()    # pytorch3d's padding: -1 and 0.0
    # without lengths: every row is live
    s2, i2 = compat.sample_farthest_points(pts[:1].to(DEV), K=K)
    assert torch.equal(i2[0].cpu().int(), want[0]) and torch.equal(s2[0].cpu(), pts[0, want[0].long()])
    # the lengths chain: the sampled queries against the cloud they were sampled from
    l1 = torch.tensor([min(l, K) for l in lens])
    dists, nbr, _ = compat.knn_points(sampled, xyz, lengths1=l1, lengths2=torch.tensor(lens), K=4)
    assert nbr.shape == dists.shape == (B, K, 4)
    b = lens.index(130)
    wi, wd = orc.knn(sampled[b:b + 1, :K].cpu(), pts[b:b + 1, :130].contiguous(), 4, 1, return_dist=True)
    assert torch.equal(nbr[b].cpu().int(), wi[0]) and torch.equal(dists[b].cpu(), wd[0])
    assert not nbr[lens.index(0)].any() and not dists[lens.index(0)].any()


def test_downsample_padded():
    g = torch.Generator().manual_seed(9)
    scans = [torch.randn(n, 3, generator=g) * 20 for n in (700, 300, 40)]
    _, gts, lens = data.collate_padded([([torch.zeros(4, 3)], [s]) for s in scans])
    assert gts[0].shape == (3, 700, 3) and lens[0].tolist() == [700, 300, 40]
    points, new_lengths = data.downsample_padded(gts[0].to(DEV), lens[0], 256)
    assert points.shape == (3, 256, 3) and new_lengths.dtype == torch.int32 and new_lengths.tolist() == [256, 256, 40]
    for b, s in enumerate(scans):
        keep = min(256, s.shape[0])
        pick = orc.furthest_point_sample(s[None].contiguous(), keep)[0].long()
        assert torch.equal(points[b, :keep].cpu(), s[pick]), b
        assert not points[b, keep:].any()
    assert len(set(orc.furthest_point_sample(scans[2][None].contiguous(), 40)[0].tolist())) == 40   # a short scan comes back whole


def test_evaluate_downsamples_whole_ground_truth_frames(tmp_path):
    """evaluate(raw_gt=True, gt_points=256) on two sequences whose ground-truth frames hold 700 / 300 / 40 points (in two orders):
    its Chamfer distance and EMD are those computed by hand from downsample_padded's output, and gt_points=None is today's value."""
    from torch.utils.data import DataLoader
    from mocopci_amd import emd
    rng = np.random.default_rng(0)
    lines, gt_sizes = [], [(700, 300, 40), (40, 700, 300)]
    for s, gts in enumerate(gt_sizes):
        names = []
        for i, n in enumerate((600, 512, 512, 530) + gts):
            names.append(f"scene00_seq{s:04d}_frame{i:02d}.bin")
            data.write_frame(tmp_path / names[-1], rng.normal(size=(n, 3)).astype(np.float32) * 20)
        lines.append(" ".join(names))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    ds = data.NLDriveDataset(str(tmp_path), str(tmp_path / "list.txt"), num_points=512, raw_gt=True)
    loader = DataLoader(ds, batch_size=2, collate_fn=data.collate_padded)
    outs = [t.to(DEV) for t in cloud(70, 6, 512, extent=(40.0, 40.0, 40.0)).split(2)]   # three fixed "predictions" (2,512,3)
    net = lambda a, b: outs
    be = ops.backend()
    np.random.seed(0)
    _, gts, lens = next(iter(loader))
    np.random.seed(0)
    res = data.evaluate(net, loader, device=DEV, raw_gt=True, raw_emd=True, gt_points=256)
    np.random.seed(0)
    plain = data.evaluate(net, loader, device=DEV, raw_gt=True, raw_emd=True, gt_points=None)
    np.random.seed(0)
    default = data.evaluate(net, loader, device=DEV, raw_gt=True, raw_emd=True)
    for j in range(3):
        assert lens[j].tolist() == [gt_sizes[0][j], gt_sizes[1][j]]
        scan, count = data.downsample_padded(gts[j].to(DEV), lens[j], 256)
        assert count.tolist() == [min(256, v) for v in lens[j].tolist()]
        assert res["chamfer"][j] == float(be.chamfer(outs[j], scan, y_lengths=count))
        assert res["emd"][j] == float(emd.EMD(outs[j].permute(0, 2, 1).contiguous(), scan.permute(0, 2, 1).contiguous(), lengths2=count))
        whole = gts[j].to(DEV)
        assert plain["chamfer"][j] == default["chamfer"][j] == float(be.chamfer(outs[j], whole, y_lengths=lens[j]))
        assert plain["emd"][j] == default["emd"][j]
        assert res["chamfer"][j] != plain["chamfer"][j]
