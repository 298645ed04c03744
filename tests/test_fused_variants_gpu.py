"""-m gpu: every forward kernel of the fused point layers (csrc/fusion.hip, cross.hip, pointconv.hip, ptblock.hip) against the float64
statements of tests/fused_reference.py, at the shapes where their persistent loops go wrong: ragged eighths of the per-XCD deal, grids
at their cap, steps that cross several batch elements, workgroups with dead waves, odd point counts, last workgroups with a few
points, both sides of the 16384-centre switch of PointConv.  tests/kernel_variants.py names the kernel and the edge each case reaches;
test_kernel_variants_cpu.py checks that the cases reach every emitted instantiation and every such edge.

Each case asserts |kernel - exact| <= c * 2^-24 * bound element-wise, with the bound the reference computes beside its value
(fused_reference.py states the rules) and one constant c per kernel family, and that the bound is tight enough to matter: the same
reference with every multiplicand cut to the first two terms of the bf16 split (two_term: a kernel that lost the third term of
mfma_split.h) lies outside it on the first SELF_ROWS points.  The data has a positive mean for that, see test_kernel_variants_gpu.py.
A second run, and every other form of the same call (neighbour list as two halves or whole, q/k/v packed or separate, operand image
kept or built on the fly), must give identical bits."""
import pytest
import torch

from mocopci_amd import ops
from tests import fused_reference as fr
from tests import kernel_variants as kv
from tests.test_kernel_variants_gpu import two_term

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = fr.U
# c: the smallest power of two that is at least twice the worst |kernel - exact| / (2^-24 * bound) measured on the MI355X (in brackets)
C_FUSION = 1.0             # fusion_split_kernel [0.432, grid-cap-2-rounds]
C_CROSS = 2.0              # cross_kernel<64 | 128, 1>, cross256_stream_kernel [0.607, batch-map d=128; 0.518 among the variant cases]
C_POINTCONV_AGG = 1.0      # pointconv_agg_kernel, pointconv_agg_lowlevel_kernel: plain fp32 fma chains [0.423, total-16384]
C_POINTCONV_LINEAR = 0.5   # pointconv_linear_kernel [0.219, <64,2> above-16384]
C_PTBLOCK = 1.0            # ptblock_kernel [0.391, xcd-ragged with logits of 80]
SELF_ROWS = 1024           # points of the two-term self-check


def dev(*ts):
    return [t.to(DEV) for t in ts]


def judge(case, got, ref, c):
    """got (points, channels) against ref(sel=None, cut=None) -> (exact, bound); prints the RATIO line of the case."""
    got = got.reshape(-1, got.shape[-1]).double().cpu()
    assert torch.isfinite(got).all()
    exact, bound = ref()
    tol = (c * U * bound).clamp_min(1e-300)
    ratio = ((got - exact).abs() / tol).max().item()
    line = f"RATIO {kv.case_id(case)} kernel={ratio:.3f}"
    ratio2 = None
    if case.get("mutant", True):
        sel = torch.arange(min(got.shape[0], SELF_ROWS))
        ratio2 = ((got[sel] - ref(sel=sel, cut=two_term)[0]).abs() / tol[sel]).max().item()
        line += f" two_term={ratio2:.2f}"
    print(line)
    assert ratio <= 1.0, f"{kv.expected_kernel(**case)}: error {ratio:.2f} x the bound"
    assert ratio2 is None or ratio2 > 1.0, f"the bound does not tell a two-term split from the kernel's three terms ({ratio2:.2f})"


# ---- fusion_split_kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kv.cases("fusion"), ids=kv.case_id)
def test_fusion_variant_matches_float64(case):
    p1, p2, idx, ws = fr.fusion_inputs(case)
    be = ops.backend()
    p1d, p2d, ia, ib = dev(p1, p2, *idx)
    wd = dev(*ws)
    got = be.fusion_mlp(p1d, p2d, (ia, ib), *wd)
    assert torch.equal(be.fusion_mlp(p1d, p2d, (ia, ib), *wd), got), "not bit-reproducible"
    assert torch.equal(be.fusion_mlp(p1d, p2d, torch.cat([ia, ib], -1), *wd), got), "one (B,N,64) list and its two halves differ"
    judge(case, got, lambda **kw: fr.fusion_reference(p1, p2, idx, *ws, **kw), C_FUSION)


# ---- cross_kernel / cross256_stream_kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kv.cases("cross"), ids=kv.case_id)
def test_cross_variant_matches_float64(case):
    xyz1, xyz2, f1, f2, idx, w = fr.cross_inputs(case)
    be = ops.backend()
    x1, x2, g1, g2, ia, ib = dev(xyz1, xyz2, f1, f2, *idx)
    wd = dev(*w)
    packed = be.cross_pack(*wd)
    got = be.cross_volume(x1, x2, g1, g2, (ia, ib), packed)
    assert torch.equal(be.cross_volume(x1, x2, g1, g2, (ia, ib), packed), got), "not bit-reproducible"
    assert torch.equal(be.cross_volume(x1, x2, g1, g2, torch.cat([ia, ib], -1), packed), got), "one (B,N1,32) list and its two halves differ"
    assert torch.equal(be.cross_layer(x1, x2, g1, g2, (ia, ib), *wd), got), "operand image built on the fly"
    assert torch.equal(be.cross_layer(x1, x2, g1, g2, (ia, ib), *wd, packed=packed), got), "operand image kept"
    judge(case, got, lambda **kw: fr.cross_reference(xyz1, xyz2, f1, f2, idx, *w, **kw), C_CROSS)


@pytest.mark.parametrize("d,n", [(64, 83), (128, 83), (256, 40)])
def test_cross_batch_map_equals_the_replicated_tensors(d, n):
    """bmap + shared in {1, 2, 4 | 2}: element b of the flagged tensors is read from element bmap[b] of a 4-element batch.  The
    9 x 83 points run on 24 workgroups by XCD (D = 64) and on 12 and 90 round-robin (D = 128, 256); the replicated call is itself
    held against float64."""
    members = torch.tensor([0, 1, 2, 3, 0, 2, 3, 1, 1])
    case = dict(op="cross", tag="batch-map", d=d, b=len(members), n1=n, n2=n, extent=True)
    xyz1, xyz2, f1, f2, (ia, ib), w = fr.cross_inputs(case)
    f1, f2, ia = f1[:4], f2[:4], ia[:4]                                 # the 4 sources ...
    r1, r2, ra = f1[members].contiguous(), f2[members].contiguous(), ia[members].contiguous()   # ... and their replication
    be = ops.backend()
    x1, x2, ibd, m = dev(xyz1, xyz2, ib, members.int())
    packed = be.cross_pack(*dev(*w))
    want = be.cross_volume(x1, x2, *dev(r1, r2), (ra.to(DEV), ibd), packed)
    for shared in (1, 2, 4 | 2):
        a1, a2, aa = (f1 if shared & 1 else r1), (f2 if shared & 2 else r2), (ia if shared & 4 else ra)
        got = be.cross_volume(x1, x2, *dev(a1, a2), (aa.to(DEV), ibd), packed, bmap=m, shared=shared)
        assert torch.equal(got, want), f"shared={shared}"
    judge(case, want, lambda **kw: fr.cross_reference(xyz1, xyz2, r1, r2, (ra, ib), *w, **kw), C_CROSS)


# ---- pointconv_agg_kernel / pointconv_agg_lowlevel_kernel ---------------------------------------------------------------------------
LOWLEVEL_CHUNK = 8192   # centres per call of the per-element comparison: the low-level route for every d (pointconv.hip:474-479)


@pytest.mark.parametrize("case", kv.cases("pointconv_agg"), ids=kv.case_id)
def test_pointconv_agg_variant_matches_float64(case):
    """The streaming kernels (above 16384 centres) must also give, bit for bit, what the low-level kernel gives for the same centres,
    run per batch element in pieces of at most 8192 centres: pointconv.hip claims the same arithmetic for both."""
    s_xyz, new_xyz, pts, idx, wn, _ = fr.pointconv_inputs(case)
    be = ops.backend()
    sx, nx, pd, ix = dev(s_xyz, new_xyz, pts, idx)
    wd = dev(*wn)
    if not case.get("aligned", True):   # the same values, 4 bytes into their storage
        buf = torch.empty(pts.numel() + 1, device=DEV)
        buf[1:].copy_(pd.flatten())
        pd = buf[1:].view(pts.shape)
        assert pd.is_contiguous() and pd.data_ptr() % 16 == 4
    got = be.pointconv_agg(sx, nx, pd, ix, *wd)
    assert torch.equal(be.pointconv_agg(sx, nx, pd, ix, *wd), got), "not bit-reproducible"
    if "lowlevel" not in kv.expected_kernel(**case):
        for b in range(case["b"]):
            for c0 in range(0, case["s"], LOWLEVEL_CHUNK):
                c1 = min(c0 + LOWLEVEL_CHUNK, case["s"])
                assert "lowlevel" in kv.expected_kernel("pointconv_agg", b=1, s=c1 - c0, d=case["d"])
                part = be.pointconv_agg(sx[b:b + 1], nx[b:b + 1, c0:c1], pd[b:b + 1], ix[b:b + 1, c0:c1], *wd)
                assert torch.equal(part[0], got[b, c0:c1]), f"streaming and low-level kernel differ (batch element {b}, centres {c0}..{c1})"
    judge(case, got, lambda **kw: fr.pointconv_agg_reference(s_xyz, new_xyz, pts, idx, *wn, **kw), C_POINTCONV_AGG)


# ---- pointconv_linear_kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kv.cases("pointconv_linear"), ids=kv.case_id)
def test_pointconv_linear_variant_matches_float64(case):
    s_xyz, new_xyz, pts, idx, wn, lin = fr.pointconv_inputs(case)
    be = ops.backend()
    args = dev(s_xyz, new_xyz, pts, idx, *wn, *lin)
    got = be.pointconv_linear(*args, 0.1)
    assert torch.equal(be.pointconv_linear(*args, 0.1), got), "not bit-reproducible"
    assert torch.equal(be.pointconv_linear(*args, 0.1, packed=be.pointconv_linear_pack(*args[-2:])), got), "operand image kept"
    if case["b"] * case["s"] >= 16384:   # where the model uses it: the two-kernel form's bits (docstring of mcp_pointconv_linear)
        assert torch.equal(be.linear(be.pointconv_agg(*args[:-2]), *args[-2:], 0.1), got)
    judge(case, got, lambda **kw: fr.pointconv_linear_reference(s_xyz, new_xyz, pts, idx, *wn, *lin, 0.1, **kw), C_POINTCONV_LINEAR)


# ---- ptblock_kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kv.cases("ptblock"), ids=kv.case_id)
def test_ptblock_variant_matches_float64(case):
    xyz, q, k, v, idx, ws = fr.ptblock_inputs(case)
    be = ops.backend()
    xd, qd, kd, vd, ix = dev(xyz, q, k, v, idx)
    wd = dev(*ws)
    packed = be.ptblock_pack(*wd)
    qkv = torch.cat([qd, kd, vd], dim=-1)   # one (B,N,192) projection: row stride 192
    strided = lambda: be.ptblock_attention(xd, qkv[..., :64], qkv[..., 64:128], qkv[..., 128:], ix, packed)
    separate = lambda: be.ptblock_attention(xd, qd, kd, vd, ix, packed)
    first, other = (strided, separate) if case.get("packed") else (separate, strided)
    got = first()
    assert torch.equal(first(), got), "not bit-reproducible"
    assert torch.equal(other(), got), "q, k, v as slices of one (B,N,192) tensor and as separate tensors differ"
    assert torch.equal(be.ptblock_layer(xd, qd, kd, vd, ix, wd), got), "operand image built on the fly"
    assert torch.equal(be.ptblock_layer(xd, qd, kd, vd, ix, wd, packed=packed), got), "operand image kept"
    judge(case, got, lambda **kw: fr.ptblock_reference(xyz, q, k, v, idx, *ws, **kw), C_PTBLOCK)
