"""-m "not gpu": the float64 statements of tests/fused_reference.py against the fp32 oracle (oracle/backend.py), at small shapes and
within the bound each statement computes beside its value -- so the references that judge the HIP kernels in
test_fused_variants_gpu.py are themselves checked on a machine without a GPU, against an independent statement of the same layers.

C_ORACLE: the oracle is plain fp32 torch on the CPU; its sums run in another order than the kernels' but obey the same rounding
model, so it gets the largest constant a kernel family may need before the issue behind these tests calls it a finding (16)."""
import pytest
import torch

from oracle.backend import OracleBackend
from tests import fused_reference as fr

C_ORACLE = 16.0


def check(want32, exact, bound):
    assert exact.dtype == bound.dtype == torch.float64 and exact.shape == bound.shape
    assert torch.isfinite(exact).all() and torch.isfinite(bound).all() and (bound >= 0).all()
    err = (want32.double().reshape(exact.shape) - exact).abs()
    ratio = (err / (C_ORACLE * fr.U * bound).clamp_min(1e-300)).max().item()
    assert ratio <= 1.0, f"oracle and float64 statement differ by {ratio:.2f} x the bound"
    # and the bound is a bound, not a licence: nowhere more than 2^-10 of the output's scale
    assert (fr.U * bound).max().item() <= 2.0 ** -10 * max(1.0, exact.abs().max().item())


@pytest.mark.parametrize("kw", [dict(b=2, n=150), dict(b=1, n=5, same=True), dict(b=2, n=70, extent=True, dup=True)], ids=str)
def test_fusion_reference_matches_the_fp32_oracle(kw):
    p1, p2, idx, ws = fr.fusion_inputs(kw)
    exact, bound = fr.fusion_reference(p1, p2, idx, *ws)
    check(OracleBackend().fusion_mlp(p1, p2, idx, *ws), exact, bound)
    whole = fr.fusion_reference(p1, p2, torch.cat(idx, -1), *ws, sel=torch.arange(3), block=2)   # one list, a selection, ragged blocks
    assert torch.equal(whole[0], exact[:3]) and torch.equal(whole[1], bound[:3])


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("extent", [False, True])
def test_cross_reference_matches_the_fp32_oracle(d, extent):
    xyz1, xyz2, f1, f2, idx, w = fr.cross_inputs(dict(b=2, n1=50, n2=41, d=d, extent=extent))
    check(OracleBackend().cross_volume(xyz1, xyz2, f1, f2, idx, tuple(w)), *fr.cross_reference(xyz1, xyz2, f1, f2, idx, *w))


@pytest.mark.parametrize("d,extent", [(5, False), (32, True), (64, False), (256, True)])
def test_pointconv_references_match_the_fp32_oracle(d, extent):
    c_out = d if d in (32, 64) else None
    s_xyz, new_xyz, pts, idx, wn, lin = fr.pointconv_inputs(dict(b=2, n=150, s=77, d=d, extent=extent, c_out=c_out))
    ob = OracleBackend()
    check(ob.pointconv_agg(s_xyz, new_xyz, pts, idx, *wn), *fr.pointconv_agg_reference(s_xyz, new_xyz, pts, idx, *wn))
    if c_out:
        exact, bound = fr.pointconv_linear_reference(s_xyz, new_xyz, pts, idx, *wn, *lin, 0.1)
        check(ob.pointconv_linear(s_xyz, new_xyz, pts, idx, *wn, *lin, 0.1), exact, bound)
        assert 0.1 < (exact > 0).double().mean().item() < 0.9     # both branches of the LeakyReLU are taken


@pytest.mark.parametrize("kw", [dict(b=2, n=75), dict(b=1, n=1), dict(b=2, n=60, logits=80.0, extent=True), dict(b=2, n=60, same=True)], ids=str)
def test_ptblock_reference_matches_the_fp32_oracle(kw):
    xyz, q, k, v, idx, ws = fr.ptblock_inputs(kw)
    exact, bound = fr.ptblock_reference(xyz, q, k, v, idx, *ws)
    check(OracleBackend().ptblock_attention(xyz, q, k, v, idx, tuple(ws)), exact, bound)
    if kw.get("logits"):
        assert abs(fr.ptblock_logits(xyz, q, k, v, idx, *ws).abs().max().item() - kw["logits"]) < 1.0


def test_a_two_term_split_leaves_every_reference_outside_its_bound():
    """What the GPU tests rely on, as far as a machine without a GPU can show it: on this data a statement whose multiplicands lost the
    third term of the bf16 split is further from the float64 value than 16 x the bound (the largest constant a family may have) for
    the layers without a softmax, and further than the bound itself (the families' constants are 1) for the two with one, where the
    normalisation takes the common part of the logits' error away."""
    from tests.test_kernel_variants_gpu import two_term

    def ratio(fn, *args, c=16.0):
        exact, bound = fn(*args)
        return ((fn(*args, cut=two_term)[0] - exact).abs() / (c * fr.U * bound).clamp_min(1e-300)).max().item()
    xyz1, xyz2, f1, f2, idx, w = fr.cross_inputs(dict(b=2, n1=50, n2=41, d=64))
    assert ratio(fr.cross_reference, xyz1, xyz2, f1, f2, idx, *w) > 1.0
    s_xyz, new_xyz, pts, idx, wn, lin = fr.pointconv_inputs(dict(b=2, n=150, s=77, d=32, c_out=32))
    assert ratio(fr.pointconv_agg_reference, s_xyz, new_xyz, pts, idx, *wn) > 1.0
    assert ratio(lambda *a, **k: fr.pointconv_linear_reference(*a, 0.1, **k), s_xyz, new_xyz, pts, idx, *wn, *lin) > 1.0
    p1, p2, idx, ws = fr.fusion_inputs(dict(b=1, n=61))
    assert ratio(fr.fusion_reference, p1, p2, idx, *ws, c=1.0) > 4.0
    xyz, q, k, v, idx, ws = fr.ptblock_inputs(dict(b=2, n=60))
    assert ratio(fr.ptblock_reference, xyz, q, k, v, idx, *ws, c=1.0) > 4.0
