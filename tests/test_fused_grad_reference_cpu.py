"""-m "not gpu": the float64 gradients of tests/fused_grad_reference.py against the unfused twins of mocopci_amd/grad.py run in float64
on the CPU with a plain row gather, and the share of every backward case's upstream gradient that the clear rules keep."""
import pytest
import torch

from mocopci_amd import grad
from tests import fused_grad_reference as gr
from tests import kernel_variants as kv

TINY = [
    dict(op="fusion", tag="tiny", b=2, n=37),
    dict(op="fusion", tag="tiny-same", b=2, n=19, same=True, dup=True),
    dict(op="cross", tag="tiny", d=64, b=2, n1=23, n2=29),
    dict(op="cross", tag="tiny", d=256, b=2, n1=5, n2=29),
    dict(op="pointconv_agg", tag="tiny", b=2, n=40, s=17, d=32),
    dict(op="ptblock", tag="tiny", b=2, n=21),
]


def twin(case, leaves, idx):
    op = case["op"]
    if op == "fusion":
        return grad.fusion_twin(gr.gather, *leaves[:2], idx, *leaves[2:])
    if op == "cross":
        return grad.cross_twin(gr.gather, *leaves[:4], idx, *leaves[4:])
    if op == "pointconv_agg":
        return grad.pointconv_agg_twin(gr.gather, *leaves[:3], idx, *leaves[3:])
    return grad.ptblock_twin(gr.gather, *leaves[:4], idx, *leaves[4:])


@pytest.mark.parametrize("case", TINY, ids=lambda c: f"{c['op']}-{c.get('d', '')}-{c['tag']}")
def test_the_float64_gradients_agree_with_the_unfused_twin_in_float64(case):
    """To 1e-10 of each gradient's largest entry; gradients that are zero in exact arithmetic are float64 rounding noise on both
    sides and are held to 1e-12 absolute."""
    prep = gr.prepare(case)
    mine = gr.gradients(prep)
    leaves = [t.double().clone().requires_grad_(True) for t in prep.leaves]
    out = twin(case, leaves, prep.idx)
    want = torch.autograd.grad(out, leaves, prep.g.reshape(out.shape))
    assert float(prep.g.abs().max()) > 0.1
    for name, a, b in zip(prep.names, mine, want):
        assert a.shape == b.shape and a.dtype == torch.float64, name
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        if gr.exact_zero(case, name):
            assert scale <= 1e-12 and err <= 1e-12, f"{name}: {scale:.2e}"
        else:
            assert scale > 0 and err <= 1e-10 * scale, f"grad {name}: max err {err:.2e}, gradient scale {scale:.2e}"


def test_a_point_contribution_is_the_gradient_with_the_upstream_masked_to_it():
    case = TINY[0]
    prep = gr.prepare(case)
    whole = gr.gradients(prep)
    parts = [gr.gradients(prep, sel=[p]) for p in range(prep.total)]
    for k, name in enumerate(prep.names):
        torch.testing.assert_close(sum(p[k] for p in parts), whole[k], rtol=0, atol=1e-12 * float(whole[k].abs().max()), msg=name)
    assert float(parts[-1][6].abs().max()) > 0    # w3 sees the last point


@pytest.mark.parametrize("case", kv.GRAD_CASES, ids=kv.grad_case_id)
def test_the_clear_rules_keep_the_upstream_gradient_of_every_backward_case(case):
    """More than 0.9 of the mask (points; (point, channel) pairs in cross), all of it in a case of 8 points or fewer; decided by the
    float64 reference alone.  The gradients that exact_zero names are zero in float64, and no other is."""
    prep = gr.prepare(case)
    share = float(prep.clear.double().mean())
    assert share > 0.9, share
    if prep.total <= 8:
        assert bool(prep.clear.all()), f"{int((~prep.clear).sum())} of {prep.clear.numel()} not clear: choose another seed"
    for name, g in zip(prep.names, gr.gradients(prep)):
        assert torch.isfinite(g).all(), name
        if gr.exact_zero(case, name):
            assert float(g.abs().max()) <= 1e-12, name
        else:
            assert float(g.abs().max()) > 1e-6, name
