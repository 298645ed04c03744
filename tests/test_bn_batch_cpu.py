"""BatchNorm on batch statistics with per-group lengths, without a GPU: the float64 reference (tests/bn_batch_reference.py) against
torch.nn.functional.batch_norm(training=True) on every group cut to its length; MoCoPCI.bn_batch(lengths=) on the CPU oracle backend
(the masked torch formulation, mocopci_amd.grad.bn_batch_lengths_twin) against the reference, with its running estimates against G
sequential calls of today's bn_batch on the cropped groups; and the argument checks and the chunking of the C entry points, which need
no device."""
import pytest
import torch
import torch.nn.functional as F

from mocopci_amd import _lib, grad, model as mm, ops
from tests import bn_batch_reference as ref
from tests.bn_batch_reference import CASES, EPS, case_id

NORMS = {64: "multi_frame_inference.multi_frame_up_1.cross_block.norm1", 128: "multi_frame_inference.multi_frame_up_2.cross_block.norm1",
         256: "multi_frame_inference.cross_block3.norm1"}


def by_tag(tag):
    return next(c for c in CASES if c["tag"] == tag)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_reference_is_batch_norm_on_every_group_cut_to_its_length(case):
    prep = ref.prepare(case)
    ev, C = prep.ev, case["c"]
    dgamma, dbeta = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for g, ln in enumerate(case["lens"]):
        m = case["f"] * ln
        assert int(ev.count[g]) == m
        assert not ev.y[g, :, ln:].any() and not ev.dx[g, :, ln:].any()
        if m == 0:
            assert not ev.mean[g].any() and not ev.var[g].any() and not ev.y[g].any() and not ev.dx[g].any()
            continue
        rows = prep.x[g, :, :ln].double().reshape(m, C)
        if m == 1:      # batch_norm refuses one value per channel: the definition gives var 0, y = beta, dx = 0
            assert torch.equal(ev.mean[g], rows[0]) and not ev.var[g].any()
            assert torch.allclose(ev.y[g, :, :ln].reshape(m, C), prep.beta.double().expand(m, C), rtol=0, atol=1e-12)
            assert torch.allclose(ev.dx[g, :, :ln], torch.zeros(()).double(), rtol=0, atol=1e-9)
            dbeta += prep.dy[g, :, :ln].double().reshape(m, C).sum(0)
            continue
        rows.requires_grad_(True)
        w, b = prep.gamma.double().requires_grad_(True), prep.beta.double().requires_grad_(True)
        y = F.batch_norm(rows, None, None, w, b, training=True, eps=EPS)
        gx, gw, gb = torch.autograd.grad(y, (rows, w, b), prep.dy[g, :, :ln].double().reshape(m, C))
        assert torch.allclose(ev.y[g, :, :ln].reshape(m, C), y.detach(), rtol=1e-10, atol=1e-10)
        assert torch.allclose(ev.mean[g], rows.detach().mean(0), rtol=1e-12, atol=1e-12)
        assert torch.allclose(ev.var[g], rows.detach().var(0, unbiased=False), rtol=1e-10, atol=1e-14)
        assert torch.allclose(ev.dx[g, :, :ln].reshape(m, C), gx, rtol=1e-8, atol=1e-9)
        dgamma += gw
        dbeta += gb
    assert torch.allclose(ev.dgamma, dgamma, rtol=1e-9, atol=1e-9) and torch.allclose(ev.dbeta, dbeta, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_torch_formulation_matches_the_reference(case):
    """grad.bn_batch_lengths_twin in float64 with NaN in the padded rows of x and of the upstream gradient."""
    prep = ref.prepare(case)
    ev = prep.ev
    pad = ~prep.live.view(case["g"], 1, case["n"], 1).expand_as(prep.x)
    x, dy = prep.x.double().clone(), prep.dy.double().clone()
    x[pad] = dy[pad] = float("nan")
    leaves = [x.requires_grad_(True), prep.gamma.double().requires_grad_(True), prep.beta.double().requires_grad_(True)]
    y, mean, var, count = grad.bn_batch_lengths_twin(*leaves, EPS, prep.lens)
    assert count.dtype == torch.int32 and torch.equal(count.long(), ev.count)
    for name, a, e in zip(("y", "mean", "var"), (y, mean, var), (ev.y, ev.mean, ev.var)):
        assert torch.isfinite(a).all() and torch.allclose(a.detach(), e, rtol=1e-10, atol=1e-10), name
    for name, a, e in zip(("dx", "dgamma", "dbeta"), torch.autograd.grad(y, leaves, dy), (ev.dx, ev.dgamma, ev.dbeta)):
        assert torch.isfinite(a).all() and torch.allclose(a, e, rtol=1e-8, atol=1e-9), name
    assert not y[pad].any()


def on_the_cpu_backend(fn):
    from oracle.backend import OracleBackend
    prev = ops.set_backend(OracleBackend())
    try:
        return fn()
    finally:
        ops.set_backend(prev)


@pytest.mark.parametrize("tag", ["frames", "wide"])
def test_the_model_on_the_cpu_backend_matches_the_reference_and_the_sequential_cropped_calls(tag):
    """MoCoPCI.bn_batch(lengths=) with the layer's own weight and bias: y against the reference; running_mean, running_var (each
    group's m / (m - 1): 2 for the one-point group of `wide`) and num_batches_tracked against G calls of today's bn_batch, one per
    group on x[g, :, :len]."""
    from tests import harness_checks as hc
    case = by_tag(tag)
    prep = ref.prepare(case)
    name = NORMS[case["c"]]
    net, seq = hc.build_model("cpu"), hc.build_model("cpu")
    P = net._params()
    x = prep.x.clone()
    x[~prep.live.view(case["g"], 1, case["n"], 1).expand_as(x)] = float("nan")
    with torch.no_grad():
        y = on_the_cpu_backend(lambda: net.bn_batch(x, name, EPS, lengths=case["lens"]))
        for g, ln in enumerate(case["lens"]):
            alone = on_the_cpu_backend(lambda: seq.bn_batch(prep.x[g:g + 1, :, :ln].contiguous(), name, EPS))
            assert torch.allclose(y[g, :, :ln], alone[0], rtol=1e-4, atol=1e-4)
    want, _, _, _ = ref.forward(prep.x.double(), prep.lens, P[name + ".weight"].double(), P[name + ".bias"].double())
    assert torch.isfinite(y).all()
    assert float((y.double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    a, b = dict(net.named_buffers()), dict(seq.named_buffers())
    assert torch.allclose(a[name + ".running_mean"], b[name + ".running_mean"], rtol=1e-5, atol=1e-6)
    assert torch.allclose(a[name + ".running_var"], b[name + ".running_var"], rtol=1e-4, atol=1e-7)
    assert int(a[name + ".num_batches_tracked"]) == int(b[name + ".num_batches_tracked"]) and int(a[name + ".num_batches_tracked"]) >= case["g"]


def test_a_group_without_a_live_row_updates_the_running_estimates_like_any_other():
    """empty-middle: the closed-form update over the three groups with the reference's statistics (mean 0, var 0 for the empty one),
    each variance scaled by its group's m / (m - 1) (1 where m < 2); three batches tracked."""
    from tests import harness_checks as hc
    case = by_tag("empty-middle")
    prep = ref.prepare(case)
    name = NORMS[64]
    net = hc.build_model("cpu")
    sd = dict(net.named_buffers())
    rm, rv, nb = (sd[name + k].clone().double() for k in (".running_mean", ".running_var", ".num_batches_tracked"))
    with torch.no_grad():
        y = on_the_cpu_backend(lambda: net.bn_batch(prep.x, name, EPS, lengths=torch.tensor(case["lens"])))
    assert torch.isfinite(y).all() and not y[1].any()
    mom = net.BN_MOMENTUM
    for g in range(3):
        m = float(prep.ev.count[g])
        rm = (1 - mom) * rm + mom * prep.ev.mean[g]
        rv = (1 - mom) * rv + mom * prep.ev.var[g] * (m / (m - 1) if m > 1 else 1.0)
    after = dict(net.named_buffers())
    assert torch.allclose(after[name + ".running_mean"].double(), rm, rtol=1e-5, atol=1e-6)
    assert torch.allclose(after[name + ".running_var"].double(), rv, rtol=1e-4, atol=1e-7)
    assert int(after[name + ".num_batches_tracked"]) == int(nb) + 3


def test_the_running_variance_factor_takes_a_row_count():
    f = mm.MoCoPCI.unbias_factor(torch.tensor([0, 1, 2, 500]), rows=1)
    assert f.tolist() == pytest.approx([1.0, 1.0, 2.0, 500.0 / 499.0], rel=1e-6)
    assert mm.MoCoPCI.unbias_factor(torch.tensor([57])).tolist() == pytest.approx([64.0 * 57 / (64.0 * 57 - 1)], rel=1e-6)


def test_the_errors_of_lengths_tensor_surface():
    from tests import harness_checks as hc
    net = hc.build_model("cpu")
    x = torch.zeros(2, 2, 8, 64)
    for bad in ((8,), (8, 9), (-1, 3), (1.5, 2.0)):
        with pytest.raises(RuntimeError, match="lengths"):
            on_the_cpu_backend(lambda: net.bn_batch(x, NORMS[64], EPS, lengths=bad))
    with pytest.raises(ValueError):
        on_the_cpu_backend(lambda: net.bn_batch(torch.zeros(2, 64), NORMS[64], EPS, lengths=(1, 1)))


def test_without_lengths_the_keyword_arguments_change_nothing():
    """lengths=None is today's code: the same bits and the same running estimates as the call without the keyword."""
    from tests import harness_checks as hc
    a, b = hc.build_model("cpu"), hc.build_model("cpu")
    x = ref.prepare(by_tag("frames")).x
    with torch.no_grad():
        ya = on_the_cpu_backend(lambda: a.bn_batch(x, NORMS[128], EPS))
        yb = on_the_cpu_backend(lambda: b.bn_batch(x, NORMS[128], EPS, lengths=None))
    assert torch.equal(ya, yb)
    assert torch.equal(dict(a.named_buffers())[NORMS[128] + ".running_var"], dict(b.named_buffers())[NORMS[128] + ".running_var"])


def test_the_chunking_and_the_argument_checks_need_no_gpu():
    lib = _lib.load()
    # a group's rows are cut into chunks of at least 256 rows, a pure function of (f, n): what the parts-* cases stand on
    assert ref.N_PARTS == 768
    assert lib.mcp_bn_batch_parts(2, 1, ref.N_PARTS, 64) == 3
    assert lib.mcp_bn_batch_parts(1, 1, 256, 64) == 1 and lib.mcp_bn_batch_parts(1, 1, 257, 64) == 2 and lib.mcp_bn_batch_parts(1, 1, 513, 32) == 3
    assert lib.mcp_bn_batch_parts(2, 3, 256, 256) == 3 and lib.mcp_bn_batch_parts(7, 3, 256, 256) == 3       # f * n rows; not a function of g
    assert lib.mcp_bn_batch_parts(8, 5, 8192, 64) == lib.mcp_bn_batch_parts(1, 5, 8192, 128) <= 128
    # (G, parts, 2, C) partial sums and (G, 2, C) merged sums, in double
    assert lib.mcp_bn_batch_workspace_bytes(2, 1, ref.N_PARTS, 64) == (2 * 3 + 2) * 2 * 64 * 8
    assert lib.mcp_bn_batch_workspace_bytes(2, 1, 768, 48) == 0 and lib.mcp_bn_batch_workspace_bytes(0, 1, 768, 64) == 0
    assert lib.mcp_bn_batch_parts(0, 1, 8, 64) == 10001 and lib.mcp_bn_batch_parts(1, 0, 8, 64) == 10001 and lib.mcp_bn_batch_parts(1, 1, -8, 64) == 10001
    assert lib.mcp_bn_batch_parts(1, 1, 8, 48) == 10002
    # nothing is launched on a bad argument: null pointers, a non-positive dimension
    assert lib.mcp_bn_batch_forward(1, 1, 8, 64, None, None, None, None, 1e-5, None, None, None, None, None, 0, None) == 10001
    assert lib.mcp_bn_batch_forward(0, 1, 8, 64, None, None, None, None, 1e-5, None, None, None, None, None, 0, None) == 10001
    assert lib.mcp_bn_batch_backward(1, 1, 8, 64, None, None, None, None, None, 1e-5, None, None, None, None, None, 0, None) == 10001
    assert lib.mcp_bn_batch_backward(1, 1, 0, 64, None, None, None, None, None, 1e-5, None, None, None, None, None, 0, None) == 10001
