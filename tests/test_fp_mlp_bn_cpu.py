"""-m "not gpu": the float64 statement of the feature-propagation layer under a training-mode BatchNorm (tests/fp_mlp_bn_reference.py)
against torch's own float64 composition, the running-statistics rule against nn.BatchNorm2d, the input search of every GPU case, the
fp32 emulation behind the cancellation case, and what of csrc/fp_mlp_bn.hip needs no GPU: declarations, bindings, the shape
predicate and argument validation."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mocopci_amd import _lib, ops
from tests import fp_mlp_bn_reference as fbr
from tests.test_abi_cpu import header_functions
from tests.test_fp_mlp_grad_cpu import C_CAP, case, case_id

# the GPU cases (tests/test_fp_mlp_bn_gpu.py): an image staged whole in LDS, three layers, a streamed wide shape
CASES = [case(64, 3, [64, 64]), case(128, 4, [128, 128, 128]), case(256, 64, [256, 128])]
SMALL = [case(64, 3, [64, 64], b, n) for b, n in ((1, 5), (2, 64))]
# The instantiations fpbn_pass_kernel<TMAX, STREAM, MODE> that the cases above do not reach (they run <2, false>, <4, true> and
# <8, true> in all four modes): <4, false>, <8, false> and <2, true>.  Each case has two layers, so that it runs all four modes
# (FWD_ROWS and BWD_MID need a second layer), at 2 x 65 rows (two workgroups, a tile that straddles two elements).
CLASSES = [case(4, 3, [64, 128], 2, 65), case(4, 3, [32, 256], 2, 65), case(512, 256, [64, 64], 2, 65)]
LENGTHS = (70, 33, 0)
OFFSET = 100.0
# every (case, rule, offset, biased, lengths) the GPU tests pick
PICKS = ([(k, "pointnet2", 0.0, True, None) for k in CASES + SMALL] + [(CASES[0], r, 0.0, True, None) for r in ("flownet3d", "given")] +
         [(CASES[0], "pointnet2", OFFSET, False, None), (CASES[0], "pointnet2", 0.0, True, LENGTHS)] +
         [(k, "pointnet2", 0.0, True, None) for k in CLASSES])


def composed(prep, l64):
    """torch's own composition over the live rows in the leaves' precision (float64 here; the GPU tests print its fp32 error beside
    the kernel's): conv2d, batch_norm(training=True), relu -> (out, [(mean, biased var)])."""
    x = fbr.blend_rows(l64[:prep.point_leaves()], prep.data, prep.rule, prep.rows).to(l64[0].dtype)
    h = x.T[None, :, :, None]                                              # (1, C, P, 1)
    stats = []
    for (w, b, gamma, beta), e in zip(prep.layer_leaves(l64), prep.eps):
        z = F.conv2d(h, w[:, :, None, None], b)
        stats.append((z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)))
        h = torch.relu(F.batch_norm(z, None, None, gamma, beta, True, 0.1, e))
    return h[0, :, :, 0].T, stats


@pytest.mark.parametrize("pick", [PICKS[0], PICKS[1], PICKS[6], PICKS[7], PICKS[8]], ids=lambda p: f"{case_id(p[0])}-{p[1]}-{p[2]}-{p[3]}-{p[4]}")
def test_reference_agrees_with_torchs_float64_composition(pick):
    prep = fbr.pick(*pick)
    out, stats, m, grads = fbr.exact(prep)
    l64 = [t.double().clone().requires_grad_(True) for t in prep.leaves]
    want, wstats = composed(prep, l64)
    wgrads = torch.autograd.grad(want, l64, prep.g[prep.rows])
    close = lambda a, b: (a - b).abs().max().item() <= 1e-10 * max(1.0, b.abs().max().item())
    assert m == len(prep.rows) and close(out[prep.rows], want.detach())
    for (mu, v), (wmu, wv) in zip(stats, wstats):
        assert close(mu, wmu.detach()) and close(v, wv.detach())
    for name, a, b in zip(prep.names, grads, wgrads):
        assert close(a, b), name
    for name, a in zip(prep.names, grads):
        if name[0] == "b" and name[1:].isdigit():
            assert a.abs().max().item() < 1e-10, f"{name}: the statistics absorb a bias, its gradient is zero in exact arithmetic"


@pytest.mark.parametrize("pick", PICKS, ids=lambda p: f"{case_id(p[0])}-{p[1]}-{p[2]}-{p[3]}-{p[4]}")
def test_every_gpu_case_finds_clear_inputs_within_a_few_hundred_seeds(pick):
    prep = fbr.pick(*pick)
    with torch.no_grad():
        _, (_, ys, _) = fbr.evaluate(prep)
    active = [float((y > 0).double().mean()) for y in ys]
    print(f"PICK {case_id(pick[0])}-{pick[1]} offset={pick[2]} biased={pick[3]} lengths={pick[4]} seed={prep.seed} tries={prep.tries} "
          f"min|y|={min(y.abs().min().item() for y in ys):.2e} active={' '.join(f'{a:.3f}' for a in active)}")
    assert fbr.clear(prep) and prep.tries <= 300
    assert all(0.25 < a < 0.75 for a in active), active


@pytest.mark.parametrize("momentum", [0.1, None])
def test_running_statistics_rule_is_batchnorm2ds(momentum):
    g = torch.Generator().manual_seed(3)
    bn = torch.nn.BatchNorm2d(16, momentum=momentum).double().train()
    rm, rv, tracked = bn.running_mean.clone(), bn.running_var.clone(), 0
    for step in range(3):
        z = torch.randn(2, 16, 37, 1, generator=g).double() * 3 + 1
        bn(z)
        rm, rv, tracked = fbr.running_update(rm, rv, tracked, momentum, z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False), 2 * 37)
        assert int(bn.num_batches_tracked) == tracked == step + 1
        assert torch.allclose(bn.running_mean, rm, rtol=1e-12, atol=1e-14) and torch.allclose(bn.running_var, rv, rtol=1e-12, atol=1e-14)


def test_naive_fp32_variance_fails_the_cancellation_case_and_two_pass_meets_it():
    """The inputs of the cancellation case (no conv bias, known_feats and skip offset by +100): relative to float64, over the channels
    of layer 1, fp32 E[z^2] - E[z]^2 misses C_CAP = 1.22e-4 on var_1 and a two-pass fp32 variance meets it."""
    prep = fbr.pick(CASES[0], "pointnet2", OFFSET, False, None)
    l64 = [t.double() for t in prep.leaves]
    z = (fbr.blend_rows(l64[:prep.point_leaves()], prep.data, prep.rule, prep.rows) @ prep.layer_leaves(l64)[0][0].T).numpy()
    exact = z.var(0)
    assert np.median(np.abs(z.mean(0)) / np.sqrt(exact)) > 30
    z32 = z.astype(np.float32)
    m = np.float32(len(z32))
    s1, s2 = np.float32(0) * z32[0], np.float32(0) * z32[0]
    for row in z32:                                                       # fp32 running sums, as a kernel would keep them
        s1 = s1 + row
        s2 = s2 + row * row
    naive = s2 / m - (s1 / m) * (s1 / m)
    mean = s1 / m
    d = z32 - mean
    acc = np.float32(0) * z32[0]
    for row in d:
        acc = acc + row * row
    two_pass = acc / m
    rel = lambda v: float(np.abs(v.astype(np.float64) - exact).max() / exact.max())
    print(f"CANCELLATION median |mu|/sigma={float(np.median(np.abs(z.mean(0)) / np.sqrt(exact))):.1f} naive={rel(naive):.3e} two_pass={rel(two_pass):.3e} C_CAP={C_CAP:.3e}")
    assert rel(naive) > C_CAP and rel(two_pass) <= C_CAP


def test_declarations_bindings_and_shape_predicate():
    decl = header_functions()
    for name, nargs in (("mcp_fp_mlp_bn_workspace_bytes", 7), ("mcp_fp_mlp_bn_forward", 26), ("mcp_fp_mlp_bn_backward", 31)):
        assert decl.get(name) == nargs, (name, decl.get(name))
        assert len(_lib.SIGNATURES[name]) == nargs
    assert _lib._RESTYPES["mcp_fp_mlp_bn_workspace_bytes"] is ctypes.c_size_t
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    for c2, c1, widths in ((4, 0, [32]), (64, 3, [64, 64]), (128, 4, [128, 128, 128]), (512, 256, [256, 256]), (256, 64, [256, 128])):
        assert ops.fp_mlp_bn_supported(c2, c1, widths) and lib.mcp_fp_mlp_bn_workspace_bytes(3, 70, c2, c1, len(widths), w(*widths), 1) > 0
    for c2, c1, widths in ((6, 0, [32]), (8, 0, [48]), (512, 260, [32]), (8, 4, [32, 32, 32, 32]), (0, 4, [32])):
        assert not ops.fp_mlp_bn_supported(c2, c1, widths)
        assert lib.mcp_fp_mlp_bn_workspace_bytes(3, 70, c2, c1, len(widths), w(*widths), 0) == 0
    fwd, bwd = (lib.mcp_fp_mlp_bn_workspace_bytes(3, 70, 64, 3, 2, w(64, 64), k) for k in (0, 1))
    assert fwd >= 4 * 210 * (64 + 64) and bwd >= fwd + 4 * 210 * (67 + 64 + 2 * (64 + 64) + 64 + 3)
    assert lib.mcp_fp_mlp_bn_workspace_bytes(0, 70, 64, 3, 2, w(64, 64), 1) == 0
    assert all(isinstance(v, int) and ops.fp_mlp_bn_supported(*k) for k, v in ops.FP_MLP_BN_FUSED_CLASSES.items())
    assert not ops.fp_mlp_bn_routes_fused(252, 3, [256, 256], 1 << 30), "a class without a measured row keeps the composition"
    assert not ops.fp_mlp_bn_routes_fused(64, 3, [64, 32], 600), "the existing module test's class must keep the composition under 'measured'"


def test_arguments_are_validated_without_a_gpu():
    """Null pointers, empty dimensions, a bad rule, eps <= 0 and misaligned buffers are refused on the host (10001); an unsupported
    shape is refused before any pointer is looked at (10002).  Nothing here launches: every pointer is a host buffer."""
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ptrs = (ctypes.c_void_p * 2)(base, base)
    nulls = (ctypes.c_void_p * 2)(None, None)
    eps = (ctypes.c_float * 2)(1e-5, 1e-5)

    def fwd(b=1, n=8, m=4, c2=8, c1=4, rule=1, layers=2, widths=w(32, 32), feats=base, skip=base, idx=base, dist=base, w3=None, packed=base, gamma=nulls,
            beta=nulls, eps=eps, out=base, mean=ptrs, var=ptrs, rstd=ptrs, count=base, ws=base, ws_bytes=0):
        return lib.mcp_fp_mlp_bn_forward(b, n, m, c2, c1, rule, layers, widths, feats, skip, idx, dist, w3, None, packed, gamma, beta, eps, out, mean, var, rstd,
                                         count, ws, ws_bytes, None)

    def bwd(b=1, n=8, m=4, c2=8, c1=4, rule=1, layers=2, widths=w(32, 32), feats=base, skip=base, gskip=base, dist=base, mean=ptrs, rstd=ptrs, g=base,
            order=None, gknown=None, gw=ptrs, ws=base, ws_bytes=0):
        return lib.mcp_fp_mlp_bn_backward(b, n, m, c2, c1, rule, layers, widths, feats, skip, base, dist, None, None, base, nulls, nulls, mean, rstd, g, order,
                                          None, gknown, gskip, gw, nulls, nulls, nulls, ws, ws_bytes, None)

    assert fwd() == 10001 and bwd() == 10001, "a workspace of 0 bytes is too small"
    for kw in (dict(b=0), dict(n=0), dict(m=0), dict(rule=3), dict(feats=None), dict(skip=None), dict(dist=None), dict(out=None), dict(count=None),
               dict(mean=nulls), dict(eps=(ctypes.c_float * 2)(1e-5, 0.0)), dict(feats=base + 4), dict(ws=None), dict(rule=0)):
        assert fwd(**kw) == 10001, kw
    for kw in (dict(b=0), dict(rule=-1), dict(feats=None), dict(skip=None), dict(gskip=None), dict(g=None), dict(gw=nulls), dict(rstd=nulls), dict(gknown=base),
               dict(g=base + 8)):
        assert bwd(**kw) == 10001, kw
    for kw in (dict(c2=6), dict(widths=w(32, 48)), dict(layers=4), dict(c1=513)):
        assert fwd(**kw) == 10002 and bwd(**kw) == 10002, kw
