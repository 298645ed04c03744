"""-m gpu: the feature-propagation layer under a training-mode BatchNorm (csrc/fp_mlp_bn.hip, ops.HipBackend.fp_mlp_bn_layer) and
PointnetFPModule's bn_route on top of it against the float64 statement of tests/fp_mlp_bn_reference.py.

Shapes: 64 + 3 -> 64/64 (every layer's slabs whole in LDS), 128 + 4 -> 128/128/128 (three layers), 256 + 64 -> 256/128 (streamed,
eight accumulator tiles) at B = 3, n = 70, m = 37 -- 210 rows: two workgroups, tiles crossing elements, a last wave of 18 rows; the
first shape also at (B, n) = (1, 5) and (2, 64): one partial wave, exactly one full workgroup; the three rules on the first shape.

Every case runs through be.fp_mlp_bn_layer with requires_grad leaves and every buffer the layer allocates refilled with NaN first.
The inputs are fp_mlp_bn_reference.pick's: every y_l of every live row is farther than 1e-4 from zero in float64 (asserted), so no
row is left out.  Asserted per case: the count, a second forward and a second backward with identical bits, finite values, exact
zeros in the rows of known_feats nobody gathers, and
    ratio = max |hip - exact| / (C max |exact|) <= 1
for out, every mean_l and var_l and every gradient (known_feats, skip, W, b, gamma, beta); a gradient that is zero in exact
arithmetic -- db_l always is: the statistics absorb a bias -- is held to the floor 2e-5.  Each case prints a RATIO line with the
relative errors themselves and those of torch's fp32 composition (conv2d, batch_norm(training=True), relu and autograd, on the CPU)
on the same inputs beside them."""
import copy

import pytest
import torch

from mocopci_amd import _lib, ops, pointnet2_utils as pu
from tests import fp_mlp_bn_reference as fbr
from tests import fused_reference as fr
from tests.test_fp_mlp_bn_cpu import CASES, CLASSES, LENGTHS, OFFSET, SMALL, composed
from tests.test_fp_mlp_grad_cpu import B, C_CAP, N, case_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
# This project's rule: the smallest power of two at least twice the worst relative error measured on the MI355X against float64
# (profiles/fp_mlp_bn_accuracy.txt holds every RATIO line), never above C_CAP = 2^-13.  Worst measured: 7.90e-07 (c64+3-64x64 at 1 x 5
# rows, grad_skip; the fp32 composition on the same inputs: 1.08e-06), 6.38e-07 through the module against its composition; twice
# that is 1.58e-06, between 2^-20 = 9.5e-07 and 2^-19 = 1.9e-06.  The cancellation case (|mu_1| about 127 sigma_1) measures 4.13e-05
# at its worst (w2; the fp32 composition: 7.15e-04 on w1, 6.51e-05 on gamma2): twice that lies between 2^-14 and 2^-13, the cap.
# The cases added later for the instantiations no other case runs (CLASSES) are held to the same 2^-19, which was not widened for them:
# their worst is 9.73e-07 (c512+256-64x64 at 2 x 65 rows, w2, 768 input channels; the fp32 composition there: 1.32e-06), 1.96 x below;
# c4+3-32x256 has the largest db against the floor 2e-5: 1.96e-05 (b1).
C_FP_MLP_BN = 2.0 ** -19
C_FP_MLP_BN_CANCELLATION = 2.0 ** -13
assert C_FP_MLP_BN <= C_FP_MLP_BN_CANCELLATION <= C_CAP


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.fixture
def nan_buffers(monkeypatch):
    """Every buffer the layer allocates starts as NaN (the byte workspace as 0xFF bytes: NaN in every float; int32 as -1)."""
    def poisoned(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        return t.fill_(255 if dtype == torch.uint8 else -1 if dtype == torch.int32 else NAN)
    monkeypatch.setattr(ops, "_grad_empty", poisoned)


def run_layer(prep, lengths=None, data=None, g=None):
    """(out, [(mean_l, var_l)], count, [gradient per leaf]) of be.fp_mlp_bn_layer; both directions run twice and must repeat bit for bit."""
    d = prep.data if data is None else data
    leaves = [t.to(DEV).requires_grad_(True) for t in prep.leaves]
    feats, skip = leaves[0], leaves[1] if prep.has_skip else None
    layers = [(*quad, e) for quad, e in zip(prep.layer_leaves(leaves), prep.eps)]
    idx, dist, w3 = dev(d["idx"], d["dist"], d["w3"])
    given = prep.rule == "given"
    call = lambda: ops.backend().fp_mlp_bn_layer(feats, skip, idx, None if given else dist, layers, rule=prep.rule, w3=w3 if given else None,
                                                 unknown_lengths=lengths)
    out, stats, count = call()
    out2, stats2, count2 = call()
    assert out.requires_grad and not count.requires_grad and not any(t.requires_grad for pair in stats for t in pair)
    assert torch.equal(out, out2) and torch.equal(count, count2), "a second forward gives other bits"
    for (a, b), (a2, b2) in zip(stats, stats2):
        assert torch.equal(a, a2) and torch.equal(b, b2), "a second forward gives other statistics"
    g = prep.g.float().view(out.shape).to(DEV) if g is None else g
    grads = torch.autograd.grad(out, leaves, g, retain_graph=True)
    again = torch.autograd.grad(out, leaves, g)
    for name, a, b in zip(prep.names, grads, again):
        assert torch.equal(a, b), f"{name}: a second backward gives other bits"
    return out.detach(), stats, count, list(grads)


def composed_fp32(prep):
    """torch's fp32 composition over the live rows on the CPU -> (out, stats, grads), for the figures printed beside the kernel's."""
    l32 = [t.clone().requires_grad_(True) for t in prep.leaves]
    out, stats = composed(prep, l32)
    grads = torch.autograd.grad(out, l32, prep.g[prep.rows].float(), allow_unused=True)
    return out.detach(), stats, [torch.zeros_like(t) if x is None else x for t, x in zip(l32, grads)]


def judge(name, prep, out, stats, count, grads, bound=C_FP_MLP_BN):
    assert fbr.clear(prep), "an input with a pre-activation within 1e-4 of zero"
    e_out, e_stats, m, e_grads = fbr.exact(prep)
    assert int(count.item()) == m
    c_out, c_stats, c_grads = composed_fp32(prep)
    c_full = torch.zeros_like(e_out)
    c_full[prep.rows] = c_out.double()
    got = [("out", out.cpu().view(e_out.shape), e_out, c_full)]
    for l, ((mu, v), (emu, ev), (cmu, cv)) in enumerate(zip(stats, e_stats, c_stats)):
        got += [(f"mean{l + 1}", mu.cpu(), emu, cmu.detach().double()), (f"var{l + 1}", v.cpu(), ev, cv.detach().double())]
    got += [(n, a.cpu(), e, c.double()) for n, a, e, c in zip(prep.names, grads, e_grads, c_grads)]
    line, worst = f"RATIO {name} seed={prep.seed}", []
    for n, a, e, c in got:
        assert torch.isfinite(a).all(), n
        r = fbr.ratio(a, e, bound)
        zero = e.abs().max().item() == 0 or (n[0] == "b" and n[1:].isdigit())
        if zero:   # zero in exact arithmetic (float64 leaves a rounding residue in db): the floor
            r = a.abs().max().item() / fbr.fgr.FLOOR
            line += f" {n}=floor:{a.abs().max().item():.2e}"
        else:
            line += f" {n}={fbr.ratio(a, e, 1.0):.2e}/{fbr.ratio(c, e, 1.0):.2e}"
        worst.append((r, n))
    print(line)
    r, n = max(worst)
    assert r <= 1.0, f"fp_mlp_bn {name}: {n} at {r:.2f} x the bound"


def check_case(k, rule, bound=C_FP_MLP_BN, **pick):
    prep = fbr.pick(k, rule, **pick)
    out, stats, count, grads = run_layer(prep)
    gathered = torch.zeros(k["b"], k["m"], dtype=torch.bool)
    gathered[torch.arange(k["b"])[:, None, None], prep.data["idx"].long()] = True
    assert (grads[0].cpu()[~gathered] == 0).all(), "a row of known_feats that nobody gathers has a non-zero gradient"
    judge(f"{case_id(k)}-{rule}" + ("-offset-nobias" if pick else ""), prep, out, stats, count, grads, bound)


@pytest.mark.parametrize("case_", CASES, ids=case_id)
def test_fp_mlp_bn_matches_float64(case_, nan_buffers):
    check_case(case_, "pointnet2")


@pytest.mark.parametrize("case_", SMALL + CLASSES, ids=case_id)   # CLASSES: the instantiations that CASES and SMALL do not reach
def test_fp_mlp_bn_partial_wave_and_full_workgroup(case_, nan_buffers):
    check_case(case_, "pointnet2")


@pytest.mark.parametrize("rule", ["flownet3d", "given"])
def test_fp_mlp_bn_other_rules_match_float64(rule, nan_buffers):
    check_case(CASES[0], rule)


def test_fp_mlp_bn_variance_survives_a_mean_a_hundred_sigmas_away(nan_buffers):
    """No conv bias, known_feats and skip offset by +100: the median |mu_1| / sigma_1 over the channels is 127.5.  On these inputs an
    fp32 E[z^2] - E[z]^2 is 4.47e-02 of max var_1 away from float64 -- 366 x C_CAP = 1.22e-04 -- and a two-pass fp32 variance
    2.46e-06 (tests/test_fp_mlp_bn_cpu.py emulates both).  Same check as every other case, with this case's own measured constant
    (2^-13, the cap: fp32 itself, not the variance, costs two digits when every h_0 is a hundred times its spread -- the fp32
    composition is 7.15e-04 away on w1).  The kernel's var_1 measures 6.18e-06."""
    check_case(CASES[0], "pointnet2", C_FP_MLP_BN_CANCELLATION, offset=OFFSET, biased=False)


def test_lengths_count_only_live_rows_and_read_nothing_from_padded_ones(nan_buffers):
    """unknown_lengths = (70, 33, 0): statistics and gradients are the float64 reference's over the 103 live rows; padded rows give
    zero outputs and a zero grad_skip; NaN in the padded rows of skip, grad_out and dist changes no bit."""
    k = CASES[0]
    prep = fbr.pick(k, "pointnet2", lengths=LENGTHS)
    out, stats, count, grads = run_layer(prep, lengths=list(LENGTHS))
    judge(f"{case_id(k)}-pointnet2-lengths", prep, out, stats, count, grads)
    d_skip = grads[1]
    d = dict(prep.data)
    skip, dist, g = prep.leaves[1].clone(), d["dist"].clone(), prep.g.float().view(B, N, -1).clone()
    for b, nu in enumerate(LENGTHS):
        assert (out[b, nu:] == 0).all() and (d_skip[b, nu:] == 0).all(), f"element {b}: padded rows are not exact zeros"
        skip[b, nu:] = NAN
        dist[b, nu:] = NAN
        g[b, nu:] = NAN
    poisoned = copy.copy(prep)
    poisoned.leaves = [prep.leaves[0], skip, *prep.leaves[2:]]
    out_p, stats_p, count_p, grads_p = run_layer(poisoned, lengths=list(LENGTHS), data=dict(d, dist=dist), g=g.to(DEV))
    assert torch.equal(out, out_p) and torch.equal(count, count_p)
    for (a, b), (a2, b2) in zip(stats, stats_p):
        assert torch.equal(a, a2) and torch.equal(b, b2)
    for name, a, b in zip(prep.names, grads, grads_p):
        assert torch.equal(a, b), f"{name}: a padded row's NaN reached it"


# ---- module ----------------------------------------------------------------------------------------------------------------------------
MB, MN, MM, MC2, MC1 = 2, 300, 80, 64, 3   # the geometry of tests/test_fp_mlp_grad_gpu.py's module tests


def fp_module(g, momentum):
    from mocopci_amd.pointnet2_modules import PointnetFPModule
    m = PointnetFPModule(mlp=[MC2 + MC1, 64, 32], bn=True)
    state = {}
    for k, v in m.state_dict().items():
        shape = list(v.shape)
        if k.endswith("conv.weight"):
            state[k] = torch.randn(shape, generator=g) * (2.0 / shape[1]) ** 0.5
        elif k.endswith("num_batches_tracked"):
            state[k] = torch.tensor(3)
        elif k.endswith("running_var"):
            state[k] = torch.rand(shape, generator=g) + 0.5
        elif k.endswith("bn.weight"):
            state[k] = torch.rand(shape, generator=g) + 1.5
        else:
            state[k] = torch.randn(shape, generator=g) * 0.3
    m.load_state_dict(state, strict=True)
    for unit in m.mlp.children():
        unit.bn.bn.momentum = momentum
    return m.train()


def module_inputs():
    g = torch.Generator().manual_seed(31)
    known = fr.clustered_cloud(g, MB, MM, 16)
    unknown = (known[:, torch.arange(MN) * MM // MN] + 0.3 * torch.randn(MB, MN, 3, generator=g)).contiguous()
    return unknown, known, torch.randn(MB, MC1, MN, generator=g) + 0.5, torch.randn(MB, MC2, MM, generator=g) + 0.5


def module_float64(m, skip, feats, idx, dist, G, grad):
    """Float64 <module(row), G[row]> over all rows from float64 copies of the parameters -> (clear, gradients for unknow_feats,
    known_feats and every parameter, in m.parameters() order)."""
    convs, bns = m._layers()
    params, layers = [], []
    for c, bn in zip(convs, bns):
        quad = [c.weight.detach().cpu().double().flatten(1), bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double()]
        quad = [t.requires_grad_(grad) for t in quad]
        params += quad
        layers.append((quad[0], None, quad[1], quad[2]))
    s64 = skip.transpose(1, 2).contiguous().double().requires_grad_(grad)
    f64 = feats.transpose(1, 2).contiguous().double().requires_grad_(grad)
    d = dict(known_feats=f64, skip=s64, idx=idx, dist=dist, w3=None)
    x = fbr.blend_rows([f64, s64], d, m.weighting, torch.arange(MB * MN))
    out, ys, _ = fbr.forward(x, layers, [bn.eps for bn in bns])
    clear = min(y.abs().min().item() for y in ys) > fbr.CLEAR
    if not grad:
        return clear, None
    got = torch.autograd.grad(out, [s64, f64, *params], G)
    return clear, [got[0].transpose(1, 2), got[1].transpose(1, 2)] + [e.view(p.shape) for e, p in zip(got[2:], m.parameters())]


def module_grads(m, u, k, s, f, G, kw):
    s, f = s.clone().requires_grad_(True), f.clone().requires_grad_(True)
    out = m(u, k, s, f, **kw)
    return out.detach(), list(torch.autograd.grad(out, [s, f, *m.parameters()], G))


def buffers(m):
    return {k: v.detach().clone() for k, v in m.named_buffers()}


@pytest.mark.parametrize("momentum", [0.1, None], ids=["momentum0.1", "cumulative"])
def test_fp_module_bn_route_against_its_composition_and_float64(momentum, nan_buffers, monkeypatch):
    unknown, known, skip, feats = module_inputs()
    u, k, s, f = dev(unknown, known, skip, feats)
    with torch.no_grad():
        dist, idx = pu.three_nn(u, k)
    dist, idx = dist.cpu(), idx.cpu()
    for t in range(fbr.TRIES):   # the first parameter seed that keeps every y_l clear of zero
        m = fp_module(torch.Generator().manual_seed(2000 + t), momentum)
        if module_float64(m, skip, feats, idx, dist, None, False)[0]:
            break
    else:
        raise AssertionError("no clear module parameters")
    G64 = torch.randn(MB * MN, 32, generator=torch.Generator().manual_seed(99)).double()
    clear, exact = module_float64(m, skip, feats, idx, dist, G64, True)
    assert clear
    G = G64.float().view(MB, MN, 32).transpose(1, 2).contiguous().to(DEV)
    fused, comp = copy.deepcopy(m).to(DEV), copy.deepcopy(m).to(DEV)
    fused.bn_route, comp.bn_route = "always", "never"
    out_c, grads_c = module_grads(comp, u, k, s, f, G, {})

    def boom(*a, **kw):
        raise AssertionError("the composition was taken")
    real = pu.three_interpolate
    monkeypatch.setattr(pu, "three_interpolate", boom)
    out_f, grads_f = module_grads(fused, u, k, s, f, G, {})
    monkeypatch.setattr(pu, "three_interpolate", real)
    assert torch.allclose(out_f, out_c, rtol=1e-4, atol=1e-5)
    names = ["unknow_feats", "known_feats"] + [n for n, _ in m.named_parameters()]
    line = f"RATIO module-{'cumulative' if momentum is None else 'momentum'} try={t + 1}"
    for name, a, c, e in zip(names, grads_f, grads_c, exact):
        assert torch.isfinite(a).all(), name
        r, rc, r2 = (fbr.ratio(x, y, C_FP_MLP_BN) for x, y in ((a.cpu(), e), (c.cpu(), e), (a.cpu(), c.cpu().double())))
        line += f" {name}={fbr.ratio(a.cpu(), e, 1.0):.2e}/{fbr.ratio(c.cpu(), e, 1.0):.2e}/{fbr.ratio(a.cpu(), c.cpu().double(), 1.0):.2e}"
        assert r <= 1.0 and r2 <= 1.0, f"{name}: {r:.2f} x the bound against float64, {r2:.2f} x against the module's composition"

    def same_buffers(step):
        nonlocal line
        bf, bc = buffers(fused), buffers(comp)
        for key in bc:
            if key.endswith("num_batches_tracked"):
                assert int(bf[key]) == int(bc[key]) == 3 + step, key
            else:
                r = fbr.ratio(bf[key].cpu(), bc[key].cpu().double(), C_FP_MLP_BN)
                line += f" {key.split('.')[0]}.{key.split('.')[-1]}@{step}={fbr.ratio(bf[key].cpu(), bc[key].cpu().double(), 1.0):.2e}"
                assert r <= 1.0, f"{key} after {step} call(s): {r:.2f} x the bound from the composition's"
    same_buffers(1)
    with torch.no_grad():   # a forward without a wanted gradient still takes the route and still updates the running statistics
        monkeypatch.setattr(pu, "three_interpolate", boom)
        out_f2 = fused(u, k, s, f)
        monkeypatch.setattr(pu, "three_interpolate", real)
        out_c2 = comp(u, k, s, f)
    assert torch.equal(out_f2, out_f) and torch.allclose(out_f2, out_c2, rtol=1e-4, atol=1e-5)
    same_buffers(2)
    print(line)


def test_fp_module_keeps_the_composition_with_lengths_or_an_unmeasured_class(monkeypatch):
    unknown, known, skip, feats = module_inputs()
    u, k, s, f = dev(unknown, known, skip, feats)
    m = fp_module(torch.Generator().manual_seed(5), 0.1).to(DEV)

    def boom(self, *a, **kw):
        raise AssertionError("the fused route with batch statistics was taken")
    monkeypatch.setattr(ops.HipBackend, "fp_mlp_bn_layer", boom)
    G = torch.randn(MB, 32, MN, generator=torch.Generator().manual_seed(1)).to(DEV)
    m.bn_route = "always"
    with pytest.raises(AssertionError, match="batch statistics"):
        module_grads(m, u, k, s, f, G, {})
    out, grads = module_grads(m, u, k, s, f, G, dict(unknown_lengths=[300, 120], known_lengths=[80, 2]))
    assert torch.isfinite(out).all() and all(torch.isfinite(t).all() for t in grads)
    m.bn_route = "measured"
    assert not ops.fp_mlp_bn_routes_fused(MC2, MC1, [64, 32], MB * MN)
    out, grads = module_grads(m, u, k, s, f, G, {})
    assert torch.isfinite(out).all() and all(torch.isfinite(t).all() for t in grads)
    m.bn_route = "always"
    m.eval()
    assert torch.isfinite(module_grads(m, u, k, s, f, G, {})[0]).all(), "eval() is not the route's"


def test_unsupported_shapes_launch_nothing():
    import ctypes
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    feats, skip = torch.zeros(1, 4, 8, device=DEV), torch.zeros(1, 8, 4, device=DEV)
    idx, dist = torch.zeros(1, 8, 3, dtype=torch.int32, device=DEV), torch.ones(1, 8, 3, device=DEV)
    buf = torch.full((1 << 16,), 7.0, device=DEV)
    g = torch.zeros(1, 8, 48, device=DEV)
    p, i = _lib.fptr, _lib.iptr
    four = lambda: (ctypes.c_void_p * 4)(*[p(buf)] * 4)
    eps = (ctypes.c_float * 4)(1e-5, 1e-5, 1e-5, 1e-5)
    for c2, c1, widths in ((6, 0, (32,)), (8, 0, (48,)), (8, 4, (32, 32, 32, 32))):
        rc = lib.mcp_fp_mlp_bn_forward(1, 8, 4, c2, c1, 1, len(widths), w(*widths), p(feats), p(skip), i(idx), p(dist), None, None, p(buf), four(), four(), eps,
                                       p(buf), four(), four(), four(), buf.data_ptr(), buf.data_ptr(), buf.numel() * 4, None)
        assert rc == 10002, (c2, c1, widths, rc)
        rc = lib.mcp_fp_mlp_bn_backward(1, 8, 4, c2, c1, 1, len(widths), w(*widths), p(feats), p(skip), i(idx), p(dist), None, None, p(buf), four(), four(),
                                        four(), four(), p(g), None, None, None, p(buf), four(), four(), four(), four(), buf.data_ptr(), buf.numel() * 4, None)
        assert rc == 10002, (c2, c1, widths, rc)
    torch.cuda.synchronize()
    assert (buf == 7.0).all()
    with pytest.raises(_lib.Unsupported):
        ops.backend().fp_mlp_bn_layer(feats, None, idx, dist, [(torch.zeros(48, 8, device=DEV), None, None, None, 1e-5)])
