"""-m gpu: the backward of the fused feature-propagation layer (csrc/fp_mlp_grad.hip, ops.HipBackend.fp_mlp_layer / fp_mlp_grad) and
PointnetFPModule's differentiable fused route against the float64 gradients of tests/fp_mlp_grad_reference.py.

Shapes: B = 3, n = 70, m = 37 over the forward's twelve shapes -- 210 rows: two workgroups, tiles crossing elements, a last wave of
18 rows; (B, n) = (1, 5) and (2, 64) on a narrow and a wide shape -- one partial wave beside three dead ones, exactly one full
workgroup; the three rules on the OTHER_RULES shapes.  The kernel does not loop persistently (one workgroup per 128 rows), so there
is no grid cap to step over.

Every case runs through be.fp_mlp_layer with requires_grad leaves and with every buffer the backward allocates refilled with NaN
first, and asserts: finite gradients, a second backward with identical bits, exact zeros in the rows of known_feats nobody gathers,
the recomputed out equal to be.fp_mlp bit for bit, and
    ratio = max |hip - exact| / (C max |exact|) <= 1
per group -- (a) the per-point gradients, (b) the weight and bias gradients -- the largest ratio over the group's tensors; a gradient
that is zero in exact arithmetic is held to the floor 2e-5.  Each case prints its RATIO line with the relative errors themselves and
the fp32 composition's (autograd over fp_mlp_reference.composition on the device) beside them."""
import functools

import pytest
import torch

from mocopci_amd import _lib, ops, pointnet2_utils as pu
from tests import fp_mlp_grad_reference as fgr
from tests import fp_mlp_reference as fpr
from tests import fused_reference as fr
from tests.test_fp_mlp_grad_cpu import B, CASES, C_CAP, M, N, OTHER_RULES, SMALL, case, case_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
# This project's rule: the smallest power of two at least twice the worst relative error measured on the MI355X against float64
# (profiles/fp_mlp_grad_accuracy.txt holds every RATIO line), never above C_CAP = 2^-13, the loosest constant any backward here carries.
# Worst measured: 6.06e-07 (c512+256-256x256, pointnet2, per-point gradients; the fp32 composition on the same inputs: 3.08e-07, and
# 4.66e-07 at its own worst), 5.36e-07 on a weight gradient (c64+64-32x256); through the module about 6e-07.  Twice that is 1.21e-06,
# between 2^-20 = 9.5e-07 and 2^-19 = 1.9e-06.
C_FP_MLP_GRAD = 2.0 ** -19
assert C_FP_MLP_GRAD <= C_CAP


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.fixture
def nan_buffers(monkeypatch):
    """Every buffer the backward allocates starts as NaN (the byte workspace as 0xFF bytes: NaN in every float)."""
    def poisoned(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        return t.fill_(255 if dtype == torch.uint8 else NAN)
    monkeypatch.setattr(ops, "_grad_empty", poisoned)


@functools.lru_cache(maxsize=None)
def prepared(key, rule):
    prep = fgr.prepare(dict(b=key[0], n=key[1], m=key[2], c2=key[3], c1=key[4], widths=list(key[5])), rule)
    return prep, fgr.gradients(prep)


def case_prepared(k, rule):
    return prepared((k["b"], k["n"], k["m"], k["c2"], k["c1"], tuple(k["widths"])), rule)


def device_leaves(prep):
    return [t.to(DEV).requires_grad_(True) for t in prep.leaves]


def split(prep, leaves):
    skip = leaves[1] if prep.has_skip else None
    wb = leaves[prep.point_leaves():]
    return leaves[0], skip, list(zip(wb[0::2], wb[1::2]))


def run_layer(prep, lengths=None, g=None):
    """(out, [gradient per leaf]) of be.fp_mlp_layer on the prepared data."""
    d = prep.data
    leaves = device_leaves(prep)
    feats, skip, weights = split(prep, leaves)
    idx, dist, w3 = dev(d["idx"], d["dist"], d["w3"])
    given = prep.rule == "given"
    out = ops.backend().fp_mlp_layer(feats, skip, idx, None if given else dist, weights, rule=prep.rule, w3=w3 if given else None, unknown_lengths=lengths)
    assert out.requires_grad
    g = prep.g.float().view(out.shape).to(DEV) if g is None else g
    grads = torch.autograd.grad(out, leaves, g, retain_graph=True)
    again = torch.autograd.grad(out, leaves, g)
    for name, a, b in zip(prep.names, grads, again):
        assert torch.equal(a, b), f"{name}: a second backward gives other bits"
    return out.detach(), list(grads)


def composed_grads(prep, rows=None):
    """fp32 autograd over the composition on the device, for the figure printed beside the kernel's."""
    d = prep.data
    leaves = device_leaves(prep)
    feats, skip, weights = split(prep, leaves)
    idx, dist, w3 = dev(d["idx"], d["dist"], d["w3"])
    out = fpr.composition(feats, skip, idx, dist, weights, rule=prep.rule, w3=w3)
    g = prep.g.float().view(out.shape).to(DEV)
    return list(torch.autograd.grad(out, leaves, g))


def judge(name, prep, grads, exact, composed=None):
    worst = {}
    line = f"RATIO {name}"
    for group, span in (("points", range(prep.point_leaves())), ("weights", range(prep.point_leaves(), len(prep.names)))):
        ratios = [fgr.ratio(grads[i].cpu(), exact[i], C_FP_MLP_GRAD) for i in span]
        rel = max(fgr.ratio(grads[i].cpu(), exact[i], 1.0) for i in span if exact[i].abs().max() > 0) if any(exact[i].abs().max() > 0 for i in span) else 0.0
        worst[group] = max(ratios)
        line += f" {group}={max(ratios):.3f} (rel {rel:.3e}"
        if composed is not None:
            crel = max(fgr.ratio(composed[i].cpu(), exact[i], 1.0) for i in span if exact[i].abs().max() > 0)
            line += f", composed_fp32 {crel:.3e}"
        line += ")"
    print(line)
    for t in grads:
        assert torch.isfinite(t).all()
    for group, r in worst.items():
        assert r <= 1.0, f"fp_mlp_grad {name}: {group} gradients at {r:.2f} x the bound"


def check_case(k, rule):
    prep, exact = case_prepared(k, rule)
    d = prep.data
    out, grads = run_layer(prep)
    be = ops.backend()
    feats, skip, weights = split(prep, [t.to(DEV) for t in prep.leaves])
    idx, dist, w3 = dev(d["idx"], d["dist"], d["w3"])
    given = rule == "given"
    packed, widths = ops.fp_mlp_pack_weights(weights, k["c2"])
    fwd = be.fp_mlp(feats, skip, idx, None if given else dist, packed, widths, rule=rule, w3=w3 if given else None)
    assert torch.equal(out, fwd)
    raw = be.fp_mlp_grad(feats, skip, idx, None if given else dist, weights, prep.g.float().view(out.shape).to(DEV), rule=rule, w3=w3 if given else None,
                         recompute_out=True)
    assert torch.equal(raw[4], fwd), "the recomputed out differs from mcp_fp_mlp's"
    assert torch.equal(raw[0], grads[0]) and all(torch.equal(a, b) for a, b in zip(raw[2], grads[prep.point_leaves()::2]))
    gathered = torch.zeros(k["b"], k["m"], dtype=torch.bool)
    gathered[torch.arange(k["b"])[:, None, None], d["idx"].long()] = True
    assert (grads[0].cpu()[~gathered] == 0).all(), "a row of known_feats that nobody gathers has a non-zero gradient"
    judge(f"{case_id(k)}-{rule}", prep, grads, exact, composed_grads(prep))


@pytest.mark.parametrize("case_", CASES, ids=case_id)
def test_fp_mlp_grad_matches_float64(case_, nan_buffers):
    check_case(case_, "pointnet2")


@pytest.mark.parametrize("case_", SMALL, ids=case_id)
def test_fp_mlp_grad_partial_wave_and_full_workgroup(case_, nan_buffers):
    check_case(case_, "pointnet2")


@pytest.mark.parametrize("rule", ["flownet3d", "given"])
@pytest.mark.parametrize("case_", OTHER_RULES, ids=case_id)
def test_fp_mlp_grad_other_rules_match_float64(case_, rule, nan_buffers):
    check_case(case_, rule)


def test_without_a_wanted_gradient_the_layer_is_the_forward():
    prep, _ = case_prepared(CASES[2], "pointnet2")
    d = prep.data
    feats, skip, weights = split(prep, [t.to(DEV) for t in prep.leaves])
    idx, dist = dev(d["idx"], d["dist"])
    out = ops.backend().fp_mlp_layer(feats, skip, idx, dist, weights)
    assert not out.requires_grad
    assert torch.equal(out, ops.backend().fp_mlp(feats, skip, idx, dist, *ops.fp_mlp_pack_weights(weights, CASES[2]["c2"])))
    with torch.no_grad():
        leaves = device_leaves(prep)
        f2, s2, w2 = split(prep, leaves)
        assert torch.equal(ops.backend().fp_mlp_layer(f2, s2, idx, dist, w2), out)


# ---- lengths ---------------------------------------------------------------------------------------------------------------------------
LEN_CASES = [case(64, 3, [64, 64]), case(256, 64, [256, 128])]


def searched(d, ulen, klen):
    """dist / idx of pu.three_nn under the lengths, and the inputs with every padded row poisoned (idx stays 0 there)."""
    u, k = dev(d["unknown"], d["known"])
    dist, idx = pu.three_nn(u, k, list(ulen), list(klen))
    dist, idx = dist.cpu(), idx.cpu()
    feats, skip = d["known_feats"].clone(), None if d["skip"] is None else d["skip"].clone()
    for b, (nu, nk) in enumerate(zip(ulen, klen)):
        feats[b, nk:] = NAN
        dist[b, nu:] = NAN
        if skip is not None:
            skip[b, nu:] = NAN
    return dict(d, known_feats=feats, skip=skip, dist=dist.contiguous(), idx=idx.contiguous())


def sliced(prep, t, b, nu, nk, **repl):
    part = {k: None if t[k] is None else t[k][b:b + 1, :nu].contiguous() for k in ("skip", "idx", "dist", "w3")}
    part["known_feats"] = t["known_feats"][b:b + 1, :max(nk, 1)].contiguous()
    data = {**t, **part, **repl}
    return fgr.Prepared(data, prep.rule, prep.names, [data["known_feats"]] + ([data["skip"]] if prep.has_skip else []) + prep.leaves[prep.point_leaves():],
                        None, None, None)


@pytest.mark.parametrize("rule", ["pointnet2", "flownet3d"])
@pytest.mark.parametrize("case_", LEN_CASES, ids=case_id)
def test_lengths_give_the_sliced_call_and_nothing_from_padded_rows(case_, rule, nan_buffers):
    """Unknown lengths (70, 41, 9) over known lengths (37, 2, 0); padded rows of skip, known_feats, dist and g hold NaN.  The live
    per-point gradients equal, bit for bit, those of the call on the element's sliced prefixes; padded rows of grad_skip are zeros;
    the element with two known points has one +inf slot, which sends nothing anywhere (pointing it at another row changes no bit);
    the element without a known point gives grad_known_feats = 0 and the grad_skip of [0 | skip]."""
    ulen, klen = (70, 41, 9), (37, 2, 0)
    d = fgr.grad_inputs(case_)
    t = searched(d, ulen, klen)
    assert torch.isinf(t["dist"][1, :41, 2]).all() and torch.isfinite(t["dist"][1, :41, :2]).all() and torch.isinf(t["dist"][2, :9]).all()
    live = torch.cat([torch.arange(nu) + b * N for b, nu in enumerate(ulen)])
    prep = fgr.prepare(rule=rule, data=t, rows=live)
    assert prep.clear[live].double().mean() > 0.9 and not prep.clear.index_fill(0, live, False).any()
    g = prep.g.float().view(B, N, -1).clone()
    for b, nu in enumerate(ulen):
        g[b, nu:] = NAN
    g = g.to(DEV)
    out, grads = run_layer(prep, lengths=list(ulen), g=g)
    for x in grads:
        assert torch.isfinite(x).all()
    d_known, d_skip = grads[0], grads[1]
    for b, (nu, nk) in enumerate(zip(ulen, klen)):
        assert (d_skip[b, nu:] == 0).all() and (out[b, nu:] == 0).all(), f"element {b}: padded rows are not exact zeros"
        _, part = run_layer(sliced(prep, t, b, nu, nk), g=g[b:b + 1, :nu].contiguous())
        assert torch.equal(part[1][0], d_skip[b, :nu]), f"element {b}: grad_skip differs from the sliced call"
        assert torch.equal(part[0][0], d_known[b, :max(nk, 1)]), f"element {b}: grad_known_feats differs from the sliced call"
        assert (d_known[b, max(nk, 1):] == 0).all()
    moved = t["idx"].clone()
    moved[1, :41, 2] = 5   # the infinite slot pointed at a poisoned row that nobody else gathers
    _, other = run_layer(fgr.Prepared(dict(t, idx=moved), rule, prep.names, prep.leaves, prep.clear, prep.g, None), lengths=list(ulen), g=g)
    for name, a, b in zip(prep.names, grads, other):
        assert torch.equal(a, b), f"{name}: the infinite slot sends something"
    assert (d_known[2] == 0).all(), "an element without a known point has a gradient for known_feats"
    zero = sliced(prep, t, 2, 9, 0, known_feats=torch.zeros(1, 1, case_["c2"]), dist=torch.ones(1, 9, 3))
    assert torch.equal(run_layer(zero, g=g[2:3, :9].contiguous())[1][1][0], d_skip[2, :9]), "grad_skip is not that of [0 | skip]"
    judge(f"{case_id(case_)}-{rule}-lengths", prep, grads, fgr.gradients(prep))


# ---- module ----------------------------------------------------------------------------------------------------------------------------
MB, MN, MM, MC2, MC1 = 2, 300, 80, 64, 3


def fp_module(g, bn):
    from mocopci_amd.pointnet2_modules import PointnetFPModule
    m = PointnetFPModule(mlp=[MC2 + MC1, 64, 32], bn=bn)
    state = {}
    for k, v in m.state_dict().items():
        shape = list(v.shape)
        if k.endswith("conv.weight"):
            state[k] = torch.randn(shape, generator=g) * (2.0 / shape[1]) ** 0.5
        elif k.endswith("num_batches_tracked"):
            state[k] = torch.tensor(3)
        elif k.endswith("running_var") or k.endswith("bn.weight"):
            state[k] = torch.rand(shape, generator=g) + 0.5
        else:
            state[k] = torch.randn(shape, generator=g) * 0.1
    m.load_state_dict(state, strict=True)
    return m.to(DEV)


def module_inputs(g):
    known = fr.clustered_cloud(g, MB, MM, 16)
    unknown = (known[:, torch.arange(MN) * MM // MN] + 0.3 * torch.randn(MB, MN, 3, generator=g)).contiguous()
    return unknown, known, torch.randn(MB, MC1, MN, generator=g) + 0.5, torch.randn(MB, MC2, MM, generator=g) + 0.5


def module_grads(m, u, k, s, f, G, kw):
    s, f = s.clone().requires_grad_(True), f.clone().requires_grad_(True)
    params = list(m.parameters())
    out = m(u, k, s, f, **kw)
    return out.detach(), list(torch.autograd.grad(out, [s, f, *params], G))


def module_float64(m, rows_f, rows_s, idx, dist, rule, live, G):
    """Float64 gradients of <module(row), G[row]> over the live rows for (unknow_feats, known_feats, parameters...): the fold in
    float64 as an autograd function of float64 copies of the parameters, then fp_mlp_grad_reference.layer."""
    convs, bns = m._layers()
    params, folded = [], []
    for c, bn in zip(convs, bns):
        w = c.weight.detach().cpu().double().flatten(1).requires_grad_(True)
        params.append(w)
        b = w.new_zeros(w.shape[0])
        if c.bias is not None:
            b = c.bias.detach().cpu().double().requires_grad_(True)
            params.append(b)
        if bn is not None:
            gam, beta = bn.weight.detach().cpu().double().requires_grad_(True), bn.bias.detach().cpu().double().requires_grad_(True)
            params += [gam, beta]
            scale = gam / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)
            w, b = w * scale[:, None], (b - bn.running_mean.detach().cpu().double()) * scale + beta
        folded += [w, b]
    f64, s64 = rows_f.double().requires_grad_(True), rows_s.double().requires_grad_(True)
    d = dict(known_feats=rows_f, skip=rows_s, idx=idx, dist=dist, w3=None)
    out, zs = fgr.layer([f64, s64, *folded], d, rule, live)
    clear = torch.stack([(z.abs() > fgr.CLEAR).all(-1) for z in zs]).all(0)
    got = torch.autograd.grad(out, [s64, f64, *params], G[live] * clear[:, None])
    return clear, got


@pytest.mark.parametrize("lengths", [None, ((300, 120), (80, 2))], ids=["full", "short"])
@pytest.mark.parametrize("mode", ["eval-bn", "train-no-bn"])
def test_fp_module_fused_backward_against_its_composition_and_float64(mode, lengths, nan_buffers):
    g = torch.Generator().manual_seed(31)
    bn = mode == "eval-bn"
    m = fp_module(g, bn)
    m = m.eval() if bn else m.train()
    m.grad_route = "always"
    unknown, known, skip, feats = module_inputs(g)
    kw = {} if lengths is None else dict(unknown_lengths=list(lengths[0]), known_lengths=list(lengths[1]))
    u, k, s, f = dev(unknown, known, skip, feats)
    with torch.no_grad():
        dist, idx = pu.three_nn(u, k, *(None, None) if lengths is None else (list(lengths[0]), list(lengths[1])))
    nu_all = (MN,) * MB if lengths is None else lengths[0]
    live = torch.cat([torch.arange(nu) + b * MN for b, nu in enumerate(nu_all)])
    G64 = torch.randn(MB * MN, 32, generator=torch.Generator().manual_seed(99)).double()
    rows_f, rows_s = feats.transpose(1, 2).contiguous(), skip.transpose(1, 2).contiguous()
    clear, exact = module_float64(m, rows_f, rows_s, idx.cpu(), dist.cpu(), m.weighting, live, G64)
    assert clear.double().mean() > 0.9
    Gm = torch.zeros(MB * MN, 32, dtype=torch.float64)
    Gm[live] = G64[live] * clear[:, None]
    G = Gm.float().view(MB, MN, 32).transpose(1, 2).contiguous().to(DEV)
    out, fused = module_grads(m, u, k, s, f, G, kw)
    m.grad_route = "never"
    out_c, composed = module_grads(m, u, k, s, f, G, kw)
    assert torch.allclose(out, out_c, rtol=1e-4, atol=1e-5)
    names = ["unknow_feats", "known_feats"] + [n for n, _ in m.named_parameters()]
    exact = [exact[0].transpose(1, 2), exact[1].transpose(1, 2)] + [e.view(p.shape) for e, p in zip(exact[2:], m.parameters())]
    line = f"RATIO module-{mode}-{'full' if lengths is None else 'short'}"
    for name, a, c, e in zip(names, fused, composed, exact):
        assert torch.isfinite(a).all(), name
        r, rc = fgr.ratio(a.cpu(), e, C_FP_MLP_GRAD), fgr.ratio(c.cpu(), e, C_FP_MLP_GRAD)
        r2 = fgr.ratio(a.cpu(), c.cpu().double(), C_FP_MLP_GRAD)
        line += f" {name}={r:.3f}/{rc:.3f}/{r2:.3f}"
        assert r <= 1.0 and r2 <= 1.0, f"{name}: {r:.2f} x the bound against float64, {r2:.2f} x against the module's composition"
    print(line)


def test_fp_module_keeps_the_composition_when_it_must(monkeypatch):
    """grad_route = "measured" with a class absent from the table, and a training-mode BatchNorm under "always", take the
    composition: a fused layer that raises proves it."""
    g = torch.Generator().manual_seed(32)
    m = fp_module(g, True).eval()
    u, k, s, f = dev(*module_inputs(g))
    G = torch.randn(MB, 32, MN, generator=g).to(DEV)
    m.grad_route = "never"
    out_c, composed = module_grads(m, u, k, s, f, G, {})

    def boom(self, *a, **kw):
        raise AssertionError("the fused differentiable route was taken")
    monkeypatch.setattr(ops.HipBackend, "fp_mlp_layer", boom)
    m.grad_route = "always"
    with pytest.raises(AssertionError, match="fused differentiable route"):
        module_grads(m, u, k, s, f, G, {})
    m.grad_route = "measured"
    assert not ops.fp_mlp_grad_routes_fused(MC2, MC1, [64, 32], MB * MN)
    out_m, measured = module_grads(m, u, k, s, f, G, {})
    # (the composition's own backward does not repeat bit for bit: its library convolutions sum in no fixed order)
    assert torch.equal(out_m, out_c) and all(torch.allclose(a, b, rtol=1e-4, atol=1e-6) for a, b in zip(measured, composed))
    m.grad_route = "always"
    m.train()
    out_t, trained = module_grads(m, u, k, s, f, G, {})
    assert torch.isfinite(out_t).all() and all(torch.isfinite(t).all() for t in trained)


def test_unsupported_shapes_launch_nothing():
    import ctypes
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    feats, skip = torch.zeros(1, 4, 8, device=DEV), torch.zeros(1, 8, 4, device=DEV)
    idx, dist = torch.zeros(1, 8, 3, dtype=torch.int32, device=DEV), torch.ones(1, 8, 3, device=DEV)
    buf = torch.full((1 << 16,), 7.0, device=DEV)
    g = torch.zeros(1, 8, 48, device=DEV)
    p, i = _lib.fptr, _lib.iptr
    ptrs = (ctypes.c_void_p * 1)(p(buf))
    for c2, c1, widths in ((6, 0, (32,)), (8, 0, (48,)), (8, 4, (32, 32, 32, 32))):
        rc = lib.mcp_fp_mlp_grad(1, 8, 4, c2, c1, 1, len(widths), w(*widths), p(feats), p(skip), i(idx), p(dist), None, None, p(buf), p(g), None, None, None,
                                 p(buf), ptrs, ptrs, None, buf.data_ptr(), buf.numel() * 4, None)
        assert rc == 10002, (c2, c1, widths, rc)
    torch.cuda.synchronize()
    assert (buf == 7.0).all()
    with pytest.raises(_lib.Unsupported):
        ops.backend().fp_mlp_grad(feats, None, idx, dist, [(torch.zeros(48, 8, device=DEV), torch.zeros(48, device=DEV))], g)
