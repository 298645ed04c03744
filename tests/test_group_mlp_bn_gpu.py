"""-m gpu: the set-abstraction layer under a training-mode BatchNorm (csrc/group_mlp_bn.hip, ops.HipBackend.group_mlp_bn_layer) and
PointnetSAModuleMSG's bn_route on top of it against the float64 statement of tests/group_mlp_bn_reference.py.

Shapes: tests/test_group_mlp_bn_cpu.py's CASES and FURTHER (it states which loop edge, register class and staging each one reaches).

Every case runs through be.group_mlp_bn_layer with requires_grad leaves and every buffer the layer allocates refilled with NaN first.
The inputs are group_mlp_bn_reference.pick's: every y_l of every live pair is farther than 1e-4 from zero in float64 (asserted), so no
pair is left out; the upstream gradient is zero where the pool's winner is not clear among different points.  Asserted per case: the
count, a second forward and a second backward with identical bits, finite values, exact zeros in the rows of features / xyz that no
slot gathers, and
    ratio = max |hip - exact| / (C max |exact|) <= 1
for out, every mean_l and var_l and every gradient (features, xyz, new_xyz, W, b, gamma, beta); a gradient that is zero in exact
arithmetic -- db_l always is: the statistics absorb a bias -- is held to the floor 2e-5.  Each case prints a RATIO line with the
relative errors themselves and those of torch's fp32 composition (conv2d, batch_norm(training=True), relu, max_pool2d / avg_pool2d
and autograd, on the CPU) on the same inputs beside them."""
import copy
import ctypes

import pytest
import torch

from mocopci_amd import _lib, ops, pointnet2_utils as pu
from tests import fused_reference as fr
from tests import group_mlp_bn_reference as gbr
from tests.test_fp_mlp_grad_cpu import C_CAP
from tests.test_group_mlp_bn_cpu import CASES, FURTHER, LENGTHS, OFFSET, case_id, composed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
# This project's rule: the smallest power of two at least twice the worst relative error measured on the MI355X against float64
# (profiles/group_mlp_bn_accuracy.txt holds every RATIO line), never above C_CAP = 2^-13.
# Worst measured: 9.98e-07 (c128-ns64-128x128x256 at 1 x 3 centres, mean pool, w3; the fp32 composition on the same inputs: 9.43e-07),
# 6.74e-07 through the module against its composition; twice the worst is 2.00e-06, between 2^-19 = 1.91e-06 and 2^-18 = 3.81e-06.  The
# cancellation case measures 2.20e-05 at its worst (w1; the fp32 composition: 1.33e-04): twice that lies between 2^-15 and 2^-14.
# The largest db against the floor 2e-5: 1.24e-05 (b1 of the first case).  The only tensors on which the kernel is more than four
# times the fp32 composition's error are variances (at most 6.7 x: var1 of c4-ns32, 2.53e-07 against 3.78e-08): torch's CPU var and
# batch_norm accumulate fp32 in double, so their error is one final rounding, the kernel's is that of fp32 Chan merges.
C_GROUP_MLP_BN = 2.0 ** -18
C_GROUP_MLP_BN_CANCELLATION = 2.0 ** -14
assert C_GROUP_MLP_BN <= C_GROUP_MLP_BN_CANCELLATION <= C_CAP


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.fixture
def nan_buffers(monkeypatch):
    """Every buffer the layer allocates starts as NaN (the byte workspace as 0xFF bytes: NaN in every float; int32 as -1)."""
    def poisoned(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        return t.fill_(255 if dtype == torch.uint8 else -1 if dtype == torch.int32 else NAN)
    monkeypatch.setattr(ops, "_grad_empty", poisoned)


def run_layer(prep, lengths=None, g=None):
    """(out, [(mean_l, var_l)], count, [gradient per leaf]) of be.group_mlp_bn_layer; both directions run twice and must repeat bit for
    bit."""
    d = prep.data
    leaves = [t.to(DEV).requires_grad_(True) for t in prep.leaves]
    named = dict(zip(prep.names, leaves))
    layers = [(*quad, e) for quad, e in zip(prep.layer_leaves(leaves), prep.eps)]
    xyz = named["xyz"] if d["use_xyz"] else d["xyz"].to(DEV)
    new_xyz = named["new_xyz"] if d["use_xyz"] else d["new_xyz"].to(DEV)
    idx = d["idx"].to(DEV)
    call = lambda: ops.backend().group_mlp_bn_layer(xyz, new_xyz, named.get("features"), idx, layers, pool=d["pool"], use_xyz=d["use_xyz"],
                                                    new_xyz_lengths=lengths)
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
    """torch's fp32 composition over the live centres on the CPU -> (out, stats, grads), for the figures printed beside the kernel's."""
    l32 = [t.clone().requires_grad_(True) for t in prep.leaves]
    out, stats = composed(prep, l32)
    grads = torch.autograd.grad(out, l32, prep.g[prep.centres].float(), allow_unused=True)
    return out.detach(), stats, [torch.zeros_like(t) if x is None else x for t, x in zip(l32, grads)]


def judge(name, prep, out, stats, count, grads, bound=C_GROUP_MLP_BN):
    assert gbr.clear(prep), "an input with a pre-activation within 1e-4 of zero"
    e_out, e_stats, m, e_grads = gbr.exact(prep)
    assert int(count.item()) == m
    c_out, c_stats, c_grads = composed_fp32(prep)
    c_full = torch.zeros_like(e_out)
    c_full[prep.centres] = c_out.double()
    got = [("out", out.cpu().view(e_out.shape), e_out, c_full)]
    for l, ((mu, v), (emu, ev), (cmu, cv)) in enumerate(zip(stats, e_stats, c_stats)):
        got += [(f"mean{l + 1}", mu.cpu(), emu, cmu.detach().double()), (f"var{l + 1}", v.cpu(), ev, cv.detach().double())]
    got += [(n, a.cpu(), e, c.double()) for n, a, e, c in zip(prep.names, grads, e_grads, c_grads)]
    line, worst = f"RATIO {name} seed={prep.seed}", []
    for n, a, e, c in got:
        assert torch.isfinite(a).all(), n
        r = gbr.ratio(a, e, bound)
        zero = e.abs().max().item() == 0 or (n[0] == "b" and n[1:].isdigit())
        if zero:   # zero in exact arithmetic (float64 leaves a rounding residue in db): the floor
            r = a.abs().max().item() / gbr.FLOOR
            line += f" {n}=floor:{a.abs().max().item():.2e}"
        else:
            line += f" {n}={gbr.ratio(a, e, 1.0):.2e}/{gbr.ratio(c, e, 1.0):.2e}"
        worst.append((r, n))
    print(line)
    r, n = max(worst)
    assert r <= 1.0, f"group_mlp_bn {name}: {n} at {r:.2f} x the bound"


def check_case(k, bound=C_GROUP_MLP_BN, **pick):
    prep = gbr.pick(k, **pick)
    out, stats, count, grads = run_layer(prep)
    gathered = torch.zeros(k["b"], k["n"], dtype=torch.bool)
    gathered[torch.arange(k["b"])[:, None, None], prep.data["idx"].long()] = True
    for name in ("features", "xyz"):
        if name in prep.names:
            assert (grads[prep.names.index(name)].cpu()[~gathered] == 0).all(), f"a row of {name} that no slot gathers has a non-zero gradient"
    judge(case_id(k) + ("-offset-nobias" if pick else ""), prep, out, stats, count, grads, bound)


@pytest.mark.parametrize("case_", CASES + FURTHER, ids=case_id)
def test_group_mlp_bn_matches_float64(case_, nan_buffers):
    check_case(case_)


def test_group_mlp_bn_variance_survives_a_mean_a_hundred_sigmas_away(nan_buffers):
    """No conv bias, features offset by +100 on the first case: |mu_1| is far above sigma_1 in every channel.  Same check as every other
    case, with this case's own measured constant under the same cap."""
    check_case(CASES[0], C_GROUP_MLP_BN_CANCELLATION, offset=OFFSET, biased=False)


def test_lengths_count_only_live_pairs_and_read_nothing_from_padded_centres(nan_buffers):
    """new_xyz_lengths = (7, 3, 0): statistics and gradients are the float64 reference's over the 80 live pairs; padded centres give
    zero outputs and a zero grad_new_xyz; NaN in the padded centres' new_xyz and grad_out changes no bit."""
    k = CASES[0]
    prep = gbr.pick(k, lengths=LENGTHS)
    assert prep.pairs() == 80
    out, stats, count, grads = run_layer(prep, lengths=list(LENGTHS))
    judge(f"{case_id(k)}-lengths", prep, out, stats, count, grads)
    at = prep.names.index("new_xyz")
    d_new = grads[at]
    new_xyz, g = prep.leaves[at].clone(), prep.g.float().view(k["b"], k["m"], -1).clone()
    for b, nu in enumerate(LENGTHS):
        assert (out[b, nu:] == 0).all() and (d_new[b, nu:] == 0).all(), f"element {b}: padded centres are not exact zeros"
        new_xyz[b, nu:] = NAN
        g[b, nu:] = NAN
    poisoned = copy.copy(prep)
    poisoned.leaves = [*prep.leaves[:at], new_xyz, *prep.leaves[at + 1:]]
    out_p, stats_p, count_p, grads_p = run_layer(poisoned, lengths=list(LENGTHS), g=g.to(DEV))
    assert torch.equal(out, out_p) and torch.equal(count, count_p)
    for (a, b), (a2, b2) in zip(stats, stats_p):
        assert torch.equal(a, a2) and torch.equal(b, b2)
    for name, a, b in zip(prep.names, grads, grads_p):
        assert torch.equal(a, b), f"{name}: a padded centre's NaN reached it"


# ---- module ----------------------------------------------------------------------------------------------------------------------------
MB, MN, MP = 2, 300, 16
SCALES = ((0.7, 8), (1.5, 16))
MLPS = [[4, 32, 32], [4, 32, 64]]


def sa_module(g, momentum):
    from mocopci_amd.pointnet2_modules import PointnetSAModuleMSG
    m = PointnetSAModuleMSG(npoint=MP, radii=[r for r, _ in SCALES], nsamples=[n for _, n in SCALES], mlps=[list(s) for s in MLPS], bn=True)
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
    for stack in m.mlps:
        for unit in stack.children():
            unit.bn.bn.momentum = momentum
    return m.train()


def module_float64(m, xyz, new_xyz, rows, idxs, G, grad):
    """Float64 <module(centre), G[centre]> over all centres from float64 copies of the parameters -> (clear, pool mask (centres, sum
    C_out), gradients for the features and every parameter, in m.parameters() order)."""
    f64 = rows.double().requires_grad_(grad)
    params, outs, keeps, clear = [], [], [], True
    sel = torch.arange(MB * MP)
    for i, idx in enumerate(idxs):
        convs, bns = m._layers(i)
        layers = []
        for c, bn in zip(convs, bns):
            trio = [c.weight.detach().cpu().double().flatten(1), bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double()]
            trio = [t.requires_grad_(grad) for t in trio]
            params += trio
            layers.append((trio[0], None, trio[1], trio[2]))
        d = dict(xyz=xyz, new_xyz=new_xyz, features=rows, idx=idx, use_xyz=True, pool="max")
        x = gbr.gather_rows([f64, xyz.double(), new_xyz.double()], d, sel)
        out, ys, _ = gbr.forward(x, layers, [bn.eps for bn in bns], "max")
        clear = clear and min(y.abs().min().item() for y in ys) > gbr.CLEAR
        keeps.append(gbr.ggr.clear_mask(dict(pool="max"), [ys[-1].detach()], idx.view(MB * MP, -1).long()))
        outs.append(out)
    keep = torch.cat(keeps, 1)
    if not grad:
        return clear, keep, None
    got = torch.autograd.grad(torch.cat(outs, 1), [f64, *params], G * keep)
    return clear, keep, [got[0].transpose(1, 2)] + [e.view(p.shape) for e, p in zip(got[1:], m.parameters())]


def module_grads(m, x, f, G, kw, with_xyz=False):
    f = f.clone().requires_grad_(True)
    x = x.clone().requires_grad_(with_xyz)
    new_xyz, out = m(x, f, **kw)
    return out.detach(), list(torch.autograd.grad(out, [f, *m.parameters()] + ([x] if with_xyz else []), G))


def buffers(m):
    return {k: v.detach().clone() for k, v in m.named_buffers()}


def raising_grouper(monkeypatch):
    def boom(self, *a, **kw):
        raise AssertionError("the composition was taken")
    monkeypatch.setattr(pu.QueryAndGroup, "forward", boom)


@pytest.mark.parametrize("momentum", [0.1, None], ids=["momentum0.1", "cumulative"])
def test_sa_module_bn_route_against_its_composition_and_float64(momentum, nan_buffers, monkeypatch):
    g = torch.Generator().manual_seed(31)
    xyz = fr.clustered_cloud(g, MB, MN, 32)
    feats = torch.randn(MB, 4, MN, generator=g) + 0.5
    x, f = dev(xyz, feats)
    be = ops.backend()
    probe = sa_module(torch.Generator().manual_seed(1), momentum).to(DEV)
    with torch.no_grad():   # the centres and the device's own ball-query lists: neither depends on a parameter
        new_xyz = probe.eval()(x, f)[0]
        idxs = [be.ball_query(x, new_xyz, r, ns).cpu() for r, ns in SCALES]
    rows = feats.transpose(1, 2).contiguous()
    for t in range(gbr.TRIES):   # the first parameter seed that keeps every y_l clear of zero
        m = sa_module(torch.Generator().manual_seed(2000 + t), momentum)
        if module_float64(m, xyz, new_xyz.cpu(), rows, idxs, None, False)[0]:
            break
    else:
        raise AssertionError("no clear module parameters")
    width = sum(s[-1] for s in MLPS)
    G64 = torch.randn(MB * MP, width, generator=torch.Generator().manual_seed(99)).double()
    clear, keep, exact = module_float64(m, xyz, new_xyz.cpu(), rows, idxs, G64, True)
    assert clear and keep.double().mean() > 0.9
    G = (G64 * keep).float().view(MB, MP, width).transpose(1, 2).contiguous().to(DEV)
    fused, comp = copy.deepcopy(m).to(DEV), copy.deepcopy(m).to(DEV)
    fused.bn_route, comp.bn_route = "always", "never"
    out_c, grads_c = module_grads(comp, x, f, G, {})
    with monkeypatch.context() as mp:   # the composition made unreachable
        raising_grouper(mp)
        out_f, grads_f = module_grads(fused, x, f, G, {})
    assert torch.allclose(out_f, out_c, rtol=1e-4, atol=1e-5)
    names = ["features"] + [n for n, _ in m.named_parameters()]
    line = f"RATIO module-{'cumulative' if momentum is None else 'momentum'} try={t + 1} kept={keep.double().mean().item():.4f}"
    for name, a, c, e in zip(names, grads_f, grads_c, exact):
        assert torch.isfinite(a).all(), name
        r, r2 = gbr.ratio(a.cpu(), e, C_GROUP_MLP_BN), gbr.ratio(a.cpu(), c.cpu().double(), C_GROUP_MLP_BN)
        line += f" {name}={gbr.ratio(a.cpu(), e, 1.0):.2e}/{gbr.ratio(c.cpu(), e, 1.0):.2e}/{gbr.ratio(a.cpu(), c.cpu().double(), 1.0):.2e}"
        assert r <= 1.0 and r2 <= 1.0, f"{name}: {r:.2f} x the bound against float64, {r2:.2f} x against the module's composition"

    def same_buffers(step):
        nonlocal line
        bf, bc = buffers(fused), buffers(comp)
        for key in bc:
            if key.endswith("num_batches_tracked"):
                assert int(bf[key]) == int(bc[key]) == 3 + step, key
            else:
                r = gbr.ratio(bf[key].cpu(), bc[key].cpu().double(), C_GROUP_MLP_BN)
                line += f" {'.'.join(key.split('.')[1:3])}.{key.split('.')[-1]}@{step}={gbr.ratio(bf[key].cpu(), bc[key].cpu().double(), 1.0):.2e}"
                assert r <= 1.0, f"{key} after {step} call(s): {r:.2f} x the bound from the composition's"
    same_buffers(1)
    with torch.no_grad():   # a forward without a wanted gradient still takes the route and still updates the running statistics
        with monkeypatch.context() as mp:
            raising_grouper(mp)
            out_f2 = fused(x, f)[1]
        out_c2 = comp(x, f)[1]
    assert torch.equal(out_f2, out_f) and torch.allclose(out_f2, out_c2, rtol=1e-4, atol=1e-5)
    same_buffers(2)
    # xyz.requires_grad: a finite xyz.grad on both routes, the two within the bound
    gx = module_grads(fused, x, f, G, {}, with_xyz=True)[1][-1]
    gx_c = module_grads(comp, x, f, G, {}, with_xyz=True)[1][-1]
    assert torch.isfinite(gx).all() and gx.abs().max() > 0
    r = gbr.ratio(gx.cpu(), gx_c.cpu().double(), 1.0)
    line += f" xyz fused/composed={r:.2e}"
    print(line)
    assert r <= C_GROUP_MLP_BN, f"xyz.grad: {r / C_GROUP_MLP_BN:.2f} x the bound between the two routes"


def test_sa_module_keeps_the_composition_when_it_must(monkeypatch):
    """With lengths, in eval(), with npoint=None and under "measured" with the empty table the route is not taken: a
    group_mlp_bn_layer that raises proves each."""
    from mocopci_amd.pointnet2_modules import PointnetSAModule
    g = torch.Generator().manual_seed(5)
    x, f = dev(fr.clustered_cloud(g, MB, MN, 32), torch.randn(MB, 4, MN, generator=g) + 0.5)
    m = sa_module(g, 0.1).to(DEV)
    width = sum(s[-1] for s in MLPS)
    G = torch.randn(MB, width, MP, generator=g).to(DEV)

    def boom(self, *a, **kw):
        raise AssertionError("the fused route with batch statistics was taken")
    monkeypatch.setattr(ops.HipBackend, "group_mlp_bn_layer", boom)
    m.bn_route = "always"
    with pytest.raises(AssertionError, match="batch statistics"):
        module_grads(m, x, f, G, {})
    out, grads = module_grads(m, x, f, G, dict(xyz_lengths=[300, 120], new_xyz_lengths=[16, 5]))
    assert torch.isfinite(out).all() and all(torch.isfinite(t).all() for t in grads)
    m.bn_route = "measured"
    assert ops.GROUP_MLP_BN_FUSED_CLASSES == {} and not ops.group_mlp_bn_routes_fused(4, [32, 32], 8, MB * MP)
    out, grads = module_grads(m, x, f, G, {})
    assert torch.isfinite(out).all() and all(torch.isfinite(t).all() for t in grads)
    m.bn_route = "always"
    m.eval()
    assert torch.isfinite(module_grads(m, x, f, G, {})[0]).all(), "eval() is not the route's"
    whole = PointnetSAModule(mlp=[4, 32, 32], bn=True).to(DEV).train()   # npoint=None: GroupAll
    whole.bn_route = "always"
    assert torch.isfinite(whole(x, f)[1]).all()


def test_unsupported_shapes_launch_nothing():
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    x, f = torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 8, 8, device=DEV)
    idx = torch.zeros(1, 4, 16, dtype=torch.int32, device=DEV)
    buf = torch.full((1 << 16,), 7.0, device=DEV)
    g = torch.zeros(1, 4, 48, device=DEV)
    p, i = _lib.fptr, _lib.iptr
    four = lambda: (ctypes.c_void_p * 4)(*[p(buf)] * 4)
    eps = (ctypes.c_float * 4)(1e-5, 1e-5, 1e-5, 1e-5)
    for c, ns, xyz, widths in ((6, 16, 1, (32,)), (8, 16, 1, (48,)), (8, 65, 1, (32,)), (0, 16, 0, (32,)), (8, 16, 1, (256, 32)), (8, 16, 1, (32, 32, 32, 32))):
        rc = lib.mcp_group_mlp_bn_forward(1, 8, 4, c, ns, xyz, 0, len(widths), w(*widths), p(x), p(x), p(f), i(idx), None, p(buf), four(), four(), eps, p(buf),
                                          four(), four(), four(), buf.data_ptr(), buf.data_ptr(), buf.numel() * 4, None)
        assert rc == 10002, (c, ns, xyz, widths, rc)
        rc = lib.mcp_group_mlp_bn_backward(1, 8, 4, c, ns, xyz, 0, len(widths), w(*widths), p(x), p(x), p(f), i(idx), None, p(buf), four(), four(), four(),
                                           four(), p(g), None, None, None, None, None, four(), four(), four(), four(), buf.data_ptr(), buf.numel() * 4, None)
        assert rc == 10002, (c, ns, xyz, widths, rc)
    torch.cuda.synchronize()
    assert (buf == 7.0).all()
    with pytest.raises(_lib.Unsupported):
        ops.backend().group_mlp_bn_layer(x, x[:, :4].contiguous(), f, idx, [(torch.zeros(48, 11, device=DEV), None, None, None, 1e-5)])
