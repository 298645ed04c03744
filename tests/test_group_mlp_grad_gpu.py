"""-m gpu: the backward of the fused set-abstraction layer (csrc/group_mlp_grad.hip, ops.HipBackend.group_mlp_layer / group_mlp_grad)
and PointnetSAModuleMSG's differentiable fused route against the float64 gradients of tests/group_mlp_grad_reference.py.

Shapes: B = 3, M = 37, N = 500 over the cases of test_group_mlp_grad_cpu.py -- with 4, 2 or 1 centres per 32-column tile the last tile
has fewer centres than groups and tiles cross element boundaries; nsample covers the group widths 8, 16, 32, a partial group and the
two-tile form; the widths reach both sides of the staging predicate (the kernel has one register class).  (B, M) = (1, 3) and a
centre count that fills the eight waves of one workgroup exactly, on a narrow and a wide shape; 3 x 700 centres at nsample = 32, the
smallest count above the persistent grid's 256 x 8 units, with a partial second trip.

Every case runs through be.group_mlp_layer with requires_grad leaves and with every buffer the backward allocates refilled with NaN
first, and asserts: finite gradients, a second backward with identical bits, exact zeros in the rows of features / xyz nobody gathers,
the recomputed out equal to be.group_mlp bit for bit, and
    ratio = max |hip - exact| / (C max |exact|) <= 1
per group -- (a) the per-point gradients (features, xyz, new_xyz, row_bias), (b) the weight and bias gradients -- the largest ratio
over the group's tensors; a gradient that is zero in exact arithmetic is held to the floor 2e-5.  Each case prints its RATIO line with
the relative errors themselves and the fp32 composition's (autograd over the composition on the device) beside them."""
import ctypes
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from mocopci_amd import _lib, ops
from tests import fused_reference as fr
from tests import group_mlp_grad_reference as ggr
from tests.test_group_mlp_grad_cpu import B, CASES, C_CAP, M, N, PERSISTENT, SMALL, case, case_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
# This project's rule: the smallest power of two at least twice the worst relative error measured on the MI355X against float64
# (profiles/group_mlp_grad_accuracy.txt holds every RATIO line), never above C_CAP = 2^-13, the loosest constant any backward here carries.
# Worst measured: 1.793e-06 on a weight gradient (c4-ns32-32x32x64 over 3 x 700 centres: 67200 pairs in mcp_linear_wgrad's fp32 sums;
# the fp32 composition on the same inputs: 7.68e-07), 8.14e-07 at B x M = 3 x 37 (c128-ns64-128x128x256, weights), 5.56e-07 on a
# per-point gradient, about 1.2e-06 through the module (a BatchNorm bias).  Twice the worst is 3.59e-06, between 2^-19 = 1.9e-06 and
# 2^-18 = 3.8e-06.
C_GROUP_MLP_GRAD = 2.0 ** -18
assert C_GROUP_MLP_GRAD <= C_CAP


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
def prepared(key):
    k = dict(key)
    k["widths"] = list(k["widths"])
    prep = ggr.prepare(k)
    return prep, ggr.gradients(prep)


def case_prepared(k):
    return prepared(tuple(sorted((n, tuple(v) if isinstance(v, list) else v) for n, v in k.items())))


def layer_args(prep, leaves):
    """(xyz, new_xyz, features, row_bias, weights) for the layer: the leaves where the layer has them, the constants elsewhere."""
    d = prep.data
    t = dict(zip(prep.names, leaves))
    xyz, new_xyz = (t["xyz"], t["new_xyz"]) if d["use_xyz"] else dev(d["xyz"], d["new_xyz"])
    weights = [(t[f"w{l + 1}"], t[f"b{l + 1}"]) for l in range(len(d["weights"]))]
    return xyz, new_xyz, t.get("features"), t.get("row_bias"), weights


def device_leaves(prep):
    return [t.to(DEV).requires_grad_(True) for t in prep.leaves]


def run_layer(prep, lengths=None, g=None):
    """(out, [gradient per leaf]) of be.group_mlp_layer on the prepared data."""
    d = prep.data
    leaves = device_leaves(prep)
    xyz, new_xyz, feats, row_bias, weights = layer_args(prep, leaves)
    out = ops.backend().group_mlp_layer(xyz, new_xyz, feats, d["idx"].to(DEV), weights, pool=d["pool"], use_xyz=d["use_xyz"], new_xyz_lengths=lengths,
                                        row_bias=row_bias)
    assert out.requires_grad
    g = prep.g.float().view(out.shape).to(DEV) if g is None else g
    grads = torch.autograd.grad(out, leaves, g, retain_graph=True)
    again = torch.autograd.grad(out, leaves, g)
    for name, a, b in zip(prep.names, grads, again):
        assert torch.equal(a, b), f"{name}: a second backward gives other bits"
    return out.detach(), list(grads)


def composition(xyz, new_xyz, feats, row_bias, weights, idx, use_xyz, pool):
    """The layer as the module composes it in fp32 torch (F.max_pool2d: the first of tied slots takes the gradient)."""
    bi = torch.arange(xyz.shape[0], device=xyz.device)[:, None, None]
    j = idx.long()
    parts = ([xyz[bi, j] - new_xyz[:, :, None]] if use_xyz else []) + ([feats[bi, j]] if feats is not None else [])
    h = torch.cat(parts, -1).permute(0, 3, 1, 2).contiguous()
    for l, (w, bias) in enumerate(weights):
        h = F.conv2d(h, w[:, :, None, None], bias)
        if l == 0 and row_bias is not None:
            h = h + row_bias.permute(0, 2, 1)[..., None]
        h = torch.relu(h)
    h = (F.max_pool2d if pool == "max" else F.avg_pool2d)(h, kernel_size=[1, h.size(3)]).squeeze(-1)
    return h.transpose(1, 2)


def composed_grads(prep):
    """fp32 autograd over the composition on the device, for the figure printed beside the kernel's."""
    d = prep.data
    leaves = device_leaves(prep)
    xyz, new_xyz, feats, row_bias, weights = layer_args(prep, leaves)
    out = composition(xyz, new_xyz, feats, row_bias, weights, d["idx"].to(DEV), d["use_xyz"], d["pool"])
    return list(torch.autograd.grad(out, leaves, prep.g.float().view(out.shape).to(DEV)))


def judge(name, prep, grads, exact, composed=None):
    worst = {}
    line = f"RATIO {name}"
    npt = prep.point_leaves()
    for group, span in (("points", range(npt)), ("weights", range(npt, len(prep.names)))):
        live = [i for i in span if exact[i].abs().max() > 0]
        ratios = [ggr.ratio(grads[i].cpu(), exact[i], C_GROUP_MLP_GRAD) for i in span]
        rel = max((ggr.ratio(grads[i].cpu(), exact[i], 1.0) for i in live), default=0.0)
        worst[group] = max(ratios)
        line += f" {group}={max(ratios):.3f} (rel {rel:.3e}"
        if composed is not None:
            line += f", composed_fp32 {max((ggr.ratio(composed[i].cpu(), exact[i], 1.0) for i in live), default=0.0):.3e}"
        line += ")"
    print(line)
    for t in grads:
        assert torch.isfinite(t).all()
    for group, r in worst.items():
        assert r <= 1.0, f"group_mlp_grad {name}: {group} gradients at {r:.2f} x the bound"


def check_case(k):
    prep, exact = case_prepared(k)
    d = prep.data
    out, grads = run_layer(prep)
    be = ops.backend()
    xyz, new_xyz, feats, row_bias, weights = layer_args(prep, [t.to(DEV) for t in prep.leaves])
    idx = d["idx"].to(DEV)
    kw = dict(pool=d["pool"], use_xyz=d["use_xyz"], row_bias=row_bias)
    fwd = be.group_mlp(xyz, new_xyz, feats, idx, *ops.group_mlp_pack_weights(weights, d["use_xyz"]), **kw)
    assert torch.equal(out, fwd)
    raw = be.group_mlp_grad(xyz, new_xyz, feats, idx, weights, prep.g.float().view(out.shape).to(DEV), recompute_out=True, **kw)
    assert torch.equal(raw[6], fwd), "the recomputed out differs from mcp_group_mlp's"
    by_name = dict(zip(prep.names, grads))
    for name, t in zip(("features", "xyz", "new_xyz", "row_bias"), raw[:4]):
        assert (t is None) == (name not in by_name) and (t is None or torch.equal(t, by_name[name])), name
    npt = prep.point_leaves()
    assert all(torch.equal(a, b) for a, b in zip(raw[4], grads[npt::2])) and all(torch.equal(a, b) for a, b in zip(raw[5], grads[npt + 1::2]))
    gathered = torch.zeros(k["b"], k["n"], dtype=torch.bool)
    gathered[torch.arange(k["b"])[:, None, None], d["idx"].long()] = True
    for name in ("features", "xyz"):
        if name in by_name:
            assert (by_name[name].cpu()[~gathered] == 0).all(), f"a row of {name} that nobody gathers has a non-zero gradient"
    judge(case_id(k), prep, grads, exact, composed_grads(prep))


@pytest.mark.parametrize("case_", CASES, ids=case_id)
def test_group_mlp_grad_matches_float64(case_, nan_buffers):
    check_case(case_)


@pytest.mark.parametrize("case_", SMALL, ids=case_id)
def test_group_mlp_grad_dead_groups_and_one_full_workgroup(case_, nan_buffers):
    check_case(case_)


@pytest.mark.parametrize("case_", PERSISTENT, ids=case_id)
def test_group_mlp_grad_beyond_the_persistent_grid(case_, nan_buffers):
    """3 x 700 centres, one per unit: 2100 units over the grid's 256 x 8 waves, the second trip partial."""
    assert case_["b"] * case_["m"] > 256 * 8 and case_["nsample"] > 16
    check_case(case_)


def test_without_a_wanted_gradient_the_layer_is_the_forward():
    prep, _ = case_prepared(CASES[2])
    d = prep.data
    xyz, new_xyz, feats, row_bias, weights = layer_args(prep, [t.to(DEV) for t in prep.leaves])
    idx = d["idx"].to(DEV)
    be = ops.backend()
    out = be.group_mlp_layer(xyz, new_xyz, feats, idx, weights)
    assert not out.requires_grad
    assert torch.equal(out, be.group_mlp(xyz, new_xyz, feats, idx, *ops.group_mlp_pack_weights(weights)))
    with torch.no_grad():
        x2, c2, f2, _, w2 = layer_args(prep, device_leaves(prep))
        assert torch.equal(be.group_mlp_layer(x2, c2, f2, idx, w2), out)


# ---- searched neighbour lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["tiny-radius", "ball", "knn"])
def test_group_mlp_grad_on_searched_neighbour_lists(source, nan_buffers):
    """idx as the searches make it: a radius so small that every slot holds the same point, a ball query with its first-hit padding,
    and a KNN list (K = 16)."""
    k = case(4, 16, [32, 32, 64])
    d = ggr.grad_inputs(k)
    be = ops.backend()
    x, c = dev(d["xyz"], d["new_xyz"])
    idx = (be.knn(c, x, 16) if source == "knn" else be.ball_query(x, c, 1e-3 if source == "tiny-radius" else 0.7, 16)).cpu()
    if source == "tiny-radius":
        assert (idx == idx[:, :, :1]).all()
    prep = ggr.prepare(data=dict(d, idx=idx.contiguous()))
    print(f"CLEAR {source} kept={prep.clear.double().mean().item():.3f}")
    assert prep.clear.double().mean() > 0.9
    _, grads = run_layer(prep)
    judge(source, prep, grads, ggr.gradients(prep), composed_grads(prep))


# ---- lengths ---------------------------------------------------------------------------------------------------------------------------
def sliced(prep, b, n):
    d = prep.data
    part = dict(d, xyz=d["xyz"][b:b + 1], new_xyz=d["new_xyz"][b:b + 1, :n].contiguous(), idx=d["idx"][b:b + 1, :n].contiguous(),
                features=None if d["features"] is None else d["features"][b:b + 1],
                row_bias=None if d["row_bias"] is None else d["row_bias"][b:b + 1, :n].contiguous())
    return ggr.Prepared(part, prep.names, ggr.leaf_list(part), None, None, None, 0.0)


@pytest.mark.parametrize("case_", [case(4, 8, [32, 32, 64]), case(64, 16, [64, 64], c2=64), case(64, 64, [64, 64, 128], pool="mean")], ids=case_id)
def test_lengths_give_the_sliced_call_and_nothing_from_padded_centres(case_, nan_buffers):
    """Centre lengths (37, 20, 0); the padded rows of new_xyz, row_bias and grad_out hold NaN.  The live per-point gradients equal, bit
    for bit, those of the call on the element's sliced prefix; padded rows of grad_new_xyz and grad_row_bias are exact zeros; the
    element without a live centre sends nothing to its features and points."""
    lens = (37, 20, 0)
    d = dict(ggr.grad_inputs(case_))
    d["new_xyz"] = d["new_xyz"].clone()
    if d["row_bias"] is not None:
        d["row_bias"] = d["row_bias"].clone()
    live = torch.cat([torch.arange(n) + b * M for b, n in enumerate(lens)])
    prep = ggr.prepare(data=d, centres=live)           # on the clean inputs
    assert prep.clear[live].double().mean() > 0.9 and not prep.clear.index_fill(0, live, False).any()
    exact = ggr.gradients(prep)
    g = prep.g.float().view(B, M, -1).clone()
    for b, n in enumerate(lens):
        g[b, n:] = NAN
        d["new_xyz"][b, n:] = NAN
        if d["row_bias"] is not None:
            d["row_bias"][b, n:] = NAN
    prep.leaves = ggr.leaf_list(d)
    g = g.to(DEV)
    out, grads = run_layer(prep, lengths=list(lens), g=g)
    by_name = dict(zip(prep.names, grads))
    for t in grads:
        assert torch.isfinite(t).all()
    for b, n in enumerate(lens):
        assert (out[b, n:] == 0).all(), f"element {b}: padded centres are not exact zeros"
        for name in ("new_xyz", "row_bias"):
            if name in by_name:
                assert (by_name[name][b, n:] == 0).all(), f"element {b}: padded rows of grad_{name} are not exact zeros"
        if n == 0:
            assert all((by_name[name][b] == 0).all() for name in ("features", "xyz") if name in by_name), "an element without a live centre sends something"
            continue
        part = dict(zip(prep.names, run_layer(sliced(prep, b, n), g=g[b:b + 1, :n].contiguous())[1]))
        for name in ("features", "xyz"):
            if name in by_name:
                assert torch.equal(part[name][0], by_name[name][b]), f"element {b}: grad_{name} differs from the sliced call"
        for name in ("new_xyz", "row_bias"):
            if name in by_name:
                assert torch.equal(part[name][0], by_name[name][b, :n]), f"element {b}: grad_{name} differs from the sliced call"
    judge(f"{case_id(case_)}-lengths", prep, grads, exact)


# ---- module ----------------------------------------------------------------------------------------------------------------------------
MB, MN, MP = 2, 3000, 128
SCALES = ((0.7, 12), (1.5, 24))


def sa_module(g, bn):
    """The two-scale fixture of pointnet2_sa_state_keys.json with sign-mixed weights (bn=False: the same stack without BatchNorm)."""
    from mocopci_amd.pointnet2_modules import PointnetSAModuleMSG
    m = PointnetSAModuleMSG(npoint=MP, radii=[r for r, _ in SCALES], nsamples=[n for _, n in SCALES], mlps=[[4, 32, 32, 64], [4, 64, 64, 128]], bn=bn)
    if bn:
        spec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet2_sa_state_keys.json")))
        assert set(spec) == set(m.state_dict())
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


def module_grads(m, x, f, G, kw, with_xyz=False):
    f = f.clone().requires_grad_(True)
    x = x.clone().requires_grad_(with_xyz)
    params = list(m.parameters())
    new_xyz, out = m(x, f, **kw)
    return new_xyz.detach(), out.detach(), list(torch.autograd.grad(out, [f, *params] + ([x] if with_xyz else []), G))


def module_float64(m, xyz, new_xyz, rows, idxs, live, G):
    """Float64 gradients of <module(centre), G[centre]> over the live centres for (features, parameters...): the fold in float64 as an
    autograd function of float64 copies of the parameters, then group_mlp_grad_reference.layer per scale.  -> (clear masks, grads)."""
    f64 = rows.double().requires_grad_(True)
    params, outs, clears = [], [], []
    for i, idx in enumerate(idxs):
        convs, bns = m._layers(i)
        folded = []
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
        d = dict(xyz=xyz, new_xyz=new_xyz, features=rows, idx=idx, row_bias=None, weights=[None] * len(convs), use_xyz=True, pool="max")
        out, zs = ggr.layer([f64, xyz.double(), new_xyz.double(), *folded], d, live)
        outs.append(out)
        clears.append(ggr.clear_mask(d, [z.detach() for z in zs], idx[live // MP, live % MP].long()))
    clear = torch.cat(clears, 1)
    got = torch.autograd.grad(torch.cat(outs, 1), [f64, *params], G[live] * clear)
    return clear, got


@pytest.mark.parametrize("lengths", [None, ((3000, 1200), (128, 50))], ids=["full", "short"])
@pytest.mark.parametrize("mode", ["eval-bn", "train-no-bn"])
def test_sa_module_fused_backward_against_its_composition_and_float64(mode, lengths, nan_buffers):
    g = torch.Generator().manual_seed(41)
    bn = mode == "eval-bn"
    m = sa_module(g, bn)
    m = m.eval() if bn else m.train()
    m.grad_route = "always"
    xyz = fr.clustered_cloud(g, MB, MN, 32)
    feats = torch.randn(MB, 4, MN, generator=g) + 0.5
    kw = {} if lengths is None else dict(xyz_lengths=list(lengths[0]), new_xyz_lengths=list(lengths[1]))
    x, f = dev(xyz, feats)
    be = ops.backend()
    with torch.no_grad():
        new_xyz = m(x, f, **kw)[0]
        rl, ql = (None, None) if lengths is None else (list(lengths[0]), list(lengths[1]))
        idxs = [be.ball_query(x, new_xyz, r, ns, xyz_lengths=rl, new_xyz_lengths=ql).cpu() for r, ns in SCALES]
    counts = (MP,) * MB if lengths is None else lengths[1]
    live = torch.cat([torch.arange(n) + b * MP for b, n in enumerate(counts)])
    width = 64 + 128
    G64 = torch.randn(MB * MP, width, generator=torch.Generator().manual_seed(99)).double()
    rows = feats.transpose(1, 2).contiguous()
    clear, exact = module_float64(m, xyz, new_xyz.cpu(), rows, idxs, live, G64)
    print(f"CLEAR module-{mode} kept={clear.double().mean().item():.3f}")
    assert clear.double().mean() > 0.9
    Gm = torch.zeros(MB * MP, width, dtype=torch.float64)
    Gm[live] = G64[live] * clear
    G = Gm.float().view(MB, MP, width).transpose(1, 2).contiguous().to(DEV)
    c_fused, out, fused = module_grads(m, x, f, G, kw)
    m.grad_route = "never"
    c_comp, out_c, composed = module_grads(m, x, f, G, kw)
    assert torch.equal(c_fused, c_comp) and torch.allclose(out, out_c, rtol=1e-4, atol=1e-5)
    names = ["features"] + [n for n, _ in m.named_parameters()]
    exact = [exact[0].transpose(1, 2)] + [e.view(p.shape) for e, p in zip(exact[1:], m.parameters())]
    line = f"RATIO module-{mode}-{'full' if lengths is None else 'short'}"
    for name, a, c, e in zip(names, fused, composed, exact):
        assert torch.isfinite(a).all(), name
        r, rc = ggr.ratio(a.cpu(), e, C_GROUP_MLP_GRAD), ggr.ratio(c.cpu(), e, C_GROUP_MLP_GRAD)
        r2 = ggr.ratio(a.cpu(), c.cpu().double(), C_GROUP_MLP_GRAD)
        line += f" {name}={r:.3f}/{rc:.3f}/{r2:.3f}"
        assert r <= 1.0 and r2 <= 1.0, f"{name}: {r:.2f} x the bound against float64, {r2:.2f} x against the module's composition"
    print(line)
    # xyz.requires_grad: a finite xyz.grad on both routes, the two within C
    m.grad_route = "always"
    gx = module_grads(m, x, f, G, kw, with_xyz=True)[2][-1]
    m.grad_route = "never"
    gx_c = module_grads(m, x, f, G, kw, with_xyz=True)[2][-1]
    assert torch.isfinite(gx).all() and torch.isfinite(gx_c).all() and gx.abs().max() > 0
    r = ggr.ratio(gx.cpu(), gx_c.cpu().double(), C_GROUP_MLP_GRAD)
    print(f"RATIO module-{mode}-{'full' if lengths is None else 'short'} xyz fused/composed={r:.3f}")
    assert r <= 1.0, f"xyz.grad: {r:.2f} x the bound between the two routes"


def test_sa_module_keeps_the_composition_when_it_must(monkeypatch):
    """grad_route = "measured" with a class absent from the table, and a training-mode BatchNorm under "always", take the
    composition: a fused layer that raises proves it."""
    g = torch.Generator().manual_seed(42)
    m = sa_module(g, True).eval()
    x, f = dev(fr.clustered_cloud(g, MB, MN, 32), torch.randn(MB, 4, MN, generator=g) + 0.5)
    G = torch.randn(MB, 192, MP, generator=g).to(DEV)
    m.grad_route = "never"
    _, out_c, composed = module_grads(m, x, f, G, {})

    def boom(self, *a, **kw):
        raise AssertionError("the fused differentiable route was taken")
    monkeypatch.setattr(ops.HipBackend, "group_mlp_layer", boom)
    m.grad_route = "always"
    with pytest.raises(AssertionError, match="fused differentiable route"):
        module_grads(m, x, f, G, {})
    m.grad_route = "measured"
    monkeypatch.setattr(ops, "GROUP_MLP_GRAD_FUSED_CLASSES", {})
    assert not ops.group_mlp_grad_routes_fused(4, [32, 32, 64], 12, MB * MP)
    _, out_m, measured = module_grads(m, x, f, G, {})
    # (the composition's own backward does not repeat bit for bit: its library convolutions sum in no fixed order)
    assert torch.equal(out_m, out_c) and all(ggr.ratio(a.cpu(), b.cpu().double(), C_GROUP_MLP_GRAD) <= 1.0 for a, b in zip(measured, composed))
    m.grad_route = "always"
    m.train()
    _, out_t, trained = module_grads(m, x, f, G, {})
    assert torch.isfinite(out_t).all() and all(torch.isfinite(t).all() for t in trained)


def test_unsupported_shapes_launch_nothing():
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    x, f = torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 8, 8, device=DEV)
    idx = torch.zeros(1, 4, 16, dtype=torch.int32, device=DEV)
    order, seg = torch.zeros(1, 64, dtype=torch.int32, device=DEV), torch.zeros(1, 9, dtype=torch.int32, device=DEV)
    buf = torch.full((1 << 16,), 7.0, device=DEV)
    g = torch.zeros(1, 4, 256, device=DEV)
    p, i = _lib.fptr, _lib.iptr
    ptrs = (ctypes.c_void_p * 4)(p(buf), p(buf), p(buf), p(buf))
    for c, ns, use_xyz, widths in ((6, 16, 1, (32,)), (8, 65, 1, (32,)), (8, 0, 1, (32,)), (0, 16, 0, (32,)), (8, 16, 1, (48,)), (8, 16, 1, (256, 32)),
                                   (8, 16, 1, (32, 32, 32, 32)), (132, 16, 1, (32,))):
        rc = lib.mcp_group_mlp_grad(1, 8, 4, c, ns, use_xyz, 0, len(widths), w(*widths), p(x), p(x[:, :4].contiguous()), p(f), i(idx), None, None, p(buf),
                                    p(g), i(order), i(seg), p(buf) if c else None, p(buf) if use_xyz else None, p(buf) if use_xyz else None, None, ptrs, ptrs, p(buf),
                                    buf.data_ptr(), buf.numel() * 4, None)
        assert rc == 10002, (c, ns, use_xyz, widths, rc)
        assert lib.mcp_group_mlp_grad_workspace_bytes(1, 4, c, ns, use_xyz, len(widths), w(*widths)) == 0
    torch.cuda.synchronize()
    assert (buf == 7.0).all()
    be = ops.backend()
    with pytest.raises(_lib.Unsupported):
        be.group_mlp_grad(x, x[:, :4].contiguous(), f, idx, [(torch.zeros(48, 11, device=DEV), torch.zeros(48, device=DEV))], torch.zeros(1, 4, 48, device=DEV))
    with pytest.raises(_lib.Unsupported):
        ops.group_mlp_grad_pack_weights([(torch.zeros(48, 11, device=DEV), torch.zeros(48, device=DEV))])
    with pytest.raises(_lib.Unsupported):
        be.group_mlp_layer(x, x[:, :4].contiguous(), f.requires_grad_(True), idx, [(torch.zeros(48, 11, device=DEV), torch.zeros(48, device=DEV))])
