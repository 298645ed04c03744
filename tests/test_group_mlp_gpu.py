"""-m gpu: the fused set-abstraction kernel (csrc/group_mlp.hip, ops.HipBackend.group_mlp) and the modules on top of it
(mocopci_amd/pointnet2_modules.py) against the float64 statement of tests/group_mlp_reference.py.

Every case asserts |kernel - exact| <= C * 2^-24 * bound element-wise and that the two-term mutant of the bf16 split lies outside that
bound on the same inputs, prints its RATIO line (with the fp32 composition's ratio on the same inputs beside it), and checks that a
second run and a kept operand image give identical bits.  Shapes: B = 3, M = 37, N = 500 -- with 4, 2 or 1 centres per 32-column tile
the last tile has fewer centres than groups and tiles cross element boundaries; nsample covers the group widths 8, 16, 32, partial
groups and the two-tile form; the widths reach both register classes and both sides of the LDS / L2 weight predicate."""
import ctypes

import pytest
import torch

from mocopci_amd import _lib, ops
from tests import fused_reference as fr
from tests import group_mlp_reference as gr
from tests.test_kernel_variants_gpu import two_term

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = fr.U
# the largest constant the families on this split chain carry (C_CROSS of test_fused_variants_gpu.py), not tuned on this kernel
C_GROUP_MLP = 2.0          # group_mlp_kernel<4 | 8, lds | l2> [0.659, c4-ns16-256; 0.192 through the modules]
B, M, N = 3, 37, 500


def case(c, nsample, widths, **kw):
    return dict(b=B, n=N, m=M, c=c, nsample=nsample, widths=widths, **kw)


def case_id(k):
    extra = "".join(f"-{n}={k[n]}" for n in ("pool", "c2", "use_xyz", "extent") if n in k)
    return f"c{k['c']}-ns{k['nsample']}-{'x'.join(map(str, k['widths']))}{extra}"


CASES = [
    *[case(4, ns, [32, 32, 64]) for ns in (8, 12, 16, 24, 32, 64)],          # group widths 8, 16, 32; partial groups; two tiles
    case(0, 16, [32]),                                                      # coordinates only, one layer
    case(64, 16, [64, 64, 128]),
    case(128, 8, [128, 128, 256]),
    case(64, 16, [64, 64, 128], use_xyz=False),
    case(4, 12, [32, 32, 64], pool="mean"), case(4, 8, [32, 64], pool="mean"), case(64, 64, [64, 64, 128], pool="mean"),
    case(128, 32, [128, 128, 256], pool="mean", extent=True),
    case(4, 16, [256]), case(80, 24, [32, 128]),                            # eight output tiles of layer 1; feature k-steps rounded up
    case(64, 16, [64, 64], c2=64, extent=True),                             # FlowEmbedding form: the centre's features as row_bias
    case(64, 64, [32, 32, 64], c2=64, pool="mean"),
]


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def split_centre(case_, ws):
    """The first layer's columns over [coordinates | features] and those over the centre's own features."""
    w1, b1 = ws[0]
    k = w1.shape[1] - case_.get("c2", 0)
    return [(w1[:, :k].contiguous(), b1), *ws[1:]], w1[:, k:].contiguous()


def run_kernel(case_, xyz, new_xyz, feats, idx, centre, ws, lengths=None, row_bias=None, packed=None):
    be = ops.backend()
    kw = dict(pool=case_.get("pool", "max"), use_xyz=case_.get("use_xyz", True))
    if centre is not None:
        ws, wc = split_centre(case_, ws)
        if row_bias is None:
            row_bias = be.linear(centre.to(DEV), wc.to(DEV))              # the centre's features through mcp_linear, once per centre
    if packed is None:
        packed = ops.group_mlp_pack_weights([tuple(dev(w, b)) for w, b in ws], use_xyz=kw["use_xyz"])
    x, c, f, i = dev(xyz, new_xyz, feats, idx)
    return be.group_mlp(x, c, f, i, *packed, new_xyz_lengths=lengths, row_bias=row_bias, **kw), packed, row_bias


def judge(name, got, ref, composed=None):
    got = got.reshape(-1, got.shape[-1]).double().cpu()
    assert torch.isfinite(got).all()
    exact, bound = ref()
    tol = (C_GROUP_MLP * U * bound).clamp_min(1e-300)
    ratio = ((got - exact).abs() / tol).max().item()
    ratio2 = ((got - ref(cut=two_term)[0]).abs() / tol).max().item()
    line = f"RATIO {name} kernel={ratio:.3f} two_term={ratio2:.2f}"
    if composed is not None:
        line += f" composed_fp32={((composed.reshape(exact.shape).double().cpu() - exact).abs() / tol).max().item():.3f}"
    print(line)
    assert ratio <= 1.0, f"group_mlp {name}: error {ratio:.2f} x the bound"
    assert ratio2 > 1.0, f"the bound does not tell a two-term split from the kernel's three terms ({ratio2:.2f})"
    return ratio


@pytest.mark.parametrize("case_", CASES, ids=case_id)
def test_group_mlp_matches_float64(case_):
    xyz, new_xyz, feats, idx, centre, ws = gr.group_mlp_inputs(case_)
    kw = dict(use_xyz=case_.get("use_xyz", True), pool=case_.get("pool", "max"), centre=centre)
    got, packed, _ = run_kernel(case_, xyz, new_xyz, feats, idx, centre, ws)
    assert got.shape == (B, M, case_["widths"][-1])
    assert torch.equal(run_kernel(case_, xyz, new_xyz, feats, idx, centre, ws)[0], got), "not bit-reproducible (operand image built again)"
    assert torch.equal(run_kernel(case_, xyz, new_xyz, feats, idx, centre, ws, packed=packed)[0], got), "operand image kept"
    composed = gr.composition(*dev(xyz, new_xyz, feats, idx), [tuple(dev(w, b)) for w, b in ws], use_xyz=kw["use_xyz"], pool=kw["pool"],
                              centre=None if centre is None else centre.to(DEV))
    judge(case_id(case_), got, lambda **k: gr.group_mlp_reference(xyz, new_xyz, feats, idx, ws, **kw, **k), composed)


def test_cases_reach_both_sides_of_the_weight_predicate_and_both_register_classes():
    """(one wave per SIMD, weights in LDS) in all four combinations: the four instantiations of group_mlp_kernel."""
    wide = lambda k: k["c"] > 64 or max(k["widths"][:-1], default=0) > 64
    reached = {(wide(k), ops.group_mlp_weights_in_lds(k["c"], k["widths"])) for k in CASES}
    assert reached == {(w, s) for w in (True, False) for s in (True, False)}


@pytest.mark.parametrize("source", ["tiny-radius", "ball", "knn"])
def test_group_mlp_on_searched_neighbour_lists(source):
    """idx as the searches make it: a radius so small that every slot is the first hit (the centre itself) or point 0, a ball query
    with its first-hit padding, and a KNN list (K = 16)."""
    case_ = case(4, 16, [32, 32, 64])
    xyz, new_xyz, feats, _, _, ws = gr.group_mlp_inputs(case_)
    be = ops.backend()
    x, c = dev(xyz, new_xyz)
    if source == "knn":
        idx = be.knn(c, x, 16)
    else:
        idx = be.ball_query(x, c, 1e-3 if source == "tiny-radius" else 0.7, 16)
    idx = idx.cpu()
    if source == "tiny-radius":
        own = (torch.arange(M) * N // M).view(1, M, 1)
        assert ((idx == own) | (idx == 0)).all()
    got, _, _ = run_kernel(case_, xyz, new_xyz, feats, idx, None, ws)
    judge(source, got, lambda **k: gr.group_mlp_reference(xyz, new_xyz, feats, idx, ws, **k))


@pytest.mark.parametrize("case_", [case(4, 8, [32, 32, 64]), case(64, 12, [64, 64], c2=64), case(4, 64, [32, 64], pool="mean")], ids=case_id)
def test_lengths_give_the_sliced_call_and_zeros(case_):
    """new_xyz_lengths (37, 20, 0) with the padding of new_xyz, idx and row_bias refilled with NaN and out-of-range indices: live rows
    equal, bit for bit, the call on the sliced prefix, padded rows are exact zeros."""
    lens = (37, 20, 0)
    xyz, new_xyz, feats, idx, centre, ws = gr.group_mlp_inputs(case_)
    whole, packed, row_bias = run_kernel(case_, xyz, new_xyz, feats, idx, centre, ws)
    bad_xyz, bad_idx = new_xyz.clone(), idx.clone()
    bad_rb = None if row_bias is None else row_bias.clone()
    for b, n in enumerate(lens):
        bad_xyz[b, n:] = float("nan")
        bad_idx[b, n:] = 1 << 30
        if bad_rb is not None:
            bad_rb[b, n:] = float("nan")
    got, _, _ = run_kernel(case_, xyz, bad_xyz, feats, bad_idx, centre, ws, lengths=list(lens), row_bias=bad_rb, packed=packed)
    lens_dev = torch.tensor(lens, dtype=torch.int64, device=DEV)
    assert torch.equal(run_kernel(case_, xyz, bad_xyz, feats, bad_idx, centre, ws, lengths=lens_dev, row_bias=bad_rb, packed=packed)[0], got)
    for b, n in enumerate(lens):
        assert (got[b, n:] == 0).all(), f"element {b}: padded centres are not exact zeros"
        if n:
            part, _, _ = run_kernel(case_, xyz[b:b + 1], new_xyz[b:b + 1, :n], None if feats is None else feats[b:b + 1], idx[b:b + 1, :n],
                                    centre, ws, row_bias=None if row_bias is None else row_bias[b:b + 1, :n].contiguous(), packed=packed)
            assert torch.equal(part[0], got[b, :n]), f"element {b}: live rows differ from the call on the sliced prefix"
            assert torch.equal(whole[b, :n], got[b, :n])


def test_unsupported_shapes_launch_nothing():
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    assert lib.mcp_group_mlp_packed_floats(6, 1, w(32)) == 0 and lib.mcp_group_mlp_packed_floats(4, 2, w(256, 32)) == 0
    assert lib.mcp_group_mlp_packed_floats(4, 3, w(32, 32, 64)) == 7 * 768 + 128 + 128
    out = torch.full((1, 4, 32), 7.0, device=DEV)
    x, idx, pk = torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 4, 16, dtype=torch.int32, device=DEV), torch.zeros(4096, device=DEV)
    f = torch.zeros(1, 8, 8, device=DEV)
    p, i = _lib.fptr, _lib.iptr
    for c, ns, use_xyz, widths in ((6, 16, 1, (32,)), (8, 65, 1, (32,)), (8, 0, 1, (32,)), (0, 16, 0, (32,)), (8, 16, 1, (48,)), (8, 16, 1, (256, 32)),
                                   (8, 16, 1, (32, 32, 32, 32)), (132, 16, 1, (32,))):
        rc = lib.mcp_group_mlp(1, 8, 4, c, ns, use_xyz, 0, len(widths), w(*widths), p(x), p(x[:, :4].contiguous()), p(f), i(idx), None, None, p(pk), p(out), None)
        assert rc == 10002, (c, ns, use_xyz, widths, rc)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(_lib.Unsupported):
        ops.group_mlp_pack_weights([(torch.zeros(48, 7, device=DEV), torch.zeros(48, device=DEV))])


# ---- modules -------------------------------------------------------------------------------------------------------------------------
def sa_module(g, route):
    from mocopci_amd.pointnet2_modules import PointnetSAModuleMSG
    import json
    import os
    spec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet2_sa_state_keys.json")))
    state = {}
    for k, shape in spec.items():
        if k.endswith("conv.weight"):
            state[k] = (2.0 * (torch.randn(shape, generator=g) + 1.0) / shape[1])
        elif k.endswith("num_batches_tracked"):
            state[k] = torch.tensor(3)
        elif k.endswith("running_var") or k.endswith("bn.weight"):
            state[k] = torch.rand(shape, generator=g) + 0.5
        else:
            state[k] = torch.randn(shape, generator=g) * 0.1 - 0.1
    m = PointnetSAModuleMSG(npoint=128, radii=[0.7, 1.5], nsamples=[12, 24], mlps=[[4, 32, 32, 64], [4, 64, 64, 128]])
    m.load_state_dict(state, strict=True)   # exactly the fixture's keys
    m.route = route
    return m.to(DEV)


def count_fused(monkeypatch):
    calls = []
    real = ops.HipBackend.group_mlp
    monkeypatch.setattr(ops.HipBackend, "group_mlp", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    return calls


def test_sa_module_msg_fused_composed_and_trained(monkeypatch):
    g = torch.Generator().manual_seed(11)
    xyz = fr.clustered_cloud(g, 2, 3000, 32)
    feats = torch.randn(2, 4, 3000, generator=g) + 0.5
    m = sa_module(g, "always").eval()
    calls = count_fused(monkeypatch)
    x, f = dev(xyz, feats)
    with torch.no_grad():
        new_xyz, out = m(x, f)
        assert len(calls) == 2, "both scales take the fused route under no-grad in eval()"
        again = m(x, f)[1]
        m.route = "never"
        composed = m(x, f)[1]
        m.route = "measured"
        assert torch.equal(m(x, f)[1], composed) or len(calls) > 4   # without a measured row the route stays off
    assert out.shape == (2, 64 + 128, 128) and new_xyz.shape == (2, 128, 3) and torch.equal(again, out)
    be = ops.backend()
    at = 0
    for i, (r, ns) in enumerate(((0.7, 12), (1.5, 24))):
        idx = be.ball_query(x, new_xyz, r, ns).cpu()
        convs, bns = m._layers(i)
        ws = [tuple(t.cpu() for t in ops.fold_conv_bn(c, b)) for c, b in zip(convs, bns)]
        width = ws[-1][0].shape[0]
        rows = feats.transpose(1, 2).contiguous()
        ref = lambda **k: gr.group_mlp_reference(xyz, new_xyz.cpu(), rows, idx, ws, **k)
        judge(f"module-scale{i}", out[:, at:at + width].transpose(1, 2), ref, composed[:, at:at + width].transpose(1, 2))
        at += width
    # a gradient wanted: the composition, with finite gradients for features and weights
    m.route = "always"
    before = len(calls)
    f.requires_grad_(True)
    out_g = m(x, f)[1]
    out_g.square().mean().backward()
    assert len(calls) == before and torch.allclose(out_g, out, rtol=1e-4, atol=1e-5)
    assert torch.isfinite(f.grad).all() and f.grad.abs().sum() > 0
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    # train() mode normalises with batch statistics: the composition
    m.train()
    with torch.no_grad():
        m(x, f.detach())
    assert len(calls) == before


def test_sa_module_falls_back_on_unsupported_widths_and_keeps_its_pack(monkeypatch):
    from mocopci_amd.pointnet2_modules import PointnetSAModule
    g = torch.Generator().manual_seed(12)
    xyz = fr.clustered_cloud(g, 2, 600, 32).to(DEV)
    feats = (torch.randn(2, 8, 600, generator=g) + 0.5).to(DEV)
    calls = count_fused(monkeypatch)
    odd = PointnetSAModule(mlp=[8, 48], npoint=32, radius=1.0, nsample=16).to(DEV).eval()
    odd.route = "always"
    m = PointnetSAModule(mlp=[8, 32, 64], npoint=32, radius=1.0, nsample=16, pool_method="avg_pool").to(DEV).eval()
    m.route = "always"
    with torch.no_grad():
        assert odd(xyz, feats)[1].shape == (2, 48, 32) and not calls
        first = m(xyz, feats)[1]
        image = m.__dict__["_packed"][0][1][0]
        assert m(xyz, feats)[1].data_ptr() != first.data_ptr() and m.__dict__["_packed"][0][1][0] is image, "the operand image is kept"
        m.route = "never"
        assert torch.allclose(m(xyz, feats)[1], first, rtol=1e-4, atol=1e-5)
        m.route = "always"
        m.mlps[0].layer0.conv.weight.mul_(0.5)                       # a parameter written in place: the image is rebuilt
        second = m(xyz, feats)[1]
        assert m.__dict__["_packed"][0][1][0] is not image and not torch.equal(second, first)
        # lengths: padded centres give zeros on both routes
        lens = [600, 300]
        a = m(xyz, feats, xyz_lengths=lens, new_xyz_lengths=[32, 10])[1]
        m.route = "never"
        b = m(xyz, feats, xyz_lengths=lens, new_xyz_lengths=[32, 10])[1]
        assert (a[1, :, 10:] == 0).all() and (b[1, :, 10:] == 0).all() and torch.allclose(a, b, rtol=1e-4, atol=1e-5)
