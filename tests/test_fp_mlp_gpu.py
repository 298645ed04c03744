"""-m gpu: the fused feature-propagation kernel (csrc/fp_mlp.hip, ops.HipBackend.fp_mlp) and PointnetFPModule on top of it
(mocopci_amd/pointnet2_modules.py) against the float64 statement of tests/fp_mlp_reference.py.

Every case asserts |kernel - exact| <= C * 2^-24 * bound element-wise and that the two-term mutant of the bf16 split lies outside that
bound on the same inputs, prints its RATIO line (with the fp32 composition's ratio on the same inputs beside it), and checks that a
second run and a kept operand image give identical bits.  Shapes: B = 3, n = 70, m = 37 -- 210 rows: six full 32-row tiles and one of
18, tiles crossing element boundaries, two workgroups; the widths reach the three register classes (2, 4, 8 accumulator tiles per
bank) on both sides of the staging predicate (image whole in LDS / streamed slab by slab)."""
import ctypes
import functools

import pytest
import torch

from mocopci_amd import _lib, ops, pointnet2_utils as pu
from tests import fp_mlp_reference as fpr
from tests import fused_reference as fr
from tests.test_kernel_variants_gpu import two_term

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = fr.U
# C_GROUP_MLP / C_CROSS: the largest constant the families on this split chain carry, taken from them and not tuned on this kernel.
# Worst measured ratio per instantiation fp_mlp_kernel<TMAX, streamed> (case, rule; the fp32 composition on the same inputs):
#   <2, whole>    0.175 (c4+0-32, pointnet2; 0.149), 0.241 through the module      <2, streamed> 0.146 (c256+128-64, pointnet2; 0.061)
#   <4, whole>    0.247 (c4+0-128, pointnet2; 0.150)                                <4, streamed> 0.071 (c128+4-128x128x128, given; 0.074)
#   <8, whole>    0.535 (c4+0-256, given; 0.247)                                    <8, streamed> 0.083 (c256+3-256x256, pointnet2; 0.033)
C_FP_MLP = 2.0
B, N, M = 3, 70, 37


def case(c2, c1, widths):
    return dict(b=B, n=N, m=M, c2=c2, c1=c1, widths=widths)


def case_id(k):
    return f"c{k['c2']}+{k['c1']}-{'x'.join(map(str, k['widths']))}"


CASES = [
    case(4, 0, [32]),
    case(20, 0, [64, 32]),                 # partial k-step
    case(64, 3, [64, 64]),                 # unaligned skip rows
    case(128, 4, [128, 128, 128]),
    case(256, 3, [256, 256]),
    case(256, 64, [256, 128]),
    case(256, 128, [256, 256]),
    case(512, 256, [256, 256]),            # the largest image, streamed
    case(64, 64, [32, 256]),
    case(256, 128, [64]), case(4, 0, [128]), case(4, 0, [256]),   # <2, streamed>, <4, whole>, <8, whole>
]
OTHER_RULES = [CASES[1], CASES[2], CASES[3], CASES[7], CASES[11]]   # rules 2 and 0: every register class, both stagings, a wide case


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def pack(d):
    return ops.fp_mlp_pack_weights([tuple(dev(w, b)) for w, b in d["weights"]], d["known_feats"].shape[-1])


def run_kernel(d, rule, packed=None, lengths=None, **repl):
    t = {**d, **repl}
    packed = pack(d) if packed is None else packed
    f, s, i, dist, w3 = dev(t["known_feats"], t["skip"], t["idx"], t["dist"], t["w3"])
    return ops.backend().fp_mlp(f, s, i, dist, *packed, rule=rule, w3=w3 if rule == "given" else None, unknown_lengths=lengths), packed


@functools.lru_cache(maxsize=None)
def reference(key, rule, cut):
    d = fpr.fp_mlp_inputs(dict(b=key[0], n=key[1], m=key[2], c2=key[3], c1=key[4], widths=list(key[5])))
    return fpr.fp_mlp_reference(d["known_feats"], d["skip"], d["idx"], d["dist"], d["weights"], rule=rule, w3=d["w3"], cut=two_term if cut else None)


def case_reference(k, rule):
    key = (k["b"], k["n"], k["m"], k["c2"], k["c1"], tuple(k["widths"]))
    return lambda cut=None: reference(key, rule, cut is not None)


def judge(name, got, ref, composed=None, rows=None, mutant_outside=True):
    got = got.reshape(-1, got.shape[-1]).double().cpu()
    assert torch.isfinite(got).all()
    exact, bound = ref()
    mutant = ref(cut=two_term)[0]
    if rows is not None:
        got, exact, bound, mutant = got[rows], exact[rows], bound[rows], mutant[rows]
    tol = (C_FP_MLP * U * bound).clamp_min(1e-300)
    ratio = ((got - exact).abs() / tol).max().item()
    ratio2 = ((got - mutant).abs() / tol).max().item()
    line = f"RATIO {name} kernel={ratio:.3f} two_term={ratio2:.2f}"
    if composed is not None:
        comp = composed.reshape(-1, composed.shape[-1]).double().cpu()
        comp = comp if rows is None else comp[rows]
        line += f" composed_fp32={((comp - exact).abs() / tol).max().item():.3f}"
    print(line)
    assert ratio <= 1.0, f"fp_mlp {name}: error {ratio:.2f} x the bound"
    if mutant_outside:
        assert ratio2 > 1.0, f"the bound does not tell a two-term split from the kernel's three terms ({ratio2:.2f})"
    return ratio


def check_case(k, rule):
    d = fpr.fp_mlp_inputs(k)
    got, packed = run_kernel(d, rule)
    assert got.shape == (B, N, k["widths"][-1])
    assert torch.equal(run_kernel(d, rule)[0], got), "not bit-reproducible (operand image built again)"
    assert torch.equal(run_kernel(d, rule, packed=packed)[0], got), "operand image kept"
    f, s, i, dist, w3 = dev(d["known_feats"], d["skip"], d["idx"], d["dist"], d["w3"])
    composed = fpr.composition(f, s, i, dist, [tuple(dev(w, b)) for w, b in d["weights"]], rule=rule, w3=w3)
    judge(f"{case_id(k)}-{rule}", got, case_reference(k, rule), composed)


@pytest.mark.parametrize("case_", CASES, ids=case_id)
def test_fp_mlp_matches_float64(case_):
    check_case(case_, "pointnet2")


@pytest.mark.parametrize("rule", ["flownet3d", "given"])
@pytest.mark.parametrize("case_", OTHER_RULES, ids=case_id)
def test_fp_mlp_other_rules_match_float64(case_, rule):
    check_case(case_, rule)


def test_cases_reach_every_register_class_on_both_sides_of_the_staging_predicate():
    """(accumulator tiles per bank, image whole in LDS): the six instantiations of fp_mlp_kernel."""
    inst = lambda k: (ops.fp_mlp_tmax(k["widths"]), ops.fp_mlp_weights_in_lds(k["c2"], k["c1"], k["widths"]))
    everything = {(t, s) for t in (2, 4, 8) for s in (True, False)}
    assert {inst(k) for k in CASES} == everything and {inst(k) for k in OTHER_RULES} >= {(2, True), (4, False), (8, False), (8, True)}
    assert not ops.fp_mlp_weights_in_lds(512, 256, [256, 256])


# ---- lengths ---------------------------------------------------------------------------------------------------------------------------
NAN = float("nan")
LEN_CASES = [case(64, 3, [64, 64]), case(128, 4, [128, 128, 128]), case(256, 64, [256, 128])]


def searched(d, ulen, klen):
    """dist / idx of pu.three_nn under the lengths, and the inputs with every padded row poisoned (idx stays 0 there)."""
    u, k = dev(d["unknown"], d["known"])
    dist, idx = pu.three_nn(u, k, list(ulen), list(klen))
    dist, idx = dist.cpu(), idx.cpu()
    feats, skip, w3 = d["known_feats"].clone(), None if d["skip"] is None else d["skip"].clone(), d["w3"].clone()
    for b, (nu, nk) in enumerate(zip(ulen, klen)):
        feats[b, nk:] = NAN
        dist[b, nu:] = NAN
        w3[b, nu:] = NAN
        assert (idx[b, nu:] == 0).all() and (idx[b] >= 0).all() and (idx[b] < max(nk, 1)).all()
        if skip is not None:
            skip[b, nu:] = NAN
    return dict(d, known_feats=feats, skip=skip, dist=dist.contiguous(), idx=idx.contiguous(), w3=w3)


@pytest.mark.parametrize("rule", ["pointnet2", "flownet3d"])
@pytest.mark.parametrize("case_", LEN_CASES, ids=case_id)
def test_lengths_give_the_sliced_call_and_zeros(case_, rule):
    """Unknown lengths (70, 41, 0 | 9) over known lengths (37, 2, 0), every padded row of skip, known_feats, dist and w3 refilled with
    NaN: live rows equal, bit for bit, the call on the element's sliced prefixes; padded rows are exact zeros; the element with two
    known points weighs its third slot with exactly 0 and never reads that slot's row; the element without a known point gives the
    MLP of [0 | skip]."""
    d = fpr.fp_mlp_inputs(case_)
    klen = (37, 2, 0)
    packed = pack(d)
    for ulen in ((70, 41, 0), (70, 41, 9)):
        t = searched(d, ulen, klen)
        assert torch.isinf(t["dist"][1, :41, 2]).all() and torch.isfinite(t["dist"][1, :41, :2]).all() and torch.isinf(t["dist"][2, :ulen[2]]).all()
        got, _ = run_kernel(t, rule, packed=packed, lengths=list(ulen))
        assert torch.isfinite(got).all()
        lens_dev = torch.tensor(ulen, dtype=torch.int64, device=DEV)
        assert torch.equal(run_kernel(t, rule, packed=packed, lengths=lens_dev)[0], got)
        for b, (nu, nk) in enumerate(zip(ulen, klen)):
            assert (got[b, nu:] == 0).all(), f"element {b}: padded rows are not exact zeros"
            if nu:
                part = {k: None if t[k] is None else t[k][b:b + 1, :nu].contiguous() for k in ("skip", "idx", "dist", "w3")}
                part["known_feats"] = t["known_feats"][b:b + 1, :max(nk, 1)].contiguous()
                assert torch.equal(run_kernel(dict(t, **part), rule, packed=packed)[0][0], got[b, :nu]), f"element {b}: live rows differ from the sliced call"
        # the third slot of element 1 weighs exactly 0 and its row is not read: pointing it at a poisoned row changes no bit
        moved = t["idx"].clone()
        moved[1, :41, 2] = 5
        assert torch.equal(run_kernel(dict(t, idx=moved), rule, packed=packed, lengths=list(ulen))[0], got)
        # against the float64 statement on the same inputs: the two-point element, and the element without a known point = MLP of [0 | skip]
        ref = lambda cut=None: fpr.fp_mlp_reference(t["known_feats"], t["skip"], t["idx"], t["dist"], t["weights"], rule=rule, cut=cut)
        live = torch.cat([torch.arange(nu) + b * N for b, nu in enumerate(ulen)])
        judge(f"{case_id(case_)}-{rule}-ulen{ulen[2]}", got, ref, rows=live)
        if ulen[2]:
            x = torch.cat([torch.zeros(ulen[2], case_["c2"]), d["skip"][2, :ulen[2]]], -1).double()
            for wl, bias in d["weights"]:
                x = torch.relu(x @ wl.double().T + bias.double())
            rows = torch.arange(ulen[2]) + 2 * N
            assert torch.allclose(ref()[0][rows], x, rtol=1e-12, atol=1e-12), "the statement of an element without a known point is the MLP of [0 | skip]"
            # (a row of zeros and C1 skip values excites too few products for the mutant to stand out: the case as a whole shows that)
            judge(f"{case_id(case_)}-{rule}-no-known-point", got, ref, rows=rows, mutant_outside=False)


def test_lengths_under_given_weights_and_full_lengths():
    """Rule "given" reads no distance: padded rows of skip and w3 poisoned, dist absent.  Full lengths give the bits of the
    length-free call, for every rule."""
    k = LEN_CASES[0]
    d = fpr.fp_mlp_inputs(k)
    packed = pack(d)
    ulen = (70, 41, 0)
    skip, w3 = d["skip"].clone(), d["w3"].clone()
    for b, nu in enumerate(ulen):
        skip[b, nu:] = NAN
        w3[b, nu:] = NAN
    t = dict(d, skip=skip, w3=w3, dist=None)
    got, _ = run_kernel(t, "given", packed=packed, lengths=list(ulen))
    whole, _ = run_kernel(d, "given", packed=packed)
    for b, nu in enumerate(ulen):
        assert (got[b, nu:] == 0).all() and torch.equal(got[b, :nu], whole[b, :nu])
    for rule in fpr.RULES:
        free, _ = run_kernel(d, rule, packed=packed)
        assert torch.equal(run_kernel(d, rule, packed=packed, lengths=[N] * B)[0], free)
        assert torch.equal(run_kernel(d, rule, packed=packed, lengths=torch.full((B,), N + 5, dtype=torch.int32, device=DEV))[0], free), "clamped to n"


def test_unsupported_shapes_launch_nothing():
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    assert lib.mcp_fp_mlp_packed_floats(6, 0, 1, w(32)) == 0 and lib.mcp_fp_mlp_packed_floats(4, 0, 1, w(48)) == 0
    assert lib.mcp_fp_mlp_packed_floats(512, 260, 1, w(32)) == 0 and lib.mcp_fp_mlp_packed_floats(4, 0, 4, w(32, 32, 32, 32)) == 0
    assert lib.mcp_fp_mlp_packed_floats(20, 3, 2, w(64, 32)) == (2 * 3 + 1 * 4) * 768 + 96
    out = torch.full((1, 8, 32), 7.0, device=DEV)
    f, s = torch.zeros(1, 4, 512, device=DEV), torch.zeros(1, 8, 512, device=DEV)
    idx, dist, pk = torch.zeros(1, 8, 3, dtype=torch.int32, device=DEV), torch.ones(1, 8, 3, device=DEV), torch.zeros(4096, device=DEV)
    p, i = _lib.fptr, _lib.iptr
    for c2, c1, widths in ((6, 0, (32,)), (4, 0, (48,)), (4, 0, (32, 32, 32, 32)), (512, 260, (32,)), (0, 4, (32,)), (516, 0, (32,)), (4, 0, (512,))):
        rc = lib.mcp_fp_mlp(1, 8, 4, c2, c1, 1, len(widths), w(*widths), p(f), p(s), i(idx), p(dist), None, None, p(pk), p(out), None)
        assert rc == 10002, (c2, c1, widths, rc)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    be = ops.backend()
    for c2, c1, widths in ((6, 0, [32]), (4, 0, [48]), (4, 0, [32, 32, 32, 32]), (512, 260, [32])):
        with pytest.raises(_lib.Unsupported):
            be.fp_mlp(f[:, :, :c2].contiguous(), s[:, :, :c1].contiguous() if c1 else None, idx, dist, pk, widths)
    with pytest.raises(_lib.Unsupported):
        ops.fp_mlp_pack_weights([(torch.zeros(48, 7, device=DEV), torch.zeros(48, device=DEV))], 4)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- module ----------------------------------------------------------------------------------------------------------------------------
MB, MN, MM, MC2, MC1 = 2, 300, 80, 64, 3


def fp_module(g, weighting, route="always"):
    from mocopci_amd.pointnet2_modules import PointnetFPModule
    m = PointnetFPModule(mlp=[MC2 + MC1, 64, 32])
    state = {}
    for k, v in m.state_dict().items():
        shape = list(v.shape)
        if k.endswith("conv.weight"):
            state[k] = 2.0 * (torch.randn(shape, generator=g) + 1.0) / shape[1]
        elif k.endswith("num_batches_tracked"):
            state[k] = torch.tensor(3)
        elif k.endswith("running_var") or k.endswith("bn.weight"):
            state[k] = torch.rand(shape, generator=g) + 0.5
        else:
            state[k] = torch.randn(shape, generator=g) * 0.1 - 0.1
    m.load_state_dict(state, strict=True)
    m.weighting, m.route = weighting, route
    return m.to(DEV)


def module_inputs(g):
    known = fr.clustered_cloud(g, MB, MM, 16)
    unknown = (known[:, torch.arange(MN) * MM // MN] + 0.3 * torch.randn(MB, MN, 3, generator=g)).contiguous()
    return unknown, known, torch.randn(MB, MC1, MN, generator=g) + 0.5, torch.randn(MB, MC2, MM, generator=g) + 0.5


def forbid_fused(monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("the fused route was taken")
    monkeypatch.setattr(ops.HipBackend, "fp_mlp", boom)


@pytest.mark.parametrize("lengths", [None, ((300, 120), (80, 2)), ((300, 50), (80, 0))], ids=["full", "short", "no-known-point"])
@pytest.mark.parametrize("weighting", ["pointnet2", "flownet3d"])
def test_fp_module_fused_against_its_composition(weighting, lengths):
    g = torch.Generator().manual_seed(21)
    m = fp_module(g, weighting).eval()
    unknown, known, skip, feats = module_inputs(g)
    kw = {} if lengths is None else dict(unknown_lengths=list(lengths[0]), known_lengths=list(lengths[1]))
    if lengths is not None:   # padded rows are never read
        for b, (nu, nk) in enumerate(zip(*lengths)):
            skip[b, :, nu:] = NAN
            feats[b, :, nk:] = NAN
    u, k, s, f = dev(unknown, known, skip, feats)
    with torch.no_grad():
        out = m(u, k, s, f, **kw)
        again = m(u, k, s, f, **kw)
        m.route = "never"
        # the composition reads padded rows (and zeroes what they give): hand it finite ones
        composed = m(u, k, torch.nan_to_num(s), torch.nan_to_num(f), **kw)
        dist, idx = pu.three_nn(u, k, *(None, None) if lengths is None else (list(lengths[0]), list(lengths[1])))
    assert out.shape == (MB, 32, MN) and torch.equal(again, out) and torch.isfinite(out).all() and torch.isfinite(composed).all()
    nu_all = (MN,) * MB if lengths is None else lengths[0]
    for b, nu in enumerate(nu_all):
        assert (out[b, :, nu:] == 0).all() and (composed[b, :, nu:] == 0).all()
    convs, bns = m._layers()
    ws = [tuple(t.cpu() for t in ops.fold_conv_bn(c, b)) for c, b in zip(convs, bns)]
    rows_f, rows_s = feats.transpose(1, 2).contiguous(), skip.transpose(1, 2).contiguous()
    ref = lambda cut=None: fpr.fp_mlp_reference(rows_f, rows_s, idx.cpu(), dist.cpu(), ws, rule=weighting, cut=cut)
    live = torch.cat([torch.arange(nu) + b * MN for b, nu in enumerate(nu_all)])
    judge(f"module-{weighting}", out.transpose(1, 2), ref, composed.transpose(1, 2), rows=live)
    if lengths is not None and lengths[1][1] == 0:   # an element without a known point: the MLP of [0 | skip]
        nu = lengths[0][1]
        x = torch.cat([torch.zeros(nu, MC2), rows_s[1, :nu]], -1).double()
        for wl, bias in ws:
            x = torch.relu(x @ wl.double().T + bias.double())
        assert torch.allclose(ref()[0][MN:MN + nu], x, rtol=1e-12, atol=1e-12)
        assert torch.allclose(composed[1, :, :nu].T.double().cpu(), x, rtol=1e-4, atol=1e-5)


def test_fp_module_takes_the_composition_when_it_must(monkeypatch):
    g = torch.Generator().manual_seed(22)
    m = fp_module(g, "pointnet2").eval()
    u, k, s, f = dev(*module_inputs(g))
    with torch.no_grad():
        fused = m(u, k, s, f)
        image = m.__dict__["_packed"][1][0]
        m(u, k, s, f)
        assert m.__dict__["_packed"][1][0] is image, "the operand image is kept"
        m.mlp.layer0.conv.weight.mul_(0.5)                           # a parameter written in place: the image is rebuilt
        assert not torch.equal(m(u, k, s, f), fused) and m.__dict__["_packed"][1][0] is not image
        m.mlp.layer0.conv.weight.mul_(2.0)
        assert torch.equal(m(u, k, s, f), fused)
    forbid_fused(monkeypatch)
    with torch.no_grad():
        with pytest.raises(AssertionError, match="fused route"):
            m(u, k, s, f)
        m.route = "never"
        composed = m(u, k, s, f)
        m.route = "measured"
        if not ops.fp_mlp_routes_fused(MC2, MC1, [64, 32], MB * MN):
            assert torch.equal(m(u, k, s, f), composed)   # a class without a measured row keeps the composition
        m.route = "always"
        assert m(u, None, s, f[:, :, :1].contiguous()).shape == (MB, 32, MN)   # known=None: the broadcast
    assert torch.allclose(composed, fused, rtol=1e-4, atol=1e-5)
    f.requires_grad_(True)                                           # a gradient wanted
    out_g = m(u, k, s, f)
    assert out_g.requires_grad and torch.allclose(out_g, fused, rtol=1e-4, atol=1e-5)
    f.requires_grad_(False)
    m.train()                                                        # batch statistics
    with torch.no_grad():
        m(u, k, s, f)


@pytest.mark.parametrize("weighting", ["pointnet2", "flownet3d"])
def test_fp_module_backward_in_train_mode(weighting):
    g = torch.Generator().manual_seed(23)
    m = fp_module(g, weighting).train()
    u, k, s, f = dev(*module_inputs(g))
    s.requires_grad_(True)
    f.requires_grad_(True)
    out = m(u, k, s, f, unknown_lengths=[300, 120], known_lengths=[80, 2])
    out.square().mean().backward()
    assert torch.isfinite(out).all()
    for t in (s, f):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().sum() > 0
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
