"""-m "not gpu": the float64 statement of the set-abstraction layer under a training-mode BatchNorm (tests/group_mlp_bn_reference.py)
against torch's own float64 composition, the input search of every GPU case, mutants of the statement that the GPU test's bound must
tell from it, and what of csrc/group_mlp_bn.hip needs no GPU: declarations, bindings, the shape predicate, the sizes."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from mocopci_amd import _lib, ops
from tests import group_mlp_bn_reference as gbr
from tests.group_mlp_bn_reference import case, case_id
from tests.test_abi_cpu import header_functions
from tests.test_fp_mlp_grad_cpu import C_CAP

# The GPU cases (tests/test_group_mlp_bn_gpu.py), n = 200 points per cloud.  Pairs B M nsample: 168 = 128 + 32 + 8 (a partial last
# wave, 56 rows per element: rows crossing elements inside a wave), 252, 336, 672 (six workgroups: the cross-workgroup merge), 640
# (nsample 64: two 32-row tiles per centre), 24 (one partial wave only), 256 (exactly two full workgroups); nsample 12 is no power of
# two; c 0 (positions only), 4, 64, 80, 128 and the widths reach the three register classes and both sides of the staging predicate.
CASES = [case(4, 8, [32, 32, 64]), case(4, 12, [32, 32, 64]), case(4, 16, [32, 32, 64]), case(4, 32, [32, 32, 64]),
         case(4, 64, [32, 32, 64], 2, 5), case(0, 16, [32]), case(64, 16, [64, 64, 128]), case(128, 8, [128, 128, 256]),
         case(128, 64, [128, 128, 256], 1, 3), case(4, 16, [256]), case(80, 24, [32, 128]), case(4, 8, [32, 32, 64], 1, 3),
         case(4, 8, [32, 32, 64], 2, 16)]
FURTHER = [case(64, 16, [64, 64, 128], use_xyz=False), case(4, 12, [32, 32, 64], pool="mean"), case(128, 64, [128, 128, 256], 1, 3, pool="mean")]
LENGTHS = (7, 3, 0)
OFFSET = 100.0
# every (case, offset, biased, lengths) the GPU tests pick
PICKS = [(k, 0.0, True, None) for k in CASES + FURTHER] + [(CASES[0], OFFSET, False, None), (CASES[0], 0.0, True, LENGTHS)]
pick_id = lambda p: f"{case_id(p[0])}-{p[1]}-{p[2]}-{p[3]}"


def composed(prep, leaves):
    """torch's own composition over the live centres in the leaves' precision (float64 here; the GPU tests print its fp32 error beside
    the kernel's): the grouped tensor, conv2d, batch_norm(training=True), relu, max_pool2d / avg_pool2d -> (out, [(mean, biased var)])."""
    x = gbr.gather_rows(leaves[:prep.point_leaves()], prep.data, prep.centres)   # (P, J, cin)
    h = x.permute(2, 0, 1)[None]                                                  # (1, cin, P, J)
    stats = []
    for (w, b, gamma, beta), e in zip(prep.layer_leaves(leaves), prep.eps):
        z = F.conv2d(h, w[:, :, None, None], b)
        stats.append((z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)))
        h = torch.relu(F.batch_norm(z, None, None, gamma, beta, True, 0.1, e))
    pool = F.max_pool2d if prep.data["pool"] == "max" else F.avg_pool2d
    return pool(h, kernel_size=[1, h.size(3)])[0, :, :, 0].T, stats


@pytest.mark.parametrize("pick", [PICKS[0], PICKS[1], PICKS[5], PICKS[13], PICKS[14], PICKS[16], PICKS[17]], ids=pick_id)
def test_reference_agrees_with_torchs_float64_composition(pick):
    prep = gbr.pick(*pick)
    out, stats, m, grads = gbr.exact(prep)
    l64 = [t.double().clone().requires_grad_(True) for t in prep.leaves]
    want, wstats = composed(prep, l64)
    wgrads = torch.autograd.grad(want, l64, prep.g[prep.centres])
    close = lambda a, b: (a - b).abs().max().item() <= 1e-10 * max(1.0, b.abs().max().item())
    assert m == len(prep.centres) * pick[0]["nsample"] and close(out[prep.centres], want.detach())
    for (mu, v), (wmu, wv) in zip(stats, wstats):
        assert close(mu, wmu.detach()) and close(v, wv.detach())
    for name, a, b in zip(prep.names, grads, wgrads):
        assert close(a, b), name
    for name, a in zip(prep.names, grads):
        if name[0] == "b" and name[1:].isdigit():
            assert a.abs().max().item() < 1e-10, f"{name}: the statistics absorb a bias, its gradient is zero in exact arithmetic"


@pytest.mark.parametrize("pick", PICKS, ids=pick_id)
def test_every_gpu_case_finds_clear_inputs_and_keeps_the_pool(pick):
    prep = gbr.pick(*pick)
    with torch.no_grad():
        _, (_, ys, _) = gbr.evaluate(prep)
    active = [float((y > 0).double().mean()) for y in ys]
    print(f"PICK {pick_id(pick)} seed={prep.seed} tries={prep.tries} pairs={prep.pairs()} min|y|={min(y.abs().min().item() for y in ys):.2e} "
          f"kept={prep.kept:.4f} active={' '.join(f'{a:.3f}' for a in active)}")
    assert gbr.clear(prep) and prep.tries <= gbr.TRIES
    assert prep.kept > 0.9, "the project's cap on what a clear mask may leave out"
    assert all(0.25 < a < 0.75 for a in active), active
    assert prep.pairs() * sum(pick[0]["widths"]) <= 1e5, "clearing every pair only works for small cases"


def worst(prep, got, which=None):
    """The largest ratio, at C_CAP, of a mutant's (out, stats, grads) against the statement's over the named tensors."""
    e_out, e_stats, _, e_grads = gbr.exact(prep)
    out, stats, grads = got
    pairs = [("out", out, e_out[prep.centres])]
    for l, ((mu, v), (emu, ev)) in enumerate(zip(stats, e_stats)):
        pairs += [(f"mean{l + 1}", mu, emu), (f"var{l + 1}", v, ev)]
    pairs += list(zip(prep.names, grads, e_grads))
    return max(gbr.ratio(a, e, C_CAP) for n, a, e in pairs if e.abs().max().item() > 0 and (which is None or n in which))


def test_mutants_of_the_statement_land_outside_the_bound():
    """Each is a wrong kernel; C_CAP is the largest constant the GPU test may use, so a mutant beyond it is beyond every bound there."""
    ns12 = gbr.pick(CASES[1])
    assert worst(ns12, gbr.gradients(ns12, stat_pad=4), {"mean1", "var1"}) > 1.0, "statistics that count four padding columns per group"
    first = gbr.pick(CASES[0])
    assert worst(first, gbr.gradients(first, unbiased=True), {"var1", "var2", "var3"}) > 1.0, "unbiased variance"
    assert worst(first, gbr.gradients(first, stats_const=True), {"features", "w1", "gamma1"}) > 1.0, "statistics as constants in the backward"
    # nsample 64 over clusters of 32 points holds every point in two slots: every maximum is attained twice
    tied = gbr.pick(CASES[4])
    assert worst(tied, gbr.gradients(tied, ties="all"), {"features", "xyz", "w3"}) > 1.0, "the maximum's gradient to every tied slot"
    out, stats, grads = gbr.gradients(first)
    flipped = [-g if n == "new_xyz" else g for n, g in zip(first.names, grads)]
    assert worst(first, (out, stats, flipped), {"new_xyz"}) > 1.0, "grad_new_xyz with the wrong sign"
    assert worst(first, (out, stats, grads)) == 0.0


def test_declarations_bindings_shape_predicate_and_sizes():
    decl = header_functions()
    for name, nargs in (("mcp_group_mlp_bn_packed_floats", 4), ("mcp_group_mlp_bn_pack", 8), ("mcp_group_mlp_bn_workspace_bytes", 8),
                        ("mcp_group_mlp_bn_forward", 26), ("mcp_group_mlp_bn_backward", 32)):
        assert decl.get(name) == nargs, (name, decl.get(name))
        assert len(_lib.SIGNATURES[name]) == nargs
    assert _lib._RESTYPES["mcp_group_mlp_bn_workspace_bytes"] is ctypes.c_size_t
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    for k in CASES + FURTHER:
        c, ns, widths, xyz = k["c"], k["nsample"], k["widths"], int(k["use_xyz"])
        assert ops.group_mlp_bn_supported(c, widths, ns, k["use_xyz"])
        assert lib.mcp_group_mlp_bn_packed_floats(c, xyz, len(widths), w(*widths)) == ops.group_mlp_bn_packed_floats(c, widths, k["use_xyz"])
        pairs = k["b"] * k["m"] * ns
        fwd, bwd = (lib.mcp_group_mlp_bn_workspace_bytes(k["b"], k["m"], c, ns, xyz, len(widths), w(*widths), back) for back in (0, 1))
        assert fwd >= 4 * pairs * sum(widths)
        assert bwd >= fwd + 4 * pairs * (c + 3 * xyz + sum(widths[:-1]) + 2 * sum(widths) + c + 3 * xyz)
    for c, ns, widths, xyz in ((6, 8, [32], 1), (4, 8, [48], 1), (4, 65, [32], 1), (4, 0, [32], 1), (132, 8, [32], 1), (0, 8, [32], 0),
                               (4, 8, [256, 32], 1), (4, 8, [32, 32, 32, 32], 1)):
        assert not ops.group_mlp_bn_supported(c, widths, ns, bool(xyz)), (c, ns, widths, xyz)
        assert lib.mcp_group_mlp_bn_workspace_bytes(3, 7, c, ns, xyz, len(widths), w(*widths), 0) == 0, (c, ns, widths, xyz)
        assert lib.mcp_group_mlp_bn_workspace_bytes(3, 7, c, ns, xyz, len(widths), w(*widths), 1) == 0
        if 1 <= ns <= 64:
            assert lib.mcp_group_mlp_bn_packed_floats(c, xyz, len(widths), w(*widths)) == 0
    assert lib.mcp_group_mlp_bn_workspace_bytes(0, 7, 4, 8, 1, 1, w(32), 1) == 0
    assert ops.GROUP_MLP_BN_FUSED_CLASSES == {}, "the table ships empty"
    assert not ops.group_mlp_bn_routes_fused(4, [32, 32, 64], 16, 1 << 30), "a class without a measured row keeps the composition"


def test_arguments_are_validated_without_a_gpu():
    """Null pointers, empty dimensions, a bad pool, eps <= 0 and misaligned buffers are refused on the host (10001); an unsupported
    shape is refused before any pointer is looked at (10002).  Nothing here launches: every pointer is a host buffer."""
    lib = _lib.load()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ptrs = (ctypes.c_void_p * 2)(base, base)
    nulls = (ctypes.c_void_p * 2)(None, None)
    eps = (ctypes.c_float * 2)(1e-5, 1e-5)

    def fwd(b=1, n=8, m=4, c=8, ns=8, xyz=1, pool=0, layers=2, widths=w(32, 32), pts=base, new=base, feats=base, idx=base, packed=base, eps=eps, out=base,
            mean=ptrs, count=base, ws=base, ws_bytes=0):
        return lib.mcp_group_mlp_bn_forward(b, n, m, c, ns, xyz, pool, layers, widths, pts, new, feats, idx, None, packed, nulls, nulls, eps, out, mean, ptrs,
                                            ptrs, count, ws, ws_bytes, None)

    def bwd(b=1, n=8, m=4, c=8, ns=8, xyz=1, pool=0, layers=2, widths=w(32, 32), pts=base, feats=base, rstd=ptrs, g=base, order=None, gfeat=None, gxyz=None,
            gw=ptrs, ws=base, ws_bytes=0):
        return lib.mcp_group_mlp_bn_backward(b, n, m, c, ns, xyz, pool, layers, widths, pts, base, feats, base, None, base, nulls, nulls, ptrs, rstd, g, order,
                                             None, gfeat, gxyz, None, gw, nulls, nulls, nulls, ws, ws_bytes, None)

    assert fwd() == 10001 and bwd() == 10001, "a workspace of 0 bytes is too small"
    for kw in (dict(b=0), dict(n=0), dict(m=0), dict(pool=2), dict(feats=None), dict(pts=None), dict(new=None), dict(idx=None), dict(out=None),
               dict(count=None), dict(mean=nulls), dict(eps=(ctypes.c_float * 2)(1e-5, 0.0)), dict(feats=base + 4), dict(ws=None)):
        assert fwd(**kw) == 10001, kw
    for kw in (dict(b=0), dict(pool=-1), dict(feats=None), dict(pts=None), dict(g=None), dict(gw=nulls), dict(rstd=nulls), dict(gfeat=base), dict(gxyz=base),
               dict(g=base + 8)):
        assert bwd(**kw) == 10001, kw
    for kw in (dict(c=6), dict(widths=w(32, 48)), dict(layers=4), dict(ns=65), dict(ns=0), dict(c=0, xyz=0), dict(widths=w(256, 32))):
        assert fwd(**kw) == 10002 and bwd(**kw) == 10002, kw
