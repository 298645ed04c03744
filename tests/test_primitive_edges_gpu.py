"""-m gpu: the index, blend and normalisation primitives (csrc/pointnet2_ops.hip, interp3.hip, norm.hip) through their C entries, at the
kernels' own boundaries: 256 points per workgroup, 8 channels per blockIdx.y, 8 lanes per row in the narrow scatter and the weight
gradient, 1024 known points per LDS tile of three_nn, the four registers-per-lane forms of add_layernorm, both alignment routes of
every float4 kernel and a second grid-stride round of every capped loop.  kernel_variants.PRIMITIVE_CASES are the shapes;
test_primitive_variants_cpu.py checks that they name every kernel the three units emit and reach every edge class.  The ball-query
kernels stay with test_ball_query_lengths_gpu.py, the search inside mcp_interp3 with the KNN tests.

Every output is a view inside a larger buffer of NaN (floats) or GUARD_INT (indices) with guard rows before and after it, which must
be untouched after every call; an output the kernel overwrites starts as the sentinel, one it adds into as a known base.  An operand
"off 16 bytes" is a contiguous view 4 bytes past a 16-byte boundary of its storage.

The gathers, scatters and blends only move, add and multiply by a blend weight, so their data makes every comparison exact: features
and gradients are integers in [-8, 8], blend weights permutations of (1/2, 1/4, 1/4), the leaky slope 0.5.  Every fp32 product and
partial sum is then exact in any order (the longest segments hold a few thousand addends), and every result -- the atomic ones too --
must EQUAL a float64 index_put_(accumulate=True) / plain-indexing reference computed on the CPU.  Index lists put a third of the
positions on three hot rows, leave rows nobody gathers (exact zeros from the sorted kernels, the untouched base from the atomic ones)
and hit rows 0 and n - 1.  (order, seg) come from torch.sort(stable=True) + searchsorted, so mcp_scatter_segments can neither mask nor
mimic a fault here; one case per sorted entry takes the pair from ops._scatter_segments and must give the same bits.  One case per
channel-major forward / sorted entry runs on real-valued data against the project's C oracle, three_nn and interp3 always do.
add_layernorm rounds: real data against float64 at the project's tolerance for it (rtol 2e-5, atol 2e-6).

Not run, on purpose: a second grid-stride round of mfa_prepare_kernel (more than 65536 x 256 float4 items in each of three outputs:
over 800 MB), and the 64-bit division of mcp_div when mcp_fits32 is false (more than 2^32 items)."""
import math

import pytest
import torch

from mocopci_amd import _lib, ops
from oracle import pointset as orc
from tests import kernel_variants as kv
from tests.test_ops_gpu import cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD_INT = -77777777
SLOPE = 0.5


def cases(entry, ok=True):
    return pytest.mark.parametrize("c", kv.primitive_cases(entry, ok=ok), ids=kv.primitive_case_id)


def cases_of(*entries):
    return pytest.mark.parametrize("c", [c for e in entries for c in kv.primitive_cases(e, ok=True)], ids=kv.primitive_case_id)


def run(name, *args):
    """The C entry on the current stream -> its return code, after the device has finished."""
    with torch.cuda.device(DEV):
        rc = getattr(_lib.load(), name)(*args, _lib.stream())
    torch.cuda.synchronize()
    return rc


class Guarded:
    """A contiguous view `t` of `shape` inside a 1-D buffer of sentinels: at least two rows of guard before and after it.  fill: what
    the view starts with (the sentinel by default, or a CPU tensor: the base of an accumulating output); off: the view starts
    4 * off bytes past a 16-byte boundary."""

    def __init__(self, shape, fill=None, dtype=torch.float32, off=0):
        self.sentinel = NAN if dtype == torch.float32 else GUARD_INT
        n, guard = math.prod(shape), 64 + 2 * ((shape[-1] + 3) & ~3)
        self.buf = torch.full((2 * guard + n + 4,), self.sentinel, dtype=dtype, device=DEV)
        self.lo, self.hi = guard + off, guard + off + n
        self.t = self.buf[self.lo:self.hi].view(shape)
        if fill is not None:
            self.t.copy_(fill)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 4 * off

    def untouched(self, t):
        return bool(torch.isnan(t).all()) if self.sentinel != self.sentinel else bool((t == self.sentinel).all())

    def check(self, what="output"):
        assert self.untouched(self.buf[:self.lo]), f"{what}: the guard rows before it were written"
        assert self.untouched(self.buf[self.hi:]), f"{what}: the guard rows after it were written"

    def refill(self):
        self.t.fill_(self.sentinel)


def dev(t, off=0):
    """The CPU tensor on the device, contiguous; off: 4 * off bytes past a 16-byte boundary of its storage."""
    if not off:
        out = t.contiguous().to(DEV)
        assert out.data_ptr() % 16 == 0
        return out
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    out = flat[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4 * off
    return out


def off_of(c, name):
    return 1 if name in c["off"] else 0


def gen_of(c):
    return torch.Generator().manual_seed(sum(ord(ch) for ch in kv.primitive_case_id(c)))


def ints(gen, *shape):
    return torch.randint(-8, 9, shape, generator=gen).float()


def index_list(gen, B, T, n):
    """(B,T) int32: uniform over the n rows, then a third of the positions moved to three hot rows, rows 3 and n - 3 left to nobody
    (n >= 8), the first position on row 0 and the last on row n - 1."""
    idx = torch.randint(0, n, (B, T), generator=gen)
    if n >= 8:
        hot = torch.tensor([1, n // 2, n - 2])
        mask = torch.rand(B, T, generator=gen) < 1 / 3
        idx[mask] = hot[torch.randint(0, 3, (int(mask.sum()),), generator=gen)]
        idx[idx == 3] = 4
        idx[idx == n - 3] = n - 4
    idx[:, 0] = 0
    idx[:, -1] = n - 1
    return idx.int()


def segment_list(gen, B, T, n):
    """(B,T) int32 whose destinations have 0, 1, 7, 8, 9, 17 and 2000 positions (the narrow kernel's 8 lanes -1 / 0 / +1, two passes
    plus one, a long chain), on other rows in every batch element; rows 0 and n - 1 are among the hit ones."""
    lengths = (2000, 1, 7, 8, 9, 17, 0, 0)
    assert T >= sum(lengths) + 2 and n >= len(lengths) + 4
    out = torch.empty(B, T, dtype=torch.int64)
    for b in range(B):
        rows = torch.randperm(n - 2, generator=gen) + 1                      # rows 1 .. n - 2 in random order
        special, rest = rows[:len(lengths)], torch.cat((rows[len(lengths):], torch.tensor([0, n - 1])))
        filler = rest[torch.randint(0, len(rest), (T - sum(lengths) - 2,), generator=gen)]
        flat = torch.cat([torch.full((k,), int(r)) for r, k in zip(special, lengths)] + [filler, torch.tensor([0, n - 1])])
        out[b] = flat[torch.randperm(T, generator=gen)]
        counts = torch.bincount(out[b], minlength=n)
        assert sorted(counts[special].tolist()) == sorted(lengths)
    return out.int()


def blend_weights(gen, B, n):
    perms = torch.tensor([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]])
    return perms[torch.randint(0, 3, (B, n), generator=gen)]


def segments(idx, n):
    """(order, seg) int32 of a (B,T) list into rows 0 .. n - 1: the stable sort by destination and its CSR offsets."""
    keys, order = torch.sort(idx.long(), dim=1, stable=True)
    seg = torch.searchsorted(keys.contiguous(), torch.arange(n + 1).expand(idx.shape[0], n + 1).contiguous())
    return order.int(), seg.int()


def segment_pairs(c, idx, n):
    """The (order, seg) pairs a sorted case runs with, on the device: the torch one, and for segments="ops" the library's as well."""
    pairs = [tuple(t.to(DEV) for t in segments(idx, n))]
    if c.get("segments") == "ops":
        pairs.append(ops._scatter_segments(idx.to(DEV), n))
        assert all(t.dtype == torch.int32 and t.is_contiguous() for t in pairs[1])
    return pairs


def scatter_rows(go, idx, n, w=None):
    """float64 (B,n,C): sum over the positions t with idx[b,t] = row of (w[b,t] *) go[b,t,:]."""
    B, T, C = go.shape
    out = torch.zeros(B, n, C, dtype=torch.float64)
    src = go.double() if w is None else go.double() * w.double().unsqueeze(-1)
    out.index_put_((torch.arange(B).view(B, 1).expand(B, T), idx.long()), src, accumulate=True)
    return out


def blend_rows(feat, idx3, w3):
    """float64 (B,n,C) = sum_j w3[b,p,j] feat[b, idx3[b,p,j], :]."""
    bi = torch.arange(feat.shape[0]).view(-1, 1)
    f = feat.double()
    return sum(w3[..., j].double().unsqueeze(-1) * f[bi, idx3[..., j].long()] for j in range(3))


def same(got, want64, what):
    """got (device, fp32) equals the float64 reference cast to fp32, bit for bit."""
    want = want64.float()
    assert torch.equal(want.double(), want64), f"{what}: the reference is not exact in fp32"
    assert torch.equal(got, want.to(DEV)), f"{what}: {int((got != want.to(DEV)).sum())} of {want.numel()} values differ"


# ---- the channel-major entries of the reference API ------------------------------------------------------------------------------------
def cm_operands(c, gen):
    """(rows on the points side, count on the thread axis, idx int32 in the shape the entry takes, blend weights or None)."""
    e, s = c["entry"], c["shape"]
    B = s["b"]
    if "three_interpolate" in e:
        src, n = s["m"], s["n"]
        if e.endswith("grad_sorted") or c.get("data") != "real":
            idx = index_list(gen, B, 3 * n, src).view(B, n, 3)
        else:
            idx = torch.randint(0, src, (B, n, 3), generator=gen, dtype=torch.int32)
        w = torch.rand(B, n, 3, generator=gen) if c.get("data") == "real" else blend_weights(gen, B, n)
        return src, n, idx, w
    src = s["n"]
    if e.endswith("grad_sorted"):
        return src, s["t"], index_list(gen, B, s["t"], src), None
    shape = (s["npoints"],) if "gather" in e else (s["npoints"], s["nsample"])
    T = math.prod(shape)
    return src, T, index_list(gen, B, T, src).view(B, *shape), None


@cases_of("mcp_gather_points", "mcp_group_points", "mcp_three_interpolate")
def test_channel_major_gathers_and_blend(c):
    gen, s, e = gen_of(c), c["shape"], c["entry"]
    B, C = s["b"], s["c"]
    real = c.get("data") == "real"
    src, T, idx, w = cm_operands(c, gen)
    points = torch.randn(B, C, src, generator=gen) if real else ints(gen, B, C, src)
    out = Guarded((B, C) + tuple(idx.shape[1:]) if w is None else (B, C, T))
    pd, idd, wd = dev(points), dev(idx), None if w is None else dev(w)
    if e == "mcp_gather_points":
        rc = run(e, B, C, src, s["npoints"], _lib.fptr(pd), _lib.iptr(idd), _lib.fptr(out.t))
        oracle = orc.gather_operation
    elif e == "mcp_group_points":
        rc = run(e, B, C, src, s["npoints"], s["nsample"], _lib.fptr(pd), _lib.iptr(idd), _lib.fptr(out.t))
        oracle = orc.grouping_operation
    else:
        rc = run(e, B, C, src, T, _lib.fptr(pd), _lib.iptr(idd), _lib.fptr(wd), _lib.fptr(out.t))
        oracle = None
    _lib.check(rc)
    out.check()
    if real:
        want = oracle(points, idx) if oracle else orc.three_interpolate(points, idx, w)
        assert torch.equal(out.t.cpu(), want), "differs from the C oracle"
        return
    bi = torch.arange(B).view(B, 1, 1)
    flat = idx.reshape(B, -1).long()
    if w is None:
        want = points.double()[bi, torch.arange(C).view(1, C, 1), flat.view(B, 1, -1)].view(out.t.shape)
    else:
        want = blend_rows(points.transpose(1, 2), idx, w).transpose(1, 2).contiguous()
    same(out.t, want, e)


@cases_of("mcp_gather_points_grad", "mcp_group_points_grad", "mcp_three_interpolate_grad")
def test_channel_major_atomic_scatters_add_into_the_callers_buffer(c):
    gen, s, e = gen_of(c), c["shape"], c["entry"]
    B, C = s["b"], s["c"]
    src, T, idx, w = cm_operands(c, gen)
    go = ints(gen, B, C, T)
    base = ints(gen, B, C, src)
    out = Guarded((B, C, src), fill=base)
    god, idd, wd = dev(go), dev(idx), None if w is None else dev(w)
    if e == "mcp_gather_points_grad":
        rc = run(e, B, C, src, s["npoints"], _lib.fptr(god), _lib.iptr(idd), _lib.fptr(out.t))
    elif e == "mcp_group_points_grad":
        rc = run(e, B, C, src, s["npoints"], s["nsample"], _lib.fptr(god), _lib.iptr(idd), _lib.fptr(out.t))
    else:
        rc = run(e, B, C, T, src, _lib.fptr(god), _lib.iptr(idd), _lib.fptr(wd), _lib.fptr(out.t))
    _lib.check(rc)
    out.check()
    if w is None:
        scat = scatter_rows(go.transpose(1, 2), idx.reshape(B, -1), src)
    else:
        scat = scatter_rows(go.transpose(1, 2).repeat_interleave(3, dim=1), idx.reshape(B, -1), src, w.reshape(B, -1))
    same(out.t, base.double() + scat.transpose(1, 2), e)


@cases_of("mcp_group_points_grad_sorted", "mcp_three_interpolate_grad_sorted")
def test_channel_major_sorted_scatters(c):
    gen, s, e = gen_of(c), c["shape"], c["entry"]
    B, C = s["b"], s["c"]
    real = c.get("data") == "real"
    src, T, idx, w = cm_operands(c, gen)
    go = torch.randn(B, C, T, generator=gen) if real else ints(gen, B, C, T)
    flat = idx.reshape(B, -1)
    counts = torch.stack([torch.bincount(flat[b].long(), minlength=src) for b in range(B)])
    if src >= 8:
        assert bool((counts == 0).any()) and int(counts.max()) > flat.shape[1] // 12, "the list has no empty or no hot row"
    assert bool((flat[:, 0] == 0).all()) and bool((flat[:, -1] == src - 1).all())
    if real:
        want = orc.grouping_operation_grad(go.unsqueeze(-1), flat.unsqueeze(-1), src) if w is None else orc.three_interpolate_grad(go, idx, w, src)
    elif w is None:
        want = scatter_rows(go.transpose(1, 2), flat, src).transpose(1, 2)
    else:
        want = scatter_rows(go.transpose(1, 2).repeat_interleave(3, dim=1), flat, src, w.reshape(B, -1)).transpose(1, 2)
    out = Guarded((B, C, src))
    god, wd = dev(go), None if w is None else dev(w)
    for order, seg in segment_pairs(c, flat, src):
        out.refill()
        if w is None:
            rc = run(e, B, C, src, T, _lib.fptr(god), _lib.iptr(order), _lib.iptr(seg), _lib.fptr(out.t))
        else:
            rc = run(e, B, C, T, src, _lib.fptr(god), _lib.iptr(order), _lib.iptr(seg), _lib.fptr(wd), _lib.fptr(out.t))
        _lib.check(rc)
        out.check()
        if real:
            assert torch.equal(out.t.cpu(), want), "differs from the C oracle's sequential loop"
        else:
            same(out.t, want, e)
        assert bool((out.t.cpu().transpose(1, 2)[counts == 0] == 0).all()), "a row nobody gathers is not zero"


# ---- the channel-last row gather and the three-neighbour blend ---------------------------------------------------------------------------
def run_twice(c, out, call, compare):
    """call() -> rc into `out`; compare(); guards; for a twice=True case once more into a refilled output."""
    for _ in range(2 if c.get("twice") else 1):
        out.refill()
        _lib.check(call())
        out.check()
        compare()


@cases("mcp_group_rows")
def test_group_rows(c):
    gen, s = gen_of(c), c["shape"]
    B, n, C, T = s["b"], s["n"], s["c"], s["t"]
    points, idx = ints(gen, B, n, C), index_list(gen, B, T, n)
    pd, idd = dev(points, off_of(c, "points")), dev(idx)
    out = Guarded((B, T, C), off=off_of(c, "out"))
    want = points.double()[torch.arange(B).view(B, 1), idx.long()]
    run_twice(c, out, lambda: run("mcp_group_rows", B, n, C, T, _lib.fptr(pd), _lib.iptr(idd), _lib.fptr(out.t)), lambda: same(out.t, want, "group_rows"))


@cases("mcp_interp3_apply")
def test_interp3_apply(c):
    gen, s = gen_of(c), c["shape"]
    B, n, S, C = s["b"], s["n"], s["s"], s["c"]
    feat, idx3, w3 = ints(gen, B, S, C), index_list(gen, B, 3 * n, S).view(B, n, 3), blend_weights(gen, B, n)
    fd, idd, wd = dev(feat, off_of(c, "feat")), dev(idx3), dev(w3)
    out = Guarded((B, n, C), off=off_of(c, "out"))
    want = blend_rows(feat, idx3, w3)
    run_twice(c, out, lambda: run("mcp_interp3_apply", B, n, S, C, _lib.fptr(fd), _lib.iptr(idd), _lib.fptr(wd), _lib.fptr(out.t)),
              lambda: same(out.t, want, "interp3_apply"))


@cases("mcp_group_rows_add_leaky")
def test_group_rows_add_leaky(c):
    gen, s = gen_of(c), c["shape"]
    B, n, C, S, K = s["b"], s["n"], s["c"], s["s"], s["k"]
    points, centre, idx = ints(gen, B, n, C), ints(gen, B, S, C), index_list(gen, B, S * K, n).view(B, S, K)
    pd, cd, idd = dev(points), dev(centre), dev(idx)
    out = Guarded((B, S, K, C))
    z = points.double()[torch.arange(B).view(B, 1, 1), idx.long()] + centre.double().unsqueeze(2)
    assert bool((z < 0).any()) and bool((z == 0).any()) and bool((z > 0).any())
    want = torch.where(z > 0, z, z * SLOPE)
    run_twice(c, out, lambda: run("mcp_group_rows_add_leaky", B, n, C, S, K, SLOPE, _lib.fptr(pd), _lib.iptr(idd), _lib.fptr(cd), _lib.fptr(out.t)),
              lambda: same(out.t, want, "group_rows_add_leaky"))


@cases("mcp_group_rows_add_leaky", ok=False)
def test_group_rows_add_leaky_refuses_what_it_cannot_read_as_float4(c):
    gen, s = gen_of(c), c["shape"]
    B, n, C, S, K = s["b"], s["n"], s["c"], s["s"], s["k"]
    pd, cd = dev(ints(gen, B, n, C), off_of(c, "points")), dev(ints(gen, B, S, C), off_of(c, "centre"))
    idd = dev(index_list(gen, B, S * K, n))
    out = Guarded((B, S, K, C), off=off_of(c, "out"))
    rc = run("mcp_group_rows_add_leaky", B, n, C, S, K, SLOPE, _lib.fptr(pd), _lib.iptr(idd), _lib.fptr(cd), _lib.fptr(out.t))
    assert rc == kv.MCP_ERR_BAD_ARG == c["status"]
    assert out.untouched(out.buf), "a refused call wrote to its output"


# ---- the sorted (deterministic) channel-last scatters --------------------------------------------------------------------------------------
@cases("mcp_group_rows_grad_sorted")
def test_group_rows_grad_sorted(c):
    gen, s = gen_of(c), c["shape"]
    B, n, C, T = s["b"], s["n"], s["c"], s["t"]
    idx = segment_list(gen, B, T, n) if n < 1000 else index_list(gen, B, T, n)
    go = ints(gen, B, T, C)
    counts = torch.stack([torch.bincount(idx[b].long(), minlength=n) for b in range(B)])
    assert bool((counts == 0).any()) and bool((counts[:, 0] > 0).all()) and bool((counts[:, -1] > 0).all())
    want = scatter_rows(go, idx, n).float().to(DEV)
    god = dev(go, off_of(c, "grad_out"))
    out = Guarded((B, n, C), off=off_of(c, "grad_points"))
    empty = (counts == 0).to(DEV)
    for order, seg in segment_pairs(c, idx, n):
        def compare():
            assert torch.equal(out.t, want), f"{int((out.t != want).sum())} of {want.numel()} values differ from the float64 scatter"
            assert bool((out.t[empty] == 0).all()), "a row nobody gathers is not zero"
        run_twice(c, out, lambda: run("mcp_group_rows_grad_sorted", B, n, C, T, _lib.fptr(god), _lib.iptr(order), _lib.iptr(seg), _lib.fptr(out.t)), compare)


@cases("mcp_interp3_apply_grad_sorted")
def test_interp3_apply_grad_sorted(c):
    gen, s = gen_of(c), c["shape"]
    B, n, S, C = s["b"], s["n"], s["s"], s["c"]
    wanted = s.get("want", ("feat", "w"))
    feat, go = ints(gen, B, S, C), ints(gen, B, n, C)
    idx3, w3 = index_list(gen, B, 3 * n, S).view(B, n, 3), blend_weights(gen, B, n)
    flat = idx3.reshape(B, 3 * n)
    bi = torch.arange(B).view(B, 1, 1)
    want_w = None
    if "w" in wanted:      # <grad_out[b,p,:], feat[b, idx3[b,p,j], :]>: integers below 2^24
        want_w = torch.stack([(go.double() * feat.double()[bi[:, :, 0], idx3[..., j].long()]).sum(-1) for j in range(3)], dim=-1).float().to(DEV)
    want_f = scatter_rows(go.repeat_interleave(3, dim=1), flat, S, w3.reshape(B, 3 * n)).float().to(DEV) if "feat" in wanted else None
    fd, god, idd, wd = dev(feat, off_of(c, "feat")), dev(go, off_of(c, "grad_out")), dev(idx3), dev(w3)
    gf = Guarded((B, S, C), off=off_of(c, "grad_feat"))
    gw = Guarded((B, n, 3))

    def call(order, seg, feat_out, w_out):
        gf.refill()
        gw.refill()
        _lib.check(run("mcp_interp3_apply_grad_sorted", B, n, S, C, _lib.fptr(fd), _lib.iptr(idd), _lib.fptr(wd), _lib.fptr(god), _lib.iptr(order), _lib.iptr(seg),
                       _lib.fptr(gf.t) if feat_out else None, _lib.fptr(gw.t) if w_out else None))
        gf.check("grad_feat")
        gw.check("grad_w3")
        if feat_out:
            assert torch.equal(gf.t, want_f), f"grad_feat: {int((gf.t != want_f).sum())} of {want_f.numel()} values differ from the float64 scatter"
        else:
            assert gf.untouched(gf.t), "grad_feat was written without being asked for"
        if w_out:
            assert torch.equal(gw.t, want_w), f"grad_w3: {int((gw.t != want_w).sum())} of {want_w.numel()} values differ from the float64 products"
        else:
            assert gw.untouched(gw.t), "grad_w3 was written without being asked for"
    for order, seg in segment_pairs(c, flat, S):
        for _ in range(2 if c.get("twice") else 1):
            call(order, seg, "feat" in wanted, "w" in wanted)
        if len(wanted) == 2 and not c.get("twice"):     # either gradient alone: the joint call's bits (both equal the one reference)
            call(order, seg, True, False)
            call(order, seg, False, True)


@cases_of("mcp_group_rows_grad", "mcp_interp3_apply_grad")
def test_channel_last_atomic_scatters_add_into_the_callers_buffer(c):
    gen, s, e = gen_of(c), c["shape"], c["entry"]
    B, C = s["b"], s["c"]
    if e == "mcp_group_rows_grad":
        n, T = s["n"], s["t"]
        idx, go, base = index_list(gen, B, T, n), ints(gen, B, T, C), ints(gen, B, n, C)
        out = Guarded((B, n, C), fill=base)
        god, idd = dev(go), dev(idx)
        rc = run(e, B, n, C, T, _lib.fptr(god), _lib.iptr(idd), _lib.fptr(out.t))
        scat = scatter_rows(go, idx, n)
    else:
        n, S = s["n"], s["s"]
        idx3, w3, go, base = index_list(gen, B, 3 * n, S).view(B, n, 3), blend_weights(gen, B, n), ints(gen, B, n, C), ints(gen, B, S, C)
        out = Guarded((B, S, C), fill=base)
        god, idd, wd = dev(go), dev(idx3), dev(w3)
        rc = run(e, B, n, S, C, _lib.fptr(god), _lib.iptr(idd), _lib.fptr(wd), _lib.fptr(out.t))
        scat = scatter_rows(go.repeat_interleave(3, dim=1), idx3.reshape(B, 3 * n), S, w3.reshape(B, 3 * n))
    _lib.check(rc)
    out.check()
    assert bool((scat.abs().sum(-1) == 0).any()), "every row is gathered: none shows the untouched base"
    same(out.t, base.double() + scat, e)


# ---- the exhaustive three_nn kernel, the interpolation weights, the fused interp3 -----------------------------------------------------------
@cases("mcp_three_nn")
def test_three_nn_at_the_tile_and_block_boundaries(c):
    s = c["shape"]
    B, n, m = s["b"], s["n"], s["m"]
    unknown, known = cloud(31 + n, B, n), cloud(32 + m, B, m)
    if c.get("grid"):
        unknown, known = (unknown * 2).round() / 2, (known * 2).round() / 2
    wd, wi = orc.three_nn(unknown, known)
    d2, i3 = Guarded((B, n, 3)), Guarded((B, n, 3), dtype=torch.int32)
    ud, kd = dev(unknown), dev(known)
    _lib.check(run("mcp_three_nn", B, n, m, _lib.fptr(ud), _lib.fptr(kd), _lib.fptr(d2.t), _lib.iptr(i3.t)))
    d2.check("dist2")
    i3.check("idx")
    assert torch.equal(i3.t.cpu(), wi)
    assert torch.equal(torch.sqrt(d2.t.cpu()), wd)
    if m < 3:
        assert bool(torch.isinf(d2.t[..., m:]).all()) and bool(torch.isfinite(d2.t[..., :m]).all())
    if c.get("grid"):       # ties that straddle the tile boundary: a known point of the second tile as far as one of the first
        tile = kv.PRIM_NN_TILE
        first, second = (((unknown[:, :, None] - known[:, None, lo:lo + tile]) ** 2).sum(-1).min(-1).values for lo in (0, tile))
        assert bool((first == second).any())


def interp3_clouds(c):
    s = c["shape"]
    dense, sparse = cloud(51 + s["n"], s["b"], s["n"]), cloud(52 + s["s"], s["b"], s["s"])
    k = c.get("coincident", 0)
    if k:
        dense[:, :k] = sparse[:, :k]
        dense[:, -1] = sparse[:, k]
    return dense, sparse


@cases("mcp_interp3")
def test_interp3_fused_call(c):
    s = c["shape"]
    B, n, S, C = s["b"], s["n"], s["s"], s["c"]
    dense, sparse = interp3_clouds(c)
    feat = torch.randn(B, S, C, generator=gen_of(c))
    out, i3, w3 = Guarded((B, n, C)), Guarded((B, n, 3), dtype=torch.int32), Guarded((B, n, 3))
    dd, sd, fd = dev(dense), dev(sparse), dev(feat)
    _lib.check(run("mcp_interp3", B, n, S, C, _lib.fptr(dd), _lib.fptr(sd), _lib.fptr(fd), _lib.fptr(out.t), _lib.iptr(i3.t), _lib.fptr(w3.t)))
    for g, what in ((out, "out"), (i3, "idx3"), (w3, "w3")):
        g.check(what)
    assert torch.equal(out.t.cpu(), orc.interp3(dense, sparse, feat))


@cases("mcp_interp3_weights")
def test_interp3_weights(c):
    """The oracle's weights, read off its blend of one-hot features: with three distinct neighbours out[b, p, idx3[b,p,j]] = w_j exactly."""
    s = c["shape"]
    B, n, S = s["b"], s["n"], s["s"]
    dense, sparse = interp3_clouds(c)
    idx3 = orc.knn(dense, sparse, 3)
    assert bool((idx3[..., 0] != idx3[..., 1]).all()) and bool((idx3[..., 1] != idx3[..., 2]).all()) and bool((idx3[..., 0] != idx3[..., 2]).all())
    want = orc.interp3(dense, sparse, torch.eye(S).expand(B, S, S).contiguous(), idx3).gather(2, idx3.long())
    w3 = Guarded((B, n, 3))
    dd, sd, idd = dev(dense), dev(sparse), dev(idx3.int())
    _lib.check(run("mcp_interp3_weights", B, n, S, _lib.fptr(dd), _lib.fptr(sd), _lib.iptr(idd), _lib.fptr(w3.t)))
    w3.check("w3")
    assert torch.equal(w3.t.cpu(), want)
    if c.get("coincident"):
        k = c["coincident"]
        assert bool(((sparse[torch.arange(B).view(B, 1), idx3[:, :k, 0].long()] - dense[:, :k]).norm(dim=-1) == 0).all())   # really coincident


# ---- add_layernorm -----------------------------------------------------------------------------------------------------------------------
def layernorm_ref(x, y, bias, gamma, beta, eps):
    z = x.double() + (0 if y is None else y.double()) + (0 if bias is None else bias.double())
    out = torch.nn.functional.layer_norm(z, (z.shape[-1],), None, None, eps)
    if gamma is not None:
        out = out * gamma.double() + (0 if beta is None else beta.double())
    return out


def column_slice(t, width, first):
    """t (rows, c) as columns first : first + c of a (rows, width) device tensor whose other columns hold NaN."""
    wide = torch.full((t.shape[0], width), NAN, device=DEV)
    wide[:, first:first + t.shape[1]] = t.to(DEV)
    return wide[:, first:first + t.shape[1]]


@cases("mcp_add_layernorm")
def test_add_layernorm_at_the_register_and_wave_boundaries(c):
    s, gen = c["shape"], gen_of(c)
    rows, C = s["rows"], s["c"]
    x, y = torch.randn(rows, C, generator=gen) * 3 + 1, torch.randn(rows, C, generator=gen)
    bias, gamma, beta = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    eps = 1e-6
    bd, gd, btd = dev(bias), dev(gamma), dev(beta)
    # (x slice, y slice, bias, gamma, beta, out_stride): everything at once on strided operands 4 bytes off; the bare call; the halves
    forms = (("all", True, True, True, True, True, C + 5), ("bare", False, False, False, False, False, C),
             ("y+gamma", False, True, False, True, False, C + 1), ("bias", True, False, True, False, False, C))
    for name, sliced, use_y, use_bias, use_gamma, use_beta, os_ in forms:
        xd = column_slice(x, C + 7, 1) if sliced else dev(x)
        yd = (column_slice(y, C + 6, 5) if sliced else dev(y)) if use_y else None
        if sliced:
            assert xd.data_ptr() % 16 == 4 and xd.stride(0) > C
        out = Guarded((rows, os_))
        rc = run("mcp_add_layernorm", rows, C, xd.data_ptr(), xd.stride(0), None if yd is None else yd.data_ptr(), 0 if yd is None else yd.stride(0),
                 _lib.fptr(bd) if use_bias else None, _lib.fptr(gd) if use_gamma else None, _lib.fptr(btd) if use_gamma and use_beta else None, eps,
                 _lib.fptr(out.t), os_)
        _lib.check(rc)
        out.check(name)
        assert out.untouched(out.t[:, C:]), f"{name}: the columns between the rows of a strided output were written"
        got = out.t[:, :C].cpu()
        want = layernorm_ref(x, y if use_y else None, bias if use_bias else None, gamma if use_gamma else None, beta if use_gamma and use_beta else None, eps)
        if C == 1:      # z - mean(z) is exactly zero
            assert torch.equal(got, (beta if use_gamma and use_beta else torch.zeros(1)).expand(rows, 1)), name
        torch.testing.assert_close(got.double(), want, rtol=2e-5, atol=2e-6, msg=lambda m: f"{name}: {m}")


@cases("mcp_add_layernorm", ok=False)
def test_add_layernorm_refusals(c):
    s = c["shape"]
    rows, C = s["rows"], s["c"]
    x = dev(torch.randn(rows, C, generator=gen_of(c)))
    out = Guarded((rows, C))
    rc = run("mcp_add_layernorm", rows, C, _lib.fptr(x), s.get("x_stride", C), None, 0, None, None, None, 1e-6, _lib.fptr(out.t), s.get("out_stride", C))
    assert rc == c["status"] and rc in (kv.MCP_ERR_UNSUPPORTED, kv.MCP_ERR_BAD_ARG)
    assert out.untouched(out.buf), "a refused call wrote to its output"


# ---- mfa_prepare ---------------------------------------------------------------------------------------------------------------------------
def mfa_operands(c):
    s, gen = c["shape"], gen_of(c)
    R, N, C, M = s["rows"], s["n"], s["c"], 7
    fea, ts, tp = ints(gen, M, N, C), ints(gen, R, C), ints(gen, R, C)
    ss = torch.randint(0, M, (R,), generator=gen, dtype=torch.int32)
    sp = ((ss + 1 + torch.randint(0, M - 1, (R,), generator=gen, dtype=torch.int32)) % M).int()
    assert bool((sp != ss).all())
    return fea, ss, sp, ts, tp, torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)


def mfa_call(c, operands):
    s = c["shape"]
    R, N, C = s["rows"], s["n"], s["c"]
    fea, ss, sp, ts, tp, sc, sh = operands
    d = {name: dev(t, off_of(c, name)) for name, t in (("fea", fea), ("te_self", ts), ("te_partner", tp), ("scale", sc), ("shift", sh))}
    outs = [Guarded((R, N, C), off=off_of(c, name)) for name in ("x", "xn", "xr")]
    ssd, spd = dev(ss), dev(sp)
    rc = run("mcp_mfa_prepare", R, N, C, _lib.fptr(d["fea"]), _lib.iptr(ssd), _lib.iptr(spd), _lib.fptr(d["te_self"]), _lib.fptr(d["te_partner"]),
             _lib.fptr(d["scale"]), _lib.fptr(d["shift"]), *(_lib.fptr(o.t) for o in outs))
    return rc, outs


@cases("mcp_mfa_prepare")
def test_mfa_prepare(c):
    from oracle.backend import OracleBackend
    operands = mfa_operands(c)
    rc, outs = mfa_call(c, operands)
    _lib.check(rc)
    for o, what in zip(outs, ("x", "xn", "xr")):
        o.check(what)
    fea, ss, sp, ts, tp, sc, sh = operands
    same(outs[0].t, fea.double()[ss.long()] + ts.double()[:, None, :], "x")
    want = OracleBackend().mfa_prepare(*operands)
    assert torch.equal(outs[0].t.cpu(), want[0])
    for got, ref in zip(outs[1:], want[1:]):
        torch.testing.assert_close(got.t.cpu(), ref, rtol=1e-6, atol=1e-6)
    assert not torch.equal(outs[1].t, outs[2].t)      # the partner rows are other rows


@cases("mcp_mfa_prepare", ok=False)
def test_mfa_prepare_refusals(c):
    rc, outs = mfa_call(c, mfa_operands(c))
    assert rc == c["status"] and rc == (kv.MCP_ERR_BAD_ARG if c["off"] else kv.MCP_ERR_UNSUPPORTED)
    for o in outs:
        assert o.untouched(o.buf), "a refused call wrote to an output"
