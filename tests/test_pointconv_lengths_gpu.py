"""-m gpu: PointConv with per-element centre lengths (csrc/pointconv_lengths.hip; mcp_pointconv_agg_lengths /
mcp_pointconv_linear_lengths / mcp_pointconv_agg_grad_lengths, ops.HipBackend.pointconv_agg / pointconv_linear(centre_lengths=)).

Every case has 96 source points, 32 neighbours and a random list.  The batch under test holds NaN in every padded row of every
per-centre float input (new_xyz, the upstream gradient) and out-of-range indices (-1 and 2^30, alternating) in the padded rows of
the list; the yardstick is the DENSE call on the same batch with finite padding (the list row of padded centre i holds i mod 96 --
what the length form's scatter puts there, grad.spread_padded_rows --, zero upstream gradient on padded centres).  The dense kernels
are held to float64 by test_fused_variants_gpu.py and test_fused_grad_variants_gpu.py, so no kernel case needs a tolerance:
  * live rows are torch.equal to the dense call's, padded rows are exact zeros (the fused Linear's too: its bias is not zero);
  * the six WeightNet weight gradients and the gradients of s_xyz / s_points are torch.equal to the dense call's;
  * full lengths, and qlen = NULL at the C entry points, give the dense call's bits;
  * a second call gives equal bits.
The forward cases reach every form of the dispatch (tests/kernel_variants.py): pointconv_agg_kernel<256, 32 | 16 | 8> at B = 2,
s = 8211 (total = 16422 > 16384; 8211 = 256 * 32 + 19 is no multiple of any form's points per workgroup, so a workgroup straddles the
two elements), pointconv_agg_lowlevel_kernel<256> (d = 32; d = 5: d % 4) and <1024> (d = 256, total <= 8192), and both fused Linears.
Backward: d = 4, 32, 64, 256 at B = 3, s = 77 -- odd, so a wave's two centres straddle elements and the live / padded edge.
Lengths per case: (0, s, ...), (1, s - 1, ...), and one on, one below and one above a multiple of the form's points per workgroup.
Two more routes: elements shorter than a workgroup's range (s = 5), and the backward at d = 5 through the masked torch formulation."""
import pytest
import torch

from mocopci_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_SRC, K = 96, 32
BIG = 1 << 30


def length_sets(b, s, ppb):
    """The length sets of a case: b elements of s centres, a form with ppb points per workgroup (module docstring)."""
    m = max(ppb, (s // 2) // ppb * ppb)          # a multiple of ppb inside the element
    sets = [[0, s, s // 3], [1, s - 1, s], [m, m - 1, m + 1], [m + 1, m, m - 1]]   # (the last: `above` for a batch of two)
    return [tuple(v[:b]) for v in sets]


class Batch:
    """One random batch on the device: `clean` (finite padding, list row i mod 96 on padded centre i) and `dirty` (NaN / out-of-range)."""

    def __init__(self, b, s, d, lens, seed, c_out=None):
        g = torch.Generator().manual_seed(seed)
        r = lambda *shape, scale=1.0: (torch.rand(*shape, generator=g) * 2 - 1) * scale
        self.b, self.s, self.d = b, s, d
        self.lens = torch.tensor(lens, dtype=torch.int32)
        self.live = torch.arange(s).view(1, s) < self.lens.view(b, 1)
        s_xyz, s_points = r(b, N_SRC, 3), r(b, N_SRC, d)
        new_xyz = r(b, s, 3)
        idx = torch.randint(0, N_SRC, (b, s, K), generator=g, dtype=torch.int32)
        self.weights = [r(8, 3, scale=0.8), r(8, scale=0.3), r(8, 8, scale=0.6), r(8, scale=0.3), r(8, 8, scale=0.6), r(8, scale=0.3)]
        gout = r(b, s, (d + 3) * 8)
        pad = ~self.live
        clean_idx, clean_g = idx.clone(), gout.clone()
        clean_idx = torch.where(pad.unsqueeze(-1), (torch.arange(s, dtype=torch.int32) % N_SRC).view(1, s, 1), clean_idx)
        clean_g[pad] = 0.0
        dirty_xyz, dirty_idx, dirty_g = new_xyz.clone(), idx.clone(), gout.clone()
        dirty_xyz[pad], dirty_g[pad] = float("nan"), float("nan")
        bad = torch.where(torch.arange(K) % 2 == 0, -1, BIG).to(torch.int32)
        dirty_idx[pad] = bad
        dev = lambda t: t.to(DEV)
        self.src = (dev(s_xyz), dev(s_points))
        self.clean = (dev(new_xyz), dev(clean_idx), dev(clean_g))
        self.dirty = (dev(dirty_xyz), dev(dirty_idx), dev(dirty_g))
        self.weights = [dev(t) for t in self.weights]
        self.live, self.lens_dev = dev(self.live), dev(self.lens)
        if c_out is not None:
            self.lin = (dev(r(c_out, (d + 3) * 8, scale=0.05)), dev(r(c_out, scale=0.5) + 0.75))   # a bias that is nowhere zero

    def agg(self, be, which, lengths=None):
        new_xyz, idx, _ = which
        kw = {} if lengths is None else dict(centre_lengths=lengths)
        return be.pointconv_agg(self.src[0], new_xyz, self.src[1], idx, *self.weights, **kw)

    def linear(self, be, which, lengths=None):
        new_xyz, idx, _ = which
        kw = {} if lengths is None else dict(centre_lengths=lengths)
        return be.pointconv_linear(self.src[0], new_xyz, self.src[1], idx, *self.weights, *self.lin, 0.1, **kw)

    def grads(self, be, which, lengths=None):
        """-> [out, d s_xyz, d new_xyz, d s_points, 6 weight gradients] through autograd"""
        new_xyz, idx, gout = which
        leaves = [t.clone().requires_grad_(True) for t in (self.src[0], new_xyz, self.src[1], *self.weights)]
        kw = {} if lengths is None else dict(centre_lengths=lengths)
        out = be.pointconv_agg(leaves[0], leaves[1], leaves[2], idx, *leaves[3:], **kw)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, gout))


def check_rows(got, want, live, what):
    assert torch.equal(got[live], want[live]), f"{what}: live rows differ from the dense call"
    pad = got[~live]
    assert pad.numel() == 0 or (pad == 0).all(), f"{what}: padded rows are not exact zeros"


def test_the_entry_points_exist():
    lib = _lib.load()
    assert lib.mcp_pointconv_agg_lengths and lib.mcp_pointconv_linear_lengths and lib.mcp_pointconv_agg_grad_lengths


# (id, b, s, d, points per workgroup of the form the dispatch takes)
FORWARD = [
    ("stream-ppb32", 2, 8211, 32, 32), ("stream-ppb16", 2, 8211, 64, 16), ("stream-ppb8", 2, 8211, 128, 8),
    ("lowlevel256", 3, 77, 32, 8), ("lowlevel1024", 2, 40, 256, 8), ("lowlevel256-d5", 3, 77, 5, 8),
]


@pytest.mark.parametrize("case", FORWARD, ids=[c[0] for c in FORWARD])
def test_aggregate_with_centre_lengths(case):
    _, b, s, d, ppb = case
    be = ops.backend()
    for i, lens in enumerate(length_sets(b, s, ppb)):
        bt = Batch(b, s, d, lens, seed=100 * d + i)
        dense = bt.agg(be, bt.clean)
        got = bt.agg(be, bt.dirty, bt.lens_dev)
        check_rows(got, dense, bt.live, f"lengths {lens}")
        assert torch.equal(got, bt.agg(be, bt.dirty, bt.lens_dev)), "two calls differ"
        assert torch.equal(got, bt.agg(be, bt.dirty, list(lens))), "a list of lengths and a device tensor differ"
    full = bt.agg(be, bt.clean, [s] * b)
    assert torch.equal(full, dense), "full lengths differ from the dense call"
    assert torch.equal(bt.agg(be, bt.clean, bt.lens_dev * 0 + (s + 5)), dense), "the kernel does not clamp a device length to s"


@pytest.mark.parametrize("d", [32, 64])
def test_fused_linear_with_centre_lengths(d):
    b, s = 3, 77
    be = ops.backend()
    for i, lens in enumerate(length_sets(b, s, 32)):
        bt = Batch(b, s, d, lens, seed=7 * d + i, c_out=d)
        dense = bt.linear(be, bt.clean)
        assert (dense != 0).all()                       # leaky(bias + ...) of the dense call: a zero row below is the length form's
        got = bt.linear(be, bt.dirty, bt.lens_dev)
        check_rows(got, dense, bt.live, f"lengths {lens}")
        assert torch.equal(got, bt.linear(be, bt.dirty, bt.lens_dev)), "two calls differ"
    assert torch.equal(bt.linear(be, bt.clean, [s] * b), dense), "full lengths differ from the dense call"


SHORT = (0, 5, 2, 0, 5)   # five elements of five centres: fewer centres than any form's points per workgroup


@pytest.mark.parametrize("fused", [False, True], ids=["aggregate", "fused-linear"])
def test_elements_shorter_than_a_workgroup(fused):
    """s below the form's points per workgroup (8 in the low-level kernel, 32 in the fused one): a workgroup's range touches more than
    two elements, so liveness is looked up per lane and the skip test walks the elements (PcSpan::direct false)."""
    b, s, d = 5, 5, 32
    be = ops.backend()
    bt = Batch(b, s, d, SHORT, seed=11, c_out=d if fused else None)
    call = bt.linear if fused else bt.agg
    dense = call(be, bt.clean)
    got = call(be, bt.dirty, bt.lens_dev)
    check_rows(got, dense, bt.live, f"lengths {SHORT}")
    assert torch.equal(got, call(be, bt.dirty, bt.lens_dev)), "two calls differ"
    assert torch.equal(call(be, bt.clean, [s] * b), dense), "full lengths differ from the dense call"
    none = Batch(b, s, d, (0,) * b, seed=12, c_out=d if fused else None)
    assert (call(be, none.dirty, none.lens_dev) == 0).all(), "a batch without a live centre is not all zeros"


def test_backward_through_the_masked_torch_formulation():
    """d = 5 (d % 4): no backward kernel, so autograd pairs the length kernel's forward with grad.pointconv_agg_lengths_twin.  Against
    the dense call of the same route on the clean batch: the forward's live rows are equal bits and its padded rows zeros (the kernel);
    the gradients are finite under NaN padding, zero on padded centres, and agree to 1e-5 of each tensor's largest magnitude -- both
    sides are float32 torch sums of at most 32 * 3 * 77 terms, in formulations that differ by the masks only."""
    b, s, d = 3, 77, 5
    be = ops.backend()
    names = ["out", "s_xyz", "new_xyz", "s_points", "w0", "b0", "w1", "b1", "w2", "b2"]
    for i, lens in enumerate(length_sets(b, s, 8)):
        bt = Batch(b, s, d, lens, seed=500 + i)
        dense = bt.grads(be, bt.clean)
        got = bt.grads(be, bt.dirty, bt.lens_dev)
        check_rows(got[0], dense[0], bt.live, f"out, lengths {lens}")
        for name, g, w in zip(names[1:], got[1:], dense[1:]):
            assert torch.isfinite(g).all(), f"{name}: not finite under lengths {lens}"
            err, bound = float((g - w).abs().max()), 1e-5 * max(1.0, float(w.abs().max()))
            print(f"masked twin, lengths {lens}, {name}: max error {err:.3e} (bound {bound:.3e})")
            assert err <= bound, f"{name}: differs from the dense route under lengths {lens}"
        assert (got[2][~bt.live] == 0).all(), "new_xyz: gradient rows of padded centres are not exact zeros"


@pytest.mark.parametrize("d", [4, 32, 64, 256])
def test_backward_with_centre_lengths(d):
    b, s = 3, 77
    be = ops.backend()
    names = ["out", "s_xyz", "new_xyz", "s_points", "w0", "b0", "w1", "b1", "w2", "b2"]
    for i, lens in enumerate(length_sets(b, s, 2)):      # a wave takes two centres
        bt = Batch(b, s, d, lens, seed=31 * d + i)
        dense = bt.grads(be, bt.clean)
        got = bt.grads(be, bt.dirty, bt.lens_dev)
        again = bt.grads(be, bt.dirty, bt.lens_dev)
        for name, g, w, a in zip(names, got, dense, again):
            assert torch.isfinite(g).all(), f"{name}: not finite under lengths {lens}"
            if name in ("out", "new_xyz"):
                check_rows(g, w, bt.live, f"{name}, lengths {lens}")
            else:
                assert torch.equal(g, w), f"{name}: differs from the dense call under lengths {lens}"
            assert torch.equal(g, a), f"{name}: two calls differ"
    for name, g, w in zip(names, bt.grads(be, bt.clean, [s] * b), bt.grads(be, bt.clean)):
        assert torch.equal(g, w), f"{name}: full lengths differ from the dense call"


@pytest.mark.parametrize("d", [32, 256])
def test_backward_entry_point_rows(d):
    """The C entry point itself: grad_gxyz and grad_rows per (centre, neighbour) -- live rows the dense call's bits, padded rows
    zeros in buffers that held NaN --, and qlen = NULL is the dense entry point."""
    b, s = 3, 77
    lib = _lib.load()
    bt = Batch(b, s, d, (1, s - 1, 40), seed=5 + d)
    need = lib.mcp_pointconv_agg_grad_workspace_bytes(b, s)

    def raw(which, qlen):
        new_xyz, idx, gout = which
        outs = [torch.full(shape, float("nan"), device=DEV) for shape in ((b, s, 3), (b, s, K, 3), (b, s, K, d), (176,))]
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
        rc = lib.mcp_pointconv_agg_grad_lengths(b, N_SRC, s, d, K, _lib.fptr(bt.src[0]), _lib.fptr(new_xyz), _lib.fptr(bt.src[1]), _lib.iptr(idx),
                                                None if qlen is None else _lib.iptr(qlen), *[_lib.fptr(w) for w in bt.weights], _lib.fptr(gout),
                                                *[_lib.fptr(o) for o in outs], ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        return outs

    dense = raw(bt.clean, None)
    got = raw(bt.dirty, bt.lens_dev)
    for name, g, w in zip(("grad_new_xyz", "grad_gxyz", "grad_rows"), got, dense):
        check_rows(g, w, bt.live, name)
    assert torch.equal(got[3], dense[3]), "weight gradients differ from the dense call"
    full = raw(bt.clean, bt.lens_dev * 0 + s)
    for g, w in zip(full, dense):
        assert torch.equal(g, w), "full lengths differ from the dense call"
