"""-m gpu: the EMD backward (csrc/emd_grad.hip: emd_grad_kernel<SIDE, LEN>, matchcost_kernel, matchcost_grad1_kernel,
matchcost_grad2_kernel) and the backward of the interpolation weights (csrc/interp3_grad.hip: interp3_weights_grad_kernel) at point
counts on and next to the kernels' own boundaries; tests/test_emd_grad.py, test_emd_lengths_gpu.py and
test_interp3_weights_grad_gpu.py compare them at clouds of 300 to 8192 points.  kernel_variants.EMD_GRAD_CASES / INTERP3_GRAD_CASES
are the shapes; test_kernel_variants_cpu.py checks that they launch every kernel the two units emit.

emd_grad_kernel: 64 lane points per workgroup, the other cloud streamed in tiles of 512 of which wave w takes entries [64 w, 64 w + 64);
yardstick of test_emd_grad.py: float64 gradients at the device's own match, within 1e-5 max |f64|.  The matchcost kernels take ANY match
array, so a random non-negative one makes the float64 formulas of grads_from_match an exact reference (cost: rtol 1e-6, the project's
figure for matchcost_kernel; gradients 1e-5 max |f64|).  grad1 splits m into eighths (empty ranges when m < 8), grad2 takes 8 rows per
workgroup and strides 256 lanes over n, the cost 1024 lanes.

interp3_weights_grad_kernel: 256 dense points per workgroup.  The project's bound (2e-4 max |ref| + 2e-5 against float64 and against the
unfused twin) is a max-norm bound and gradients scale as 1 / d^2, so on random clouds the nearest pair dominates it and a wrong row
elsewhere hides below.  band_clouds() therefore keeps every distance in a narrow band (dense points sit near the centres of the unit
cells of a jittered sparse lattice, never on a sparse point) and spread_gw() gives the upstream gradient a fixed spread over the three
neighbours (about +-(1, 0, -1): with a plain random one a row's gradient is below 1 % of the maximum once in a few hundred rows).  In
float64 every dense point's gradient norm is then at least 1 % of the tensor's maximum -- asserted here, and checked on the CPU with an
exhaustive 3-NN search when these cases were written (the smallest row is 23 % of the maximum or more in every case) -- so the bound
bites on every row.

Lines starting with ERR carry each error as a fraction of its bound (profiles/attention_wide_grad_edges_accuracy.txt)."""
import pytest
import torch

from mocopci_amd import _lib, emd, emd_cuda, grad, ops
from tests import kernel_variants as kv
from tests.test_emd_grad import clouds, grads_from_match, lean_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2
GRAD_COST = (1.7, -0.6)


def ratio(got, want, rel, floor=0.0):
    """max |got - want| as a fraction of rel max |want| + floor."""
    want = want.double().to(got.device)
    return float((got.double() - want).abs().max()) / (rel * float(want.abs().max()) + floor)


# ---- emd_grad_kernel through the public metric ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", kv.emd_cases("lean"), ids=lambda c: f"{c['n']}x{c['m']}")
def test_emd_backward_at_the_lane_block_and_tile_boundaries(c):
    n, m = c["n"], c["m"]
    x, y = clouds(B, n, m, 7 + 3 * n + m)
    g = torch.tensor(GRAD_COST)
    _, g1, g2 = lean_grads(x, y, g)
    _, a1, a2 = lean_grads(x, y, g)
    assert torch.equal(g1, a1) and torch.equal(g2, a2), "two runs differ"
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all())
    match = emd.approxmatch_forward(x.to(DEV), y.to(DEV))
    w1, w2 = grads_from_match(g.to(DEV), x.to(DEV), y.to(DEV), match)
    r1, r2 = ratio(g1, w1, 1e-5), ratio(g2, w2, 1e-5)
    print(f"ERR emd_grad[n={n},m={m}] grad1={r1:.3f} grad2={r2:.3f} of the bound")
    assert float(w1.abs().max()) > 0 and float(w2.abs().max()) > 0
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


def emd_grad_lengths(x, y, g, len1, len2, kept_with_lengths):
    """mcp_emd_grad_lengths on the levels the forward kept -> (grad1, grad2), both pre-filled with NaN."""
    lib = _lib.load()
    n, m = x.shape[1], y.shape[1]
    l1, l2 = ops.lengths_tensor(list(len1), B, n, DEV), ops.lengths_tensor(list(len2), B, m, DEV)
    levels = emd._emd(x, y, False, keep_levels=True, **(dict(len1=l1, len2=l2) if kept_with_lengths else {}))[2]
    g1, g2 = torch.full((B, n, 3), float("nan"), device=DEV), torch.full((B, m, 3), float("nan"), device=DEV)
    with torch.cuda.device(x.device):
        _lib.check(lib.mcp_emd_grad_lengths(B, n, m, _lib.fptr(g), _lib.fptr(x), _lib.fptr(y), _lib.iptr(l1), _lib.iptr(l2), _lib.fptr(levels),
                                            _lib.fptr(g1), _lib.fptr(g2), _lib.stream()))
    torch.cuda.synchronize()
    return g1, g2


@pytest.mark.parametrize("c", kv.emd_cases("lean-lengths"), ids=lambda c: f"{c['n']}x{c['m']}-len{'_'.join(map(str, c['len1'] + c['len2']))}")
def test_emd_backward_length_instantiations_at_the_boundaries(c):
    """Full lengths: the plain call's bits.  Short lengths: live rows are the plain call on the sliced clouds bit for bit, the rows
    beyond are exact zeros."""
    n, m, len1, len2 = c["n"], c["m"], c["len1"], c["len2"]
    x, y = clouds(B, n, m, 7 + 3 * n + m)
    g = torch.tensor(GRAD_COST)
    full = len1 == (n,) * B and len2 == (m,) * B
    g1, g2 = emd_grad_lengths(x.to(DEV), y.to(DEV), g.to(DEV), len1, len2, kept_with_lengths=not full)
    if full:
        _, p1, p2 = lean_grads(x, y, g)
        assert torch.equal(g1, p1) and torch.equal(g2, p2), "full lengths differ from the plain call"
        return
    for b in range(B):
        a, k = len1[b], len2[b]
        _, s1, s2 = lean_grads(x[b:b + 1, :a].contiguous(), y[b:b + 1, :k].contiguous(), g[b:b + 1])
        assert torch.equal(g1[b, :a], s1[0]) and torch.equal(g2[b, :k], s2[0]), f"element {b} differs from its sliced call"
        assert bool((g1[b, a:] == 0).all()) and bool((g2[b, k:] == 0).all()), f"element {b}: rows beyond the lengths are not zero"
        assert float(s1.abs().max()) > 0 and float(s2.abs().max()) > 0


# ---- the explicit-match kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", kv.emd_cases("match"), ids=lambda c: f"{c['n']}x{c['m']}")
def test_matchcost_kernels_with_fewer_rows_than_lanes(c):
    n, m = c["n"], c["m"]
    x, y = (t.to(DEV) for t in clouds(B, n, m, 19 + 5 * n + m))
    match = torch.rand(B, m, n, generator=torch.Generator().manual_seed(n + 31 * m)).to(DEV)
    g = torch.tensor(GRAD_COST, device=DEV)
    cost = emd_cuda.matchcost_forward(x, y, match)
    d2 = ((y.double().unsqueeze(2) - x.double().unsqueeze(1)) ** 2).sum(-1)            # (B,M,N)
    exact = (match.double() * d2).sum((1, 2))
    g1, g2 = emd_cuda.matchcost_backward(g, x, y, match)
    a1, a2 = emd_cuda.matchcost_backward(g, x, y, match)
    assert torch.equal(g1, a1) and torch.equal(g2, a2) and torch.equal(cost, emd_cuda.matchcost_forward(x, y, match)), "two runs differ"
    w1, w2 = grads_from_match(g, x, y, match)
    rc = float(((cost.double() - exact).abs() / (1e-6 * exact.abs())).max())
    r1, r2 = ratio(g1, w1, 1e-5), ratio(g2, w2, 1e-5)
    print(f"ERR matchcost[n={n},m={m}] cost={rc:.3f} grad1={r1:.3f} grad2={r2:.3f} of the bound")
    assert float(exact.abs().min()) > 0 and float(w1.abs().max()) > 0 and float(w2.abs().max()) > 0
    torch.testing.assert_close(cost.double(), exact, rtol=1e-6, atol=0)
    assert g1.shape == (B, n, 3) and g2.shape == (B, m, 3)
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


# ---- interp3_weights_grad_kernel ---------------------------------------------------------------------------------------------------------
def band_clouds(n, s, seed):
    """dense (B,n,3), sparse (B,s,3) on the CPU.  The sparse points are the first s nodes of a 2 x 2 x 10 lattice of unit spacing
    (node i at (i % 2, (i // 2) % 2, i // 4): the first three are a triangle), jittered by at most 0.1 per axis.  A dense point sits at
    the centre of one of the lattice's unit cells (s = 3: above the triangle's centroid), jittered by at most 0.15 per axis: its three
    nearest sparse points are between 0.38 and 1.24 away."""
    gen = torch.Generator().manual_seed(seed)
    i = torch.arange(s)
    sparse = torch.stack((i % 2, (i // 2) % 2, i // 4), dim=-1).float().expand(B, s, 3) + (torch.rand(B, s, 3, generator=gen) - 0.5) * 0.2
    if s == 3:
        base = torch.tensor([1 / 3, 1 / 3, 0.5]).expand(B, n, 3)
    else:
        cell = torch.randint(0, s // 4 - 1, (B, n), generator=gen)
        base = torch.stack((torch.full((B, n), 0.5), torch.full((B, n), 0.5), cell.float() + 0.5), dim=-1)
    dense = base + (torch.rand(B, n, 3, generator=gen) - 0.5) * 0.3
    return dense.contiguous(), sparse.contiguous()


def spread_gw(n, seed):
    """dL/dw (B,n,3) on the CPU: +-(1, 0, -1) over a point's three neighbours plus 0.2 N(0, 1).  The gradient of a dense point is then
    about a r_0 - b r_2 with a, b of one sign and r_0 - r_2 the vector between two distinct sparse points: never small."""
    gen = torch.Generator().manual_seed(seed)
    sign = (torch.randint(0, 2, (B, n, 1), generator=gen) * 2 - 1).float()
    return sign * torch.tensor([1.0, 0.0, -1.0]) + 0.2 * torch.randn((B, n, 3), generator=gen)


def weights_f64(dense, sparse, idx3):
    bi = torch.arange(dense.shape[0], device=dense.device).view(-1, 1, 1)
    return grad.interp3_weights_twin(lambda pts, i: pts[bi, i.long()], dense, sparse, idx3)


def weights_grad_entry(dense, sparse, idx3, gw, want_dense=True, want_nb=True):
    """mcp_interp3_weights_grad -> (grad_dense or None, grad_nb (B,N,3,3) or None), pre-filled with NaN."""
    lib = _lib.load()
    n, s = dense.shape[1], sparse.shape[1]
    gd = torch.full((B, n, 3), float("nan"), device=DEV) if want_dense else None
    nb = torch.full((B, n, 3, 3), float("nan"), device=DEV) if want_nb else None
    with torch.cuda.device(dense.device):
        _lib.check(lib.mcp_interp3_weights_grad(B, n, s, _lib.fptr(dense), _lib.fptr(sparse), _lib.iptr(idx3), _lib.fptr(gw),
                                                None if gd is None else _lib.fptr(gd), None if nb is None else _lib.fptr(nb), _lib.stream()))
    torch.cuda.synchronize()
    return gd, nb


@pytest.mark.parametrize("c", kv.INTERP3_GRAD_CASES, ids=lambda c: f"n={c['n']},s={c['s']}" + (",coincident" if c["coincident"] else ""))
def test_interp3_weights_backward_at_the_workgroup_boundaries(c):
    be = ops.backend()
    n, s, k = c["n"], c["s"], c["coincident"]
    dense, sparse = (t.to(DEV) for t in band_clouds(n, s, 900 + n + s))
    if k:   # distance exactly 0 to the first neighbour: the clamp branch, in the first workgroup and for the one point of the last
        dense[:, :k] = sparse[:, :k]
        dense[:, n - 1] = sparse[:, k]
    idx3 = be.interp3_search(dense, sparse)[0]
    gw = spread_gw(n, 903 + n).to(DEV)

    def grads(fn, dtype=torch.float32):
        leaves = [t.detach().to(dtype).requires_grad_(True) for t in (dense, sparse)]
        return torch.autograd.grad(fn(*leaves), leaves, gw.to(dtype))
    hip = grads(lambda d, s_: be.interp3_search(d, s_)[1])
    again = grads(lambda d, s_: be.interp3_search(d, s_)[1])
    twin = grads(lambda d, s_: grad.interp3_weights_twin(be.group_rows, d, s_, idx3))
    ref = grads(lambda d, s_: weights_f64(d, s_, idx3), torch.float64)
    if not k:
        norms = ref[0].norm(dim=-1)
        assert float(norms.min()) >= 0.01 * float(norms.max()), f"a dense row's gradient is {float(norms.min() / norms.max()):.1e} of the largest"
    # the C entry: both outputs, and either one alone
    gd, nb = weights_grad_entry(dense, sparse, idx3, gw)
    assert torch.equal(gd, hip[0]), "the public call's grad_dense differs from the entry's"
    assert torch.equal(weights_grad_entry(dense, sparse, idx3, gw, want_nb=False)[0], gd), "grad_dense alone differs"
    assert torch.equal(weights_grad_entry(dense, sparse, idx3, gw, want_dense=False)[1], nb), "grad_nb alone differs"
    assert bool(torch.isfinite(nb).all())
    if k:
        hit = torch.cat((torch.arange(k), torch.tensor([n - 1]))).to(DEV)
        bi = torch.arange(B, device=DEV).view(B, 1)
        assert bool(((sparse[bi, idx3[:, hit, 0].long()] - dense[:, hit]).norm(dim=-1) == 0).all())   # the coincident points really are coincident
        assert bool((nb[:, hit, 0] == 0).all()), "grad_nb of a coincident neighbour is not zero"
        assert bool((nb[:, hit, 1:] != 0).any())
    label, failures, line = f"n={n},s={s}" + (",coincident" if k else ""), [], []
    for name, a, a2, t32, r64 in zip(("dense", "sparse"), hip, again, twin, ref):
        r_f64, r_twin = ratio(a, r64, 2e-4, 2e-5), ratio(a, t32, 2e-4, 2e-5)
        line.append(f"{name}: f64={r_f64:.3f} twin={r_twin:.3f}")
        if not torch.equal(a, a2):
            failures.append(f"{name}: two runs differ")
        if not torch.isfinite(a).all():
            failures.append(f"{name}: not finite")
        if not r_twin <= 1.0:
            failures.append(f"{name}: |hip - twin| is {r_twin:.2f} of the bound")
        if not r_f64 <= 1.0:
            failures.append(f"{name}: |hip - f64| is {r_f64:.2f} of the bound")
    print(f"ERR interp3_weights_grad[{label}] " + " ".join(line) + " of the bound")
    assert not failures, "; ".join(failures)
