"""-m gpu: the hand-written backward of the inverse-distance interpolation weights (mcp_interp3_weights_grad, csrc/interp3_grad.hip)
behind HipBackend.interp3_search: against autograd over the unfused formula (grad.interp3_weights_twin) on the device and against
float64 autograd over the same formula, at max|hip - ref| <= 2e-4 max|ref| + 2e-5 (the project's compare_grads bound); finite at
coincident points (distance exactly 0: the clamp branch); bit-reproducible; either output alone equals the pair's."""
import pytest
import torch

from mocopci_amd import _lib, grad, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cloud(seed, b, n, scale=10.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(b, n, 3, generator=g) * 2 - 1) * scale


def rnd(seed, *shape, scale=1.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale


def graph_nodes(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(nx for nx, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


def clouds(n, s):
    dense, sparse = cloud(300 + n, 2, n).to(DEV), cloud(301 + s, 2, s).to(DEV)
    if (n, s) == (900, 40):
        dense[:, :20] = sparse[:, :20]                          # distance exactly 0 to the first neighbour: the clamp branch
        sparse[:, 39] = sparse[:, 38] + torch.tensor([0.3, 0.0, 0.0], device=DEV)   # two sparse rows 0.3 apart, and a third of the dense
        dense[:, 300:600] = (sparse[:, 38:39] + sparse[:, 39:40]) / 2 + rnd(302, 2, 300, 3, scale=0.05).to(DEV)   # points around their
    return dense, sparse                                        # midpoint: both rows' scatter segments have ~300 entries


def test_the_entry_point_exists_and_the_weights_have_no_recompute_node():
    assert hasattr(_lib.load(), "mcp_interp3_weights_grad")
    be = ops.backend()
    dense, sparse = clouds(300, 100)
    idx3, w3 = be.interp3_search(dense.requires_grad_(True), sparse.requires_grad_(True))
    names = graph_nodes(w3)
    assert "RecomputeFnBackward" not in names and "_Interp3WeightsFnBackward" in names, names
    with torch.no_grad():
        assert torch.equal(w3.detach(), be.interp3_search(dense, sparse)[1])


@pytest.mark.parametrize("n,s", [(300, 100), (4096, 2048), (900, 40)])
def test_interp3_weights_backward_matches_the_unfused_formula_and_float64(n, s):
    be = ops.backend()
    dense, sparse = clouds(n, s)
    idx3 = be.interp3_search(dense, sparse)[0]
    if (n, s) == (900, 40):
        r0 = (sparse[torch.arange(2, device=DEV).view(2, 1), idx3[:, :20, 0].long()] - dense[:, :20]).norm(dim=-1)
        assert bool((r0 == 0).all())                            # the coincident points really are coincident
    gw = rnd(303, 2, n, 3).to(DEV)

    def grads(fn, dtype=torch.float32, wanted=(True, True)):
        leaves = [t.detach().to(dtype).requires_grad_(wt) for t, wt in zip((dense, sparse), wanted)]
        return torch.autograd.grad(fn(*leaves), [t for t in leaves if t.requires_grad], gw.to(dtype))
    hip = grads(lambda d, s_: be.interp3_search(d, s_)[1])
    again = grads(lambda d, s_: be.interp3_search(d, s_)[1])
    twin = grads(lambda d, s_: grad.interp3_weights_twin(be.group_rows, d, s_, idx3))
    bi = torch.arange(2, device=DEV).view(2, 1, 1)
    ref = grads(lambda d, s_: grad.interp3_weights_twin(lambda pts, i: pts[bi, i.long()], d, s_, idx3), torch.float64)
    only_dense = grads(lambda d, s_: be.interp3_search(d, s_)[1], wanted=(True, False))
    only_sparse = grads(lambda d, s_: be.interp3_search(d, s_)[1], wanted=(False, True))
    assert torch.equal(only_dense[0], hip[0]) and torch.equal(only_sparse[0], hip[1])
    print(f"\n[n={n} s={s}] {'gradient':8s} {'max|f64|':>10s} {'hip-f64':>10s} {'twin-f64':>10s} {'ratio':>7s} {'hip-twin':>10s}")
    failures = []
    for name, a, a2, t32, r64 in zip(("dense", "sparse"), hip, again, twin, ref):
        e_hip, e_twin = float((a.double() - r64).abs().max()), float((t32.double() - r64).abs().max())
        e_ht, s64, s32 = float((a - t32).abs().max()), float(r64.abs().max()), float(t32.abs().max())
        print(f"{'':{len(f'[n={n} s={s}] ')}s}{name:8s} {s64:10.3e} {e_hip:10.3e} {e_twin:10.3e} {e_hip / max(e_twin, 1e-30):7.2f} {e_ht:10.3e}")
        if not torch.equal(a, a2):
            failures.append(f"{name}: two runs differ")
        if not torch.isfinite(a).all():
            failures.append(f"{name}: not finite")
        if not e_ht <= 2e-4 * s32 + 2e-5:
            failures.append(f"{name}: |hip - twin| {e_ht:.2e}, gradient scale {s32:.2e}")
        if not e_hip <= 2e-4 * s64 + 2e-5:
            failures.append(f"{name}: |hip - f64| {e_hip:.2e}, gradient scale {s64:.2e}")
    assert not failures, "; ".join(failures)
