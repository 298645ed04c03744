"""-m gpu: the fusion layer's own kernels under per-cloud lengths (csrc/fusion_lengths.hip: mcp_fusion_lengths /
mcp_fusion_grad_lengths; csrc/fusion_bn_lengths.hip: mcp_fusion_bn_forward_save_lengths / mcp_fusion_bn_backward_saved_lengths) and the
public routes that reach them (ops.HipBackend.fusion_mlp(lengths=), fusion_bn(lengths=)).

The shapes are the CASES of tests/fusion_bn_lengths_reference.py, each named after the edge it reaches (one live point beside three
dead waves, an empty element in a round-robin deal, no live point, a padded tail inside a workgroup's deal, a padded first point, a
padded total above the backward's one-workgroup-per-CU grid, above both caps); the two large ones skip off 256 CUs as
test_fusion_bn_lengths_gpu.py does.  The forward alone also runs b = 2, n = 8200, lens = (8200, 37): 16400 points, above its
4096-workgroup grid, so workgroups loop.

Every case: padded rows of p1, p2 and of the upstream gradient are NaN, padded rows of the lists are -1 and 2^30, every output and
workspace buffer is NaN-filled beforehand.  Everything is held to the BITS of a dense call (torch.equal) -- no tolerance anywhere:
the forward to mcp_fusion on each cloud alone, the backward to mcp_fusion_grad on the batch zeroed by hand (zero rows, list rows 0,
zero upstream rows), the kept-score pair to the pair that keeps nothing."""
import ctypes
import types

import pytest
import torch

from mocopci_amd import _lib, ops
from tests import fusion_bn_lengths_reference as lr
from tests import fusion_bn_reference as br
from tests.fusion_bn_lengths_reference import CASES, case_id
from tests.test_fused_grad_variants_gpu import poisoned_buffers
from tests.test_fusion_bn_lengths_gpu import DEV, poisoned, skip_unless_256

pytestmark = pytest.mark.gpu
LOOPING = dict(tag="forward-grid-loops", b=2, n=8200, lens=(8200, 37))   # forward only
NEW = ("mcp_fusion_lengths", "mcp_fusion_grad_lengths", "mcp_fusion_bn_forward_save_lengths", "mcp_fusion_bn_backward_saved_lengths")
_inputs = {}


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return torch.cuda.current_stream().cuda_stream


def inputs(case):
    """The case's padded batch (CPU; padded rows zero, list rows 0), computed once and left unchanged: what `poisoned` reads."""
    key = case["tag"]
    if key not in _inputs:
        leaves, idx, live = lr.case_inputs(case)
        g = torch.randn(case["b"] * case["n"], 3, generator=torch.Generator().manual_seed(31))
        g[~live.reshape(-1)] = 0.0
        _inputs[key] = types.SimpleNamespace(case=case, leaves=leaves, idx=idx, live=live, g=g)
    return _inputs[key]


def device_lens(case, values=None):
    return torch.tensor(case["lens"] if values is None else values, dtype=torch.int32, device=DEV)


def clean(prep):
    """(leaves, halves, g) on the device: the batch zeroed by hand"""
    return [t.to(DEV) for t in prep.leaves], tuple(t.to(DEV) for t in prep.idx), prep.g.view(prep.case["b"], prep.case["n"], 3).to(DEV)


def forward(leaves, halves, lens="dense"):
    """mcp_fusion (lens == "dense") or mcp_fusion_lengths (a device tensor, or None for len = NULL) into a NaN-filled out"""
    lib = _lib.load()
    B, N, _ = leaves[0].shape
    with poisoned_buffers():
        out = torch.empty(B, N, 3, device=DEV)
    head = (B, N, 64, P(leaves[0]), P(leaves[1]), P(halves[0]), P(halves[1]))
    if isinstance(lens, str):
        rc = lib.mcp_fusion(*head, *[P(t) for t in leaves[2:8]], P(out), stream())
    else:
        rc = lib.mcp_fusion_lengths(*head, P(lens), *[P(t) for t in leaves[2:8]], P(out), stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


def backward(leaves, halves, g, lens="dense"):
    """mcp_fusion_grad / mcp_fusion_grad_lengths into NaN-filled outputs and workspace -> (grad_p1, grad_nb, grad_weights)"""
    lib = _lib.load()
    B, N, _ = leaves[0].shape
    need = lib.mcp_fusion_grad_workspace_bytes(B, N)
    with poisoned_buffers():
        d_p1, d_nb = torch.empty(B, N, 3, device=DEV), torch.empty(B, N, 64, 3, device=DEV)
        d_w, ws = torch.empty(lib.mcp_fusion_grad_floats(), device=DEV), torch.empty(need, dtype=torch.uint8, device=DEV)
    head = (B, N, 64, P(leaves[0]), P(leaves[1]), P(halves[0]), P(halves[1]))
    tail = (*[P(t) for t in leaves[2:8]], P(g), P(d_p1), P(d_nb), P(d_w), P(ws), need, stream())
    rc = lib.mcp_fusion_grad(*head, *tail) if isinstance(lens, str) else lib.mcp_fusion_grad_lengths(*head, P(lens), *tail)
    assert rc == 0
    torch.cuda.synchronize()
    return d_p1, d_nb, d_w


def test_the_four_entry_points_exist():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES


@pytest.mark.parametrize("case", CASES + [LOOPING], ids=case_id)
def test_forward_with_lengths_is_the_dense_kernel_on_each_cloud_alone(case):
    if case is not LOOPING:
        skip_unless_256(case)
    prep = inputs(case)
    B, N = case["b"], case["n"]
    live = prep.live.to(DEV)
    lens = device_lens(case)
    leaves, halves, _ = poisoned(prep)
    out = forward(leaves, halves, lens)
    assert torch.isfinite(out).all(), "out is not finite"
    assert not out[~live].any(), "a padded row of out is not zero"
    cl, ch, _ = clean(prep)
    for e, ln in enumerate(case["lens"]):
        if ln > 0:
            alone = forward([cl[0][e:e + 1, :ln].contiguous(), cl[1][e:e + 1, :ln].contiguous()] + cl[2:8], [h[e:e + 1, :ln].contiguous() for h in ch])
            assert torch.equal(out[e, :ln], alone[0]), f"element {e}: other bits than mcp_fusion on the cloud alone"
    assert torch.equal(out, forward(leaves, halves, lens)), "a second call gives other bits"
    ol, oh, _ = poisoned(prep, value=7.5, ia_pad=3 % N, ib_pad=5 % N)
    assert torch.equal(out, forward(ol, oh, lens)), "other values in the padded rows change the result"
    # len = NULL and len = (n, ..., n) are mcp_fusion
    dense = forward(cl, ch)
    assert torch.equal(dense, forward(cl, ch, None)), "len = NULL gives other bits than mcp_fusion"
    assert torch.equal(dense, forward(cl, ch, device_lens(case, [N] * B))), "every length n gives other bits than mcp_fusion"
    # the kernel clamps: -3 is 0, n + 5 is n
    odd = [-3 if ln == 0 else (N + 5 if ln == N else ln) for ln in case["lens"]]
    if odd != list(case["lens"]):
        assert torch.equal(out, forward(leaves, halves, device_lens(case, odd))), "lengths of -3 / n + 5 do not behave as 0 / n"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_backward_with_lengths_is_the_dense_kernel_on_the_batch_zeroed_by_hand(case):
    skip_unless_256(case)
    prep = inputs(case)
    B, N = case["b"], case["n"]
    live = prep.live.to(DEV)
    lens = device_lens(case)
    leaves, halves, g = poisoned(prep)
    got = backward(leaves, halves, g, lens)
    cl, ch, cg = clean(prep)
    want = backward(cl, ch, cg)
    for name, a, b in zip(("grad_p1", "grad_nb", "grad_weights"), got, want):
        assert torch.isfinite(a).all(), f"{name}: not finite"
        assert torch.equal(a, b), f"{name}: other bits than mcp_fusion_grad on the batch zeroed by hand"
    assert not got[0][~live].any() and not got[1][~live].any(), "a padded point has a gradient"
    again = backward(leaves, halves, g, lens)
    other = backward(*poisoned(prep, value=7.5, ia_pad=3 % N, ib_pad=5 % N, g_pad=1.0), lens)
    for name, a, a2, a3 in zip(("grad_p1", "grad_nb", "grad_weights"), got, again, other):
        assert torch.equal(a, a2), f"{name}: a second call gives other bits"
        assert torch.equal(a, a3), f"{name}: other values in the padded rows change the result"
    # on the whole batch (every point with an upstream row): full lengths and len = NULL are mcp_fusion_grad
    fg = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(32)).to(DEV)
    dense = backward(cl, ch, fg)
    for tag, ln in (("len = NULL", None), ("every length n", device_lens(case, [N] * B))):
        for name, a, b in zip(("grad_p1", "grad_nb", "grad_weights"), dense, backward(cl, ch, fg, ln)):
            assert torch.equal(a, b), f"{name}: {tag} gives other bits than mcp_fusion_grad"


def bn_vector(aff):
    bn = torch.zeros(1024, device=DEV)
    at = 0
    for c, gm, bt in zip((64, 64, 128), aff[0::2], aff[1::2]):
        bn[at + 2 * c:at + 3 * c], bn[at + 3 * c:at + 4 * c] = gm, bt
        at += 4 * c
    return bn


def bn_forward(name, leaves, halves, lens, save):
    """One of the four train-mode forwards through the C ABI -> dict(out, bn, var, count, save_c, save_z, save_s)"""
    lib = _lib.load()
    B, N, _ = leaves[0].shape
    rows, need = B * N * 64, lib.mcp_fusion_bn_workspace_bytes(B, N)
    with_len = name.endswith("_lengths")
    r = dict(bn=bn_vector(leaves[8:]))
    with poisoned_buffers():
        r.update(var=torch.empty(256, device=DEV), out=torch.empty(B, N, 3, device=DEV), count=torch.empty(1, dtype=torch.int32, device=DEV),
                 save_c=torch.empty(rows, dtype=torch.int32, device=DEV), save_z=torch.empty(rows, device=DEV), save_s=torch.empty(rows, device=DEV),
                 ws=torch.empty(need, dtype=torch.uint8, device=DEV))
    args = [B, N, 64, P(leaves[0]), P(leaves[1]), P(halves[0]), P(halves[1])] + ([P(lens)] if with_len else [])
    args += [P(t) for t in leaves[2:8]] + [br.EPS, P(r["bn"]), P(r["var"]), P(r["out"])] + ([P(r["count"])] if with_len else [])
    args += [P(r["save_c"]), P(r["save_z"]), P(r["save_s"])] if save else []
    assert getattr(lib, name)(*args, P(r["ws"]), need, stream()) == 0, name
    torch.cuda.synchronize()
    return r


def bn_backward(name, leaves, halves, lens, bn, g, kept):
    """One of the four train-mode backwards through the C ABI -> dict(d_p1, d_nb, d_w, d_aff)"""
    lib = _lib.load()
    B, N, _ = leaves[0].shape
    rows, need = B * N * 64, lib.mcp_fusion_bn_grad_workspace_bytes(B, N)
    with poisoned_buffers():
        scr = dict(row_c=torch.empty(rows, dtype=torch.int32, device=DEV), row_dy=torch.empty(rows, device=DEV), row_a=torch.empty(rows, device=DEV),
                   dy2=torch.empty(rows, 64, device=DEV), dy1=torch.empty(rows, 64, device=DEV), d_p1=torch.empty(B, N, 3, device=DEV),
                   d_nb=torch.empty(B, N, 64, 3, device=DEV), d_w=torch.empty(lib.mcp_fusion_grad_floats(), device=DEV),
                   d_aff=torch.empty(512, device=DEV), ws=torch.empty(need, dtype=torch.uint8, device=DEV))
    args = [B, N, 64, P(leaves[0]), P(leaves[1]), P(halves[0]), P(halves[1])] + ([P(lens)] if name.endswith("_lengths") else [])
    args += [P(t) for t in leaves[2:8]] + [P(bn), P(g)] + ([P(kept["save_c"]), P(kept["save_z"]), P(kept["save_s"])] if kept else [])
    args += [P(scr[k]) for k in ("row_c", "row_dy", "row_a", "dy2", "dy1", "d_p1", "d_nb", "d_w", "d_aff", "ws")]
    assert getattr(lib, name)(*args, need, stream()) == 0, name
    torch.cuda.synchronize()
    return {k: scr[k] for k in ("d_p1", "d_nb", "d_w", "d_aff")}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_pair_that_keeps_its_scores_is_the_pair_that_keeps_nothing(case):
    skip_unless_256(case)
    prep = inputs(case)
    live = prep.live.to(DEV)
    lens = device_lens(case)
    leaves, halves, g = poisoned(prep)
    plain = bn_forward("mcp_fusion_bn_forward_lengths", leaves, halves, lens, False)
    kept = bn_forward("mcp_fusion_bn_forward_save_lengths", leaves, halves, lens, True)
    for k in ("out", "bn", "var", "count"):
        assert torch.equal(plain[k], kept[k]), f"{k}: the forward that keeps its scores gives other bits"
    assert int(kept["count"]) == int(live.sum())
    chan = kept["save_c"].view(case["b"], case["n"], 64)[live]
    assert ((chan >= 0) & (chan <= 127)).all(), "a kept channel of a live row is outside 0..127"
    a = bn_backward("mcp_fusion_bn_backward_lengths", leaves, halves, lens, plain["bn"], g, None)
    b = bn_backward("mcp_fusion_bn_backward_saved_lengths", leaves, halves, lens, kept["bn"], g, kept)
    for k in a:
        assert torch.isfinite(b[k]).all(), f"{k}: not finite"
        assert torch.equal(a[k], b[k]), f"{k}: the backward that reads the kept scores gives other bits"
    assert not b["d_p1"][~live].any() and not b["d_nb"][~live].any(), "a padded point has a gradient"
    # len = NULL is the dense pair
    cl, ch, cg = clean(prep)
    dense = bn_forward("mcp_fusion_bn_forward_save", cl, ch, None, True)
    null = bn_forward("mcp_fusion_bn_forward_save_lengths", cl, ch, None, True)
    for k in ("out", "bn", "var", "save_c", "save_z", "save_s"):
        assert torch.equal(dense[k].view(torch.int32), null[k].view(torch.int32)), f"{k}: len = NULL gives other bits than mcp_fusion_bn_forward_save"
    assert int(null["count"]) == case["b"] * case["n"]
    a = bn_backward("mcp_fusion_bn_backward_saved", cl, ch, None, dense["bn"], cg, dense)
    b = bn_backward("mcp_fusion_bn_backward_saved_lengths", cl, ch, None, dense["bn"], cg, dense)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k}: len = NULL gives other bits than mcp_fusion_bn_backward_saved"


@pytest.fixture
def calls(monkeypatch):
    """the names of the library calls that go through ops._call, in order"""
    names, real = [], ops._call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(ops, "_call", recording)
    return names


def test_fusion_mlp_with_lengths_runs_the_length_kernels(calls):
    case = next(c for c in CASES if c["tag"] == "empty-middle")
    prep = inputs(case)
    be = ops.backend()
    lens = device_lens(case)
    leaves, halves, g = poisoned(prep)
    with poisoned_buffers():
        plain = be.fusion_mlp(leaves[0], leaves[1], halves, *leaves[2:8], lengths=lens)
    assert "mcp_fusion_lengths" in calls and "mcp_fusion" not in calls, calls
    assert torch.equal(plain, forward(leaves, halves, lens))
    del calls[:]
    lv = [t.clone().requires_grad_(True) for t in leaves[:8]]
    with poisoned_buffers():
        out = be.fusion_mlp(lv[0], lv[1], halves, *lv[2:], lengths=lens)
        assert "mcp_fusion_lengths" in calls and "mcp_fusion" not in calls, calls
        grads = torch.autograd.grad(out, lv, g)
    assert "mcp_fusion_grad_lengths" in calls and "mcp_fusion_grad" not in calls, calls
    assert torch.equal(out.detach(), plain) and all(torch.isfinite(t).all() for t in grads)
    live = prep.live.to(DEV)
    assert not grads[0][~live].any() and not grads[1][~live].any(), "a padded point has a gradient"


def test_fusion_bn_with_lengths_keeps_its_scores_unless_switched_off(calls, monkeypatch):
    case = next(c for c in CASES if c["tag"] == "empty-middle")
    prep = inputs(case)
    be = ops.backend()
    lens = device_lens(case)
    leaves, halves, g = poisoned(prep)
    assert type(be).FUSION_BN_KEEP_SCORES_WITH_LENGTHS is True

    def run():
        del calls[:]
        lv = [t.clone().requires_grad_(True) for t in leaves]
        with poisoned_buffers():
            res = be.fusion_bn(lv[0], lv[1], halves, lv[2:8], lv[8:], br.EPS, lengths=lens)
            grads = torch.autograd.grad(res[0], lv, g)
        return [t.detach() for t in res] + list(grads), [n for n in calls if n.startswith("mcp_fusion_bn_") and n.endswith("_lengths")]
    kept, kept_calls = run()
    assert kept_calls == ["mcp_fusion_bn_forward_save_lengths", "mcp_fusion_bn_backward_saved_lengths"], kept_calls
    monkeypatch.setattr(type(be), "FUSION_BN_KEEP_SCORES_WITH_LENGTHS", False)
    again, again_calls = run()
    assert again_calls == ["mcp_fusion_bn_forward_lengths", "mcp_fusion_bn_backward_lengths"], again_calls
    assert len(kept) == 4 + 14
    for name, a, b in zip(["out", "bn", "var", "count"] + list(br.LEAVES), kept, again):
        assert torch.isfinite(a).all() and torch.equal(a, b), f"{name}: the two settings of the switch give other bits"
