"""-m gpu: the training forward (kept log-sum-exp, in-kernel dropout) and the hand-written backward of the wide-head attention
(head widths 32 / 64 / 256: csrc/attention_wide_grad.hip) behind HipBackend.attention: gradients against float64 autograd over
softmax(q k^T scale) v, with and without the dropout mask (rebuilt here with the kernel's integer arithmetic), bit-reproducibility,
bit identity of the training forward with the inference forward, the autograd graph (no RecomputeFn node, no library attention in a
training step any more) and the C ABI's error contract.

Bound on every gradient: max|hip - f64| <= 1e-4 max|f64| + 1e-6, the project's bound for the narrow-head kernels
(tests/test_grad_gpu.py).  The gradients of the unfused twin (grad.attention_twin: what these widths differentiated before) are printed
beside the kernel's for comparison and not asserted on."""
import ctypes

import pytest
import torch

from mocopci_amd import _lib, grad, ops, synth, training
from tests import harness_checks as hc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M32 = 0xFFFFFFFF


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


def keep_mask(seed, bf, heads, nq, nk, p):
    """The kernels' mask in torch: a hash of (seed, row = (bf * heads + head) * nq + query, key) -> (bf, heads, nq, nk) bool."""
    row = torch.arange(bf * heads * nq, device=DEV, dtype=torch.int64).view(bf, heads, nq, 1)
    key = torch.arange(nk, device=DEV, dtype=torch.int64).view(1, 1, 1, nk)
    x = (seed ^ ((row * 0x9E3779B1) & M32) ^ ((key * 0x85EBCA77) & M32)) & M32
    x = x ^ (x >> 16); x = (x * 0x7FEB352D) & M32; x = x ^ (x >> 15); x = (x * 0x846CA68B) & M32; x = x ^ (x >> 16)
    return x >= int(p * 4294967296.0)


def dense(a, b, heads, keep=None):
    """softmax(q k^T scale) (* keep) v per head in the dtype of the inputs; keep (bf, heads, nq, nk) already scaled by 1 / (1 - p)."""
    bf, nq, C = a.shape
    nk, hd = b.shape[1], C // heads
    qh = a.reshape(bf, nq, heads, hd).permute(0, 2, 1, 3)
    kvh = b.reshape(bf, nk, 2, heads, hd).permute(2, 0, 3, 1, 4)
    p = torch.softmax(qh @ kvh[0].transpose(-2, -1) * hd ** -0.5, dim=-1)
    if keep is not None:
        p = p * keep
    return (p @ kvh[1]).permute(0, 2, 1, 3).reshape(bf, nq, C)


def check_grads(tag, got, want, twin=None):
    failures = []
    for k, (name, a, b) in enumerate(zip(("q", "kv"), got, want)):
        scale, err = float(b.abs().max()), float((a.double() - b).abs().max())
        line = f"[{tag}] grad {name:2s}: max|f64| {scale:9.3e}  |hip - f64| {err:9.3e}  bound {1e-4 * scale + 1e-6:9.3e}"
        if twin is not None:
            line += f"  |twin - f64| {float((twin[k].double() - b).abs().max()):9.3e}"
        print(line)
        if not torch.isfinite(a).all():
            failures.append(f"grad {name}: not finite")
        if not err <= 1e-4 * scale + 1e-6:
            failures.append(f"grad {name}: max err {err:.2e}, gradient scale {scale:.2e}")
    assert not failures, f"[{tag}] " + "; ".join(failures)


SHAPES = [  # bf, heads, hd, nq, nk, factor on q
    (2, 8, 32, 333, 517, 1.0),        # partial tiles on both sides
    (3, 4, 32, 100, 20, 1.0),         # fewer keys than one tile
    (8, 8, 32, 256, 256, 1.0),        # the CrossAttention of the level-3 EI cross-former
    (2, 4, 64, 130, 100, 1.0),        # nk % 64 != 0
    (1, 2, 64, 130, 1000, 1.0),       # long key axis
    (16, 3, 256, 256, 256, 1.0),      # Cross_Frame_Att in the training step: the forward splits the keys
    (2, 3, 256, 130, 100, 1.0),       # fewer than 128 keys: the forward's query-stationary form
    (8, 4, 256, 1024, 300, 1.0),      # enough workgroups to cover the chip: the query-stationary form again
    (2, 3, 256, 200, 333, 4.0),       # large logits (about 18 at the maximum)
]


@pytest.mark.parametrize("bf,heads,hd,nq,nk,qf", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{s[3]}q-{s[4]}k" + ("-large-logits" if s[5] != 1.0 else "") for s in SHAPES])
def test_wide_attention_gradients_match_float64_and_repeat(bf, heads, hd, nq, nk, qf):
    be = ops.backend()
    C = heads * hd
    q, kv, g = (rnd(300, bf, nq, C) * qf).to(DEV), rnd(301, bf, nk, 2 * C).to(DEV), rnd(302, bf, nq, C).to(DEV)

    def grads(fn, dt):
        leaves = [t.detach().to(dt).clone().requires_grad_(True) for t in (q, kv)]
        return torch.autograd.grad(fn(*leaves), leaves, g.to(dt))
    hip = grads(lambda a, b: be.attention(a, b, heads), torch.float32)
    again = grads(lambda a, b: be.attention(a, b, heads), torch.float32)
    twin = grads(lambda a, b: grad.run(be._attention, grad.attention_twin, a, b, heads, hd ** -0.5), torch.float32)
    want = grads(lambda a, b: dense(a, b, heads), torch.float64)
    if qf != 1.0:
        logits = (q.double().reshape(bf, nq, heads, hd).permute(0, 2, 1, 3) @ kv.double().reshape(bf, nk, 2, heads, hd)[:, :, 0].permute(0, 2, 3, 1)) * hd ** -0.5
        print(f"\nlargest logit {float(logits.max()):.1f}")
        assert float(logits.max()) > 12.0
    print()
    for name, a, a2 in zip(("q", "kv"), hip, again):
        assert torch.equal(a, a2), f"grad {name}: two runs differ"
    check_grads(f"{bf}x{heads}x{hd} nq={nq} nk={nk}", hip, want, twin)


@pytest.mark.parametrize("bf,heads,hd,nq,nk,p", [(2, 8, 32, 333, 517, 0.25), (1, 2, 64, 130, 1000, 0.25), (16, 3, 256, 256, 256, 0.05)],
                         ids=["hd32", "hd64", "hd256-training-shape"])
def test_wide_attention_dropout_matches_the_dense_formulation_under_the_same_mask(bf, heads, hd, nq, nk, p):
    be = ops.backend()
    C, seed = heads * hd, 123457
    q, kv, g = rnd(310, bf, nq, C).to(DEV), rnd(311, bf, nk, 2 * C).to(DEV), rnd(312, bf, nq, C).to(DEV)
    kept = keep_mask(seed, bf, heads, nq, nk, p)
    frac = float(kept.double().mean())
    print(f"\nkept fraction {frac:.4f} at p = {p}")
    assert abs(frac - (1.0 - p)) < 5e-3
    keep = kept.double() / (1.0 - p)
    l64 = [t.detach().double().clone().requires_grad_(True) for t in (q, kv)]
    want_out = dense(*l64, heads, keep)
    want = torch.autograd.grad(want_out, l64, g.double())
    l32 = [t.detach().clone().requires_grad_(True) for t in (q, kv)]
    out = ops._AttentionWideFn.apply(be, l32[0], l32[1], heads, hd ** -0.5, p, seed)
    got = torch.autograd.grad(out, l32, g)
    out2 = ops._AttentionWideFn.apply(be, l32[0], l32[1], heads, hd ** -0.5, p, seed)
    got2 = torch.autograd.grad(out2, l32, g)
    print(f"output: max|f64| {float(want_out.detach().abs().max()):.3e}  |hip - f64| {float((out.detach().double() - want_out.detach()).abs().max()):.3e}")
    torch.testing.assert_close(out.double(), want_out.detach(), rtol=1e-4, atol=1e-5)
    check_grads(f"dropout {bf}x{heads}x{hd} p={p}", got, want)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(got, got2))


def test_no_gradient_leaks_through_dropped_entries_and_the_public_call_follows_the_torch_seed():
    be = ops.backend()
    # a high rate on a few queries: many keys are dropped by every query; their rows of dV are exactly zero
    hd, nq, nk, p, seed = 32, 8, 200, 0.9, 99
    q, kv, g = rnd(320, 1, nq, hd).to(DEV), rnd(321, 1, nk, 2 * hd).to(DEV), rnd(322, 1, nq, hd).to(DEV)
    kept = keep_mask(seed, 1, 1, nq, nk, p)
    dead = ~kept.any(dim=2).view(nk)
    print(f"\nkeys dropped by all {nq} queries: {int(dead.sum())} of {nk}")
    assert int(dead.sum()) >= 1
    l64 = [t.detach().double().clone().requires_grad_(True) for t in (q, kv)]
    want = torch.autograd.grad(dense(*l64, 1, kept.double() / (1.0 - p)), l64, g.double())
    l32 = [t.detach().clone().requires_grad_(True) for t in (q, kv)]
    got = torch.autograd.grad(ops._AttentionWideFn.apply(be, l32[0], l32[1], 1, hd ** -0.5, p, seed), l32, g)
    check_grads("p = 0.9", got, want)
    assert bool((want[1][0, dead, hd:] == 0.0).all())
    assert bool((got[1][0, dead, hd:] == 0.0).all())
    assert float(got[1][0, ~dead, hd:].abs().max()) > 0.0
    # through the public entry (this raised for wide heads before): reproducible under torch.manual_seed, different across seeds
    for heads, w in ((8, 32), (4, 64), (3, 256)):
        C = heads * w
        q, kv = rnd(323, 2, 300, C).to(DEV), rnd(324, 2, 260, 2 * C).to(DEV)
        torch.manual_seed(5); o1 = be.attention(q, kv, heads, dropout_p=0.25)
        torch.manual_seed(5); o2 = be.attention(q, kv, heads, dropout_p=0.25)
        torch.manual_seed(6); o3 = be.attention(q, kv, heads, dropout_p=0.25)
        assert torch.equal(o1, o2) and not torch.equal(o1, o3), w
        ql, kvl = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        torch.manual_seed(5); o4 = be.attention(ql, kvl, heads, dropout_p=0.25)     # the training forward draws the same mask
        assert torch.equal(o4.detach(), o1), w


@pytest.mark.parametrize("bf,heads,hd,nq,nk", [(2, 8, 32, 301, 450), (2, 4, 64, 130, 100), (2, 3, 256, 130, 100), (16, 3, 256, 256, 256)],
                         ids=["hd32", "hd64", "hd256-query-stationary", "hd256-key-split"])
def test_the_training_forward_is_the_inference_forward(bf, heads, hd, nq, nk):
    """mcp_attention_wide_lse at drop_p = 0: the output of mcp_attention_wide bit for bit on every dispatch branch; lse against float64;
    with a mask: the output of mcp_attention_wide_dropout bit for bit."""
    lib, be = _lib.load(), ops.backend()
    C, scale = heads * hd, hd ** -0.5
    q, kv = rnd(500, bf, nq, C).to(DEV), rnd(501, bf, nk, 2 * C).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    Pk, Pv = ctypes.c_void_p(kv.data_ptr()), ctypes.c_void_p(kv.data_ptr() + 4 * C)
    out, lse = torch.empty_like(q), torch.empty(bf, heads, nq, device=DEV)
    assert lib.mcp_attention_wide_lse(bf, nq, nk, heads, hd, P(q), C, Pk, 2 * C, Pv, 2 * C, scale, 0.0, 0, P(out), P(lse), st) == 0
    assert torch.equal(out, be._attention(q, kv, heads, scale))
    qh = q.double().reshape(bf, nq, heads, hd).permute(0, 2, 1, 3)
    kh = kv.double().reshape(bf, nk, 2, heads, hd)[:, :, 0].permute(0, 2, 1, 3)
    want = torch.logsumexp(qh @ kh.transpose(-2, -1) * scale, dim=-1) / 0.6931471805599453      # log2 domain
    print(f"\nlse: max|f64| {float(want.abs().max()):.3e}  |hip - f64| {float((lse.double() - want).abs().max()):.3e}")
    torch.testing.assert_close(lse.double(), want, rtol=1e-5, atol=1e-5)
    ql, kvl = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    assert torch.equal(be.attention(ql, kvl, heads).detach(), out)            # the public call in a training graph
    out_d, lse_d, ref = torch.empty_like(q), torch.empty_like(lse), torch.empty_like(q)
    assert lib.mcp_attention_wide_lse(bf, nq, nk, heads, hd, P(q), C, Pk, 2 * C, Pv, 2 * C, scale, 0.25, 4242, P(out_d), P(lse_d), st) == 0
    assert lib.mcp_attention_wide_dropout(bf, nq, nk, heads, hd, P(q), C, Pk, 2 * C, Pv, 2 * C, scale, 0.25, 4242, P(ref), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out_d, ref) and not torch.equal(out_d, out)
    assert torch.equal(lse_d, lse)                                             # row sums are taken before the mask


@pytest.mark.parametrize("heads,hd", [(8, 32), (4, 64), (3, 256)])
def test_wide_attention_has_no_recompute_node(heads, hd):
    be = ops.backend()
    C = heads * hd
    q, kv = rnd(600, 2, 200, C).to(DEV).requires_grad_(True), rnd(601, 2, 150, 2 * C).to(DEV).requires_grad_(True)
    names = graph_nodes(be.attention(q, kv, heads))
    assert "_AttentionWideFnBackward" in names and "RecomputeFnBackward" not in names, names


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_a_training_step_calls_no_library_attention(mode, monkeypatch):
    """net.train() with the reference's dropout rates, and the inference graph differentiated (net.eval(), train=True): one forward +
    loss + backward with F.scaled_dot_product_attention replaced by a function that raises."""
    def refuse(*a, **k):
        raise AssertionError("library attention called in a training step")
    x1, x2, gt = synth.make_batch(1, 1, 1024, device=DEV)
    gtc = [t.transpose(1, 2).contiguous() for t in gt]
    net = hc.build_model(DEV)
    if mode == "train":
        net.train()
        assert (net.drop_rate, net.attn_drop_rate, net.drop_path_rate) == (0.05, 0.05, 0.04)
    else:
        net.eval()
    monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention", refuse)
    torch.manual_seed(3)
    out = net(x1, x2, gtc, None, True)
    loss, _ = training.multiscale_loss(*out, gtc)
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert len(grads) >= 280 and all(torch.isfinite(t).all() for t in grads)


def test_wide_attention_entry_points_reject_bad_arguments_and_handle_one_token():
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    assert lib.mcp_attention_wide_grad_workspace_bytes(2, 100, 77, 8, 32) == 2 * 8 * 100 * 4
    for bad in ((0, 100, 77, 8, 32), (2, -1, 77, 8, 32), (2, 100, 0, 8, 32), (2, 100, 77, 0, 32), (2, 100, 77, 8, 0)):
        assert lib.mcp_attention_wide_grad_workspace_bytes(*bad) == 0, bad
    heads, hd, n = 2, 32, 64
    C = heads * hd
    q, kv = torch.zeros(1, n, C, device=DEV), torch.zeros(1, n, 2 * C, device=DEV)
    out, lse, dq, dkv = torch.full((1, n, C), 7.0, device=DEV), torch.full((1, heads, n), 7.0, device=DEV), torch.full((1, n, C), 7.0, device=DEV), torch.full((1, n, 2 * C), 7.0, device=DEV)
    need = lib.mcp_attention_wide_grad_workspace_bytes(1, n, n, heads, hd)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def fwd(hd_=hd, qs=C, p=0.0, qp=None, lsep=True, name="mcp_attention_wide_lse"):
        return getattr(lib, name)(1, n, n, heads, hd_, P(q) if qp is None else qp, qs, P(kv), 2 * C, P(kv, 4 * C), 2 * C, 1.0, p, 0, P(out), P(lse) if lsep else None, st)

    def bwd(hd_=hd, qs=C, p=0.0, qp=None, wsb=need, dqp=True, name="mcp_attention_wide_grad_lse"):
        return getattr(lib, name)(1, n, n, heads, hd_, P(q) if qp is None else qp, qs, P(kv), 2 * C, P(kv, 4 * C), 2 * C, 1.0, p, 0, P(out), P(out), P(lse),
                                  P(dq) if dqp else None, P(dkv), P(ws), wsb, st)
    for f in (fwd, bwd):
        assert f(hd_=48) == 10002                    # MCP_ERR_UNSUPPORTED: head widths 32 / 64 / 256
        assert f(hd_=16) == 10002
        assert f(p=1.5) == 10001                     # MCP_ERR_BAD_ARG: drop_p outside [0, 1)
        assert f(p=-0.1) == 10001
        assert f(qs=C + 2) == 10001                  # stride not a multiple of 4
        assert f(qp=P(q, 4)) == 10001                # pointer not 16-byte aligned
        assert f(qp=ctypes.c_void_p(0)) == 10001     # null pointer
    assert fwd(lsep=False) == 10001
    assert bwd(wsb=need - 1) == 10001                # workspace one byte short
    assert bwd(dqp=False) == 10001
    # the narrow entries keep refusing wide heads
    assert fwd(name="mcp_attention_small_lse") == 10002 and bwd(name="mcp_attention_small_grad_lse") == 10002
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (out, lse, dq, dkv)) and not bool(ws.any())   # nothing ran
    assert lib.mcp_attention_wide_dropout(1, n, n, heads, hd, P(q), C, P(kv), 2 * C, P(kv, 4 * C), 2 * C, 1.0, 0.0, 0, P(out), st) == 0
    # one query, one key: the softmax is 1, out = v, dQ = dK = 0, dV = dO
    q1, kv1, g1 = rnd(700, 1, 1, 32).to(DEV), rnd(701, 1, 1, 64).to(DEV), rnd(702, 1, 1, 32).to(DEV)
    o1, l1, dq1, dkv1 = torch.empty_like(q1), torch.empty(1, 1, 1, device=DEV), torch.full_like(q1, 7.0), torch.full_like(kv1, 7.0)
    w1 = torch.empty(lib.mcp_attention_wide_grad_workspace_bytes(1, 1, 1, 1, 32), dtype=torch.uint8, device=DEV)
    assert lib.mcp_attention_wide_lse(1, 1, 1, 1, 32, P(q1), 32, P(kv1), 64, P(kv1, 128), 64, 32 ** -0.5, 0.0, 0, P(o1), P(l1), st) == 0
    assert lib.mcp_attention_wide_grad_lse(1, 1, 1, 1, 32, P(q1), 32, P(kv1), 64, P(kv1, 128), 64, 32 ** -0.5, 0.0, 0, P(o1), P(g1), P(l1), P(dq1), P(dkv1),
                                           P(w1), w1.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(o1, kv1[:, :, 32:])
    # at this width both backward kernels form s with the forward's products in the forward's order, so p = exp2(s - L) = 1 exactly and
    # dV = dO bit for bit; ds = p (dP - D) subtracts two fp32 sums of the same 32 products taken in different orders (an MFMA chain, a
    # lane butterfly): zero to a few ulp of a sum of 32 products of unit normals (1e-6), hence |dQ|, |dK| <= 1e-5
    print(f"\none token: max|dQ| {float(dq1.abs().max()):.2e}  max|dK| {float(dkv1[:, :, :32].abs().max()):.2e}  max|dV - dO| {float((dkv1[:, :, 32:] - g1).abs().max()):.2e}")
    assert float(dq1.abs().max()) <= 1e-5 and float(dkv1[:, :, :32].abs().max()) <= 1e-5
    assert torch.equal(dkv1[:, :, 32:], g1)
