"""Times of the wide-head attention (head widths 32 / 64 / 256) in a training graph: the hand-written backward
(mcp_attention_wide_grad_lse behind ops._AttentionWideFn) against autograd over the unfused twin (grad.run(be._attention,
grad.attention_twin, ...): a second forward through the library's attention plus its backward kernels), and the training forward
that keeps the log-sum-exp (mcp_attention_wide_lse) against the inference forward (mcp_attention_wide).  One process, alternating,
warm, device events around work that ends in a synchronise.  The two forwards are timed as 20 back-to-back launches of the C entry points
on preallocated buffers (per-launch time reported), so that the figure is the kernels' and not the host's.

Shapes: the wide-head calls of a B = 8, N = 8192 training step -- recorded from one traced forward with `--trace` (the calls of
HipBackend.attention with a head width of 32 or more, printed as they come) -- and one shape at head width 64, which no layer of the
model uses.  Each backward repeat builds the forward graph untimed and times only the backward.  Prints one JSON line per shape and
measurement; `--out FILE` appends them there too."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import _lib, grad, ops  # noqa: E402

# (layer, bf, heads, head width, nq, nk)
SHAPES = [("cross_block3 (Cross_Frame_Att), as traced: both directions x 16 in one call", 32, 3, 256, 256, 256), ("cross_block3, one direction", 16, 3, 256, 256, 256),
          ("ei3 CrossAttention (two calls per step)", 8, 8, 32, 256, 256), ("head width 64 (no layer)", 8, 4, 64, 512, 512)]
FORWARD_LAUNCHES = 20   # C-ABI launches per timed interval of the forward comparison: the kernels are 20-100 us, one launch is host-bound


def rnd(seed, *shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)).cuda()


def timed_ms(fn):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alternate(fa, fb, reps):
    for f in (fa, fb, fa, fb):   # warm: code objects, allocator, library algorithm choices
        f()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(fa())
        tb.append(fb())
    med = lambda v: sorted(v)[len(v) // 2]
    r3 = lambda v: round(v, 4)
    return (r3(med(ta)), [r3(min(ta)), r3(max(ta))]), (r3(med(tb)), [r3(min(tb)), r3(max(tb))])


def measure(layer, bf, heads, hd, nq, nk, reps):
    be = ops.backend()
    C, scale = heads * hd, hd ** -0.5
    q, kv, g = rnd(1, bf, nq, C).requires_grad_(True), rnd(2, bf, nk, 2 * C).requires_grad_(True), rnd(3, bf, nq, C)

    def backward_of(forward):
        def run():
            out = forward()
            torch.cuda.synchronize()
            return timed_ms(lambda: torch.autograd.grad(out, (q, kv), g))
        return run
    twin, hip = alternate(backward_of(lambda: grad.run(be._attention, grad.attention_twin, q, kv, heads, scale)),
                          backward_of(lambda: be.attention(q, kv, heads)), reps)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    qd, kvd, out, lse_t = q.detach(), kv.detach(), torch.empty(bf, nq, C, device="cuda"), torch.empty(bf, heads, nq, device="cuda")
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def launches(call):
        def run():
            for _ in range(FORWARD_LAUNCHES):
                assert call() == 0
        return lambda: timed_ms(run) / FORWARD_LAUNCHES
    inf, lse = alternate(launches(lambda: lib.mcp_attention_wide(bf, nq, nk, heads, hd, P(qd), C, P(kvd), 2 * C, P(kvd, 4 * C), 2 * C, scale, P(out), C, st)),
                         launches(lambda: lib.mcp_attention_wide_lse(bf, nq, nk, heads, hd, P(qd), C, P(kvd), 2 * C, P(kvd, 4 * C), 2 * C, scale, 0.0, 0, P(out), P(lse_t), st)),
                         reps)
    base = {"layer": layer, "bf": bf, "heads": heads, "hd": hd, "nq": nq, "nk": nk, "reps": reps}
    return [{**base, "what": "backward", "twin_ms": twin[0], "twin_min_max_ms": twin[1], "hip_ms": hip[0], "hip_min_max_ms": hip[1],
             "twin_over_hip": round(twin[0] / hip[0], 3), "hip_within_twin_spread": hip[0] <= twin[0] + (twin[1][1] - twin[1][0])},
            {**base, "what": "forward", "inference_ms": inf[0], "inference_min_max_ms": inf[1], "with_lse_ms": lse[0], "with_lse_min_max_ms": lse[1],
             "lse_within_inference_spread": lse[0] <= inf[0] + (inf[1][1] - inf[1][0])}]


def trace(batch, npoints):
    """The wide-head attention calls of one training forward (eval graph), in call order."""
    from mocopci_amd import synth
    from mocopci_amd.model import MoCoPCI
    net = MoCoPCI()
    net.load_state_dict(synth.weights_by_name(net._spec), strict=True)
    net = net.cuda().eval()
    x1, x2, gt = synth.make_batch(2, batch, npoints, device="cuda")
    gtc = [t.transpose(1, 2).contiguous() for t in gt]
    seen, be = [], ops.backend()
    inner = be.attention

    def recording(q, kv, heads, **k):
        if q.shape[-1] // heads >= 32:
            seen.append({"bf": q.shape[0], "heads": heads, "hd": q.shape[-1] // heads, "nq": q.shape[1], "nk": kv.shape[1], "wants_grad": grad.wants_grad(q, kv)})
        return inner(q, kv, heads, **k)
    be.attention = recording
    try:
        net(x1, x2, gtc, None, True)
    finally:
        del be.attention
    torch.cuda.synchronize()
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="first record the wide-head calls of one B = 8, N = 8192 training forward")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev, lines = torch.cuda.get_device_name(0), []
    if a.trace:
        lines.append(json.dumps({"what": "traced wide-head calls, B = 8, N = 8192", "calls": trace(8, 8192), "device": dev}))
        print(lines[-1], flush=True)
    for shape in SHAPES:
        for r in measure(*shape, a.reps):
            r["device"] = dev
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
