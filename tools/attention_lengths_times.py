"""What per-element lengths cost the attention kernels, and what a half-empty batch saves: the plain C entry points against their
length forms (mcp_attention vs mcp_attention_lengths; mcp_attention_{small,wide}_lse vs ..._lse_lengths; ..._grad_lse vs
..._grad_lse_lengths) on preallocated buffers, at full lengths and at lengths of half the padded size.  One process, plain and length
form alternating, warm, medians of `--reps` (25) timed intervals of back-to-back launches between device events, per-launch time
reported.  The plain call of the same process is the yardstick; no threshold is asserted.

Shapes: the attention calls of a traced step -- 8 x 8 heads x 256 x 256 at head width 32, 32 x 3 x 256 x 256 at
width 256 -- and 40 x 8 x 2048 x 2048 at width 8.  Prints one JSON line per shape and pass; `--out FILE` appends them there too."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import _lib  # noqa: E402

# (layer, bf, heads, head width, nq, nk, launches per timed interval)
SHAPES = [("ei3 CrossAttention", 8, 8, 32, 256, 256, 20), ("cross_block3 (Cross_Frame_Att), both directions in one call", 32, 3, 256, 256, 256, 20),
          ("InterFrameAttention at 2048 tokens", 40, 8, 8, 2048, 2048, 2)]


def rnd(seed, *shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)).cuda()


def timed_ms(fn):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alternate(calls, launches, reps):
    """{name: (median, [min, max])} in ms per launch of each call, the calls taking turns."""
    def interval(call):
        def run():
            for _ in range(launches):
                assert call() == 0
        return timed_ms(run) / launches
    for _ in range(2):   # warm: code objects, the kernels' LDS attribute
        for call in calls.values():
            interval(call)
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            times[name].append(interval(call))
    return {name: (round(sorted(v)[len(v) // 2], 4), [round(min(v), 4), round(max(v), 4)]) for name, v in times.items()}


def measure(layer, bf, heads, hd, nq, nk, launches, reps):
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    C, scale = heads * hd, hd ** -0.5
    fam = "small" if hd in (8, 16) else "wide"
    q, kv, g = rnd(1, bf, nq, C), rnd(2, bf, nk, 2 * C), rnd(3, bf, nq, C)
    out, lse = torch.empty_like(q), torch.empty(bf, heads, nq, device="cuda")
    gq, gkv = torch.empty_like(q), torch.empty_like(kv)
    need = lib.mcp_attention_small_grad_workspace_bytes(bf, nq, heads) if fam == "small" else lib.mcp_attention_wide_grad_workspace_bytes(bf, nq, nk, heads, hd)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    lens = {"full": (torch.full((bf,), nq, dtype=torch.int32, device="cuda"), torch.full((bf,), nk, dtype=torch.int32, device="cuda")),
            "half": (torch.full((bf,), nq // 2, dtype=torch.int32, device="cuda"), torch.full((bf,), nk // 2, dtype=torch.int32, device="cuda"))}
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    qkv = (bf, nq, nk, heads, hd, P(q), C, P(kv), 2 * C, P(kv, 4 * C), 2 * C)
    f_lse, f_lse_len = getattr(lib, f"mcp_attention_{fam}_lse"), getattr(lib, f"mcp_attention_{fam}_lse_lengths")
    f_bwd, f_bwd_len = getattr(lib, f"mcp_attention_{fam}_grad_lse"), getattr(lib, f"mcp_attention_{fam}_grad_lse_lengths")
    passes = {
        "inference forward": {"plain": lambda: lib.mcp_attention(*qkv, 0, scale, P(out), C, st),
                              **{k: (lambda a=a, b=b: lib.mcp_attention_lengths(*qkv, 0, scale, P(a), P(b), P(out), C, st)) for k, (a, b) in lens.items()}},
        "training forward": {"plain": lambda: f_lse(*qkv, scale, 0.0, 0, P(out), P(lse), st),
                             **{k: (lambda a=a, b=b: f_lse_len(*qkv, scale, 0.0, 0, P(out), P(lse), P(a), P(b), st)) for k, (a, b) in lens.items()}},
    }
    rows = []
    base = {"layer": layer, "bf": bf, "heads": heads, "hd": hd, "nq": nq, "nk": nk, "reps": reps, "launches_per_interval": launches}

    def report(what, res):
        plain = res["plain"][0]
        rows.append({**base, "what": what, **{f"{k}_ms": v[0] for k, v in res.items()}, **{f"{k}_min_max_ms": v[1] for k, v in res.items()},
                     "full_over_plain": round(res["full"][0] / plain, 4), "half_over_plain": round(res["half"][0] / plain, 4)})
    for what, calls in passes.items():
        report(what, alternate(calls, launches, reps))
    # the backward reads the forward's out / lse: a forward per length setting in front of its timed backward calls
    assert f_lse(*qkv, scale, 0.0, 0, P(out), P(lse), st) == 0
    half_out, half_lse = torch.empty_like(out), torch.empty_like(lse)
    assert f_lse_len(*qkv, scale, 0.0, 0, P(half_out), P(half_lse), P(lens["half"][0]), P(lens["half"][1]), st) == 0
    bwd = {"plain": lambda: f_bwd(*qkv, scale, 0.0, 0, P(out), P(g), P(lse), P(gq), P(gkv), P(ws), need, st),
           "full": lambda: f_bwd_len(*qkv, scale, 0.0, 0, P(out), P(g), P(lse), P(gq), P(gkv), P(ws), need, P(lens["full"][0]), P(lens["full"][1]), st),
           "half": lambda: f_bwd_len(*qkv, scale, 0.0, 0, P(half_out), P(g), P(half_lse), P(gq), P(gkv), P(ws), need, P(lens["half"][0]), P(lens["half"][1]), st)}
    report("backward", alternate(bwd, max(1, launches // 2), reps))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev, lines = torch.cuda.get_device_name(0), []
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
