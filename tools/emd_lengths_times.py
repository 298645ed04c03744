"""Device times of the length-aware EMD forward / backward against the length-free calls (device events after warm-up).

B = 8, N = M = 8192, the cube [0, 4]^3 of the tests.  In one process, alternating per repetition:
    mcp_emd       |  mcp_emd_lengths with every length full       |  mcp_emd_lengths with every length at N / 2
    mcp_emd_grad  |  mcp_emd_grad_lengths with every length full  |  mcp_emd_grad_lengths with every length at N / 2
(each backward on the levels its own level-keeping forward wrote).  Medians of --reps (15) single calls with min and max.
Expectations evaluated and recorded with the numbers:
  * full lengths do the same arithmetic plus two loads and a few bounds per workgroup: the median should sit within
    max(10 %, the length-free call's own (max - min) / median) of the length-free median;
  * halved lengths skip the padded workgroups and tiles (not mask them): the median should be below the full-length one by more
    than that spread (recorded as the ratio).
The full-length results are also compared with the length-free ones bit for bit.

--parent LIB: additionally times mcp_emd, mcp_emd_keep and mcp_emd_grad of another build of the library (the parent commit's) and
of this one, in fresh processes in the order parent, new, parent, new (each child loads its library through MCP_HIP_LIB and binds
only those three entry points), and holds the new medians to the same margin.
Prints one JSON document; `--out FILE` writes it there."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mocopci_amd import _lib  # noqa: E402

B, N = 8, 8192
PLAIN = ("mcp_emd", "mcp_emd_keep", "mcp_emd_grad")


def timed(fn):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def alternate(runs, reps):
    for _ in range(2):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(reps):
        for name, fn in runs.items():
            times[name].append(timed(fn))
    return {name: stats(v) for name, v in times.items()}


def clouds():
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(B, N, 3, generator=gen) * 4
    y = x[:, torch.randperm(N, generator=gen)] + 0.3 * torch.randn(B, N, 3, generator=gen)
    return x.cuda().contiguous(), y.cuda().contiguous()


def buffers(x):
    dev = x.device
    return (torch.empty(B, device=dev), torch.empty(B * 5 * N, device=dev), torch.empty(B * 10 * 2 * N, device=dev),
            torch.linspace(0.5, 2.0, B, device=dev), torch.empty_like(x), torch.empty_like(x))


def judge(r, base, full, half):
    spread = (r[base]["max_ms"] - r[base]["min_ms"]) / r[base]["median_ms"]
    r["spread_of_" + base] = round(spread, 4)
    r["full_over_" + base] = round(r[full]["median_ms"] / r[base]["median_ms"], 4)
    r["allowed_full_over_" + base] = round(1 + max(0.10, spread), 4)
    r["full_within_expectation"] = r["full_over_" + base] <= r["allowed_full_over_" + base]
    r["half_over_full"] = round(r[half]["median_ms"] / r[full]["median_ms"], 4)
    r["half_faster_than_full_by_more_than_the_spread"] = r["half_over_full"] < 1 - spread
    return r


def measure(reps):
    lib = _lib.load()
    x, y = clouds()
    p, i, st = _lib.fptr, _lib.iptr, _lib.stream
    full = torch.full((B,), N, dtype=torch.int32, device=x.device)
    half = torch.full((B,), N // 2, dtype=torch.int32, device=x.device)
    out = {name: buffers(x) for name in ("plain", "full", "half")}

    def fwd(name, lens):
        cost, ws = out[name][0], out[name][1]
        if lens is None:
            return lambda: _lib.check(lib.mcp_emd(B, N, N, p(x), p(y), None, p(cost), p(ws), st()))
        return lambda: _lib.check(lib.mcp_emd_lengths(B, N, N, p(x), p(y), i(lens), i(lens), None, p(cost), p(ws), st()))

    def keep(name, lens):
        cost, ws, levels = out[name][:3]
        if lens is None:
            _lib.check(lib.mcp_emd_keep(B, N, N, p(x), p(y), p(cost), p(levels), p(ws), st()))
        else:
            _lib.check(lib.mcp_emd_keep_lengths(B, N, N, p(x), p(y), i(lens), i(lens), p(cost), p(levels), p(ws), st()))

    def bwd(name, lens):
        _, _, levels, g, g1, g2 = out[name]
        if lens is None:
            return lambda: _lib.check(lib.mcp_emd_grad(B, N, N, p(g), p(x), p(y), p(levels), p(g1), p(g2), st()))
        return lambda: _lib.check(lib.mcp_emd_grad_lengths(B, N, N, p(g), p(x), p(y), i(lens), i(lens), p(levels), p(g1), p(g2), st()))

    lens = {"plain": None, "full": full, "half": half}
    names = {"plain": "mcp_emd", "full": "lengths_full", "half": "lengths_half"}
    forward = alternate({names[k]: fwd(k, v) for k, v in lens.items()}, reps)
    forward["full_lengths_bits_equal_mcp_emd"] = bool(torch.equal(out["plain"][0], out["full"][0]))
    for k, v in lens.items():
        keep(k, v)
    names = {"plain": "mcp_emd_grad", "full": "lengths_full", "half": "lengths_half"}
    backward = alternate({names[k]: bwd(k, v) for k, v in lens.items()}, reps)
    backward["full_lengths_bits_equal_mcp_emd_grad"] = bool(torch.equal(out["plain"][4], out["full"][4])
                                                            and torch.equal(out["plain"][5], out["full"][5]))
    backward["half_lengths_padded_rows_zero"] = bool(int(torch.count_nonzero(out["half"][4][:, N // 2:])) == 0
                                                     and int(torch.count_nonzero(out["half"][5][:, N // 2:])) == 0)
    return {"forward": judge(forward, "mcp_emd", "lengths_full", "lengths_half"),
            "backward": judge(backward, "mcp_emd_grad", "lengths_full", "lengths_half")}


def child(reps):
    """The three length-free entry points of whichever library MCP_HIP_LIB names, bound directly: an older build has no more."""
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in PLAIN:
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    x, y = clouds()
    cost, ws, levels, g, g1, g2 = buffers(x)
    p, st = _lib.fptr, _lib.stream

    def ok(rc):
        assert rc == 0, rc

    runs = {"mcp_emd": lambda: ok(lib.mcp_emd(B, N, N, p(x), p(y), None, p(cost), p(ws), st())),
            "mcp_emd_keep": lambda: ok(lib.mcp_emd_keep(B, N, N, p(x), p(y), p(cost), p(levels), p(ws), st())),
            "mcp_emd_grad": lambda: ok(lib.mcp_emd_grad(B, N, N, p(g), p(x), p(y), p(levels), p(g1), p(g2), st()))}
    r = alternate(runs, reps)
    r["cost_sum"] = float(cost.double().sum())
    r["grad_abs_sum"] = float(g1.double().abs().sum() + g2.double().abs().sum())
    print(json.dumps(r), flush=True)


def against_parent(parent, reps):
    new = os.path.join(ROOT, "mocopci_amd", "libmocopci_hip.so")
    runs = []
    for tag, path in (("parent", parent), ("new", new), ("parent", parent), ("new", new)):
        env = dict(os.environ, MCP_HIP_LIB=os.path.abspath(path))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True,
                             text=True, timeout=300)
        if res.returncode != 0:
            raise RuntimeError(f"{tag} run failed ({res.returncode}): {res.stderr[-2000:]}")
        runs.append(dict(json.loads(res.stdout.strip().splitlines()[-1]), library=tag))
    doc = {"order": [r["library"] for r in runs], "runs": runs}
    for name in PLAIN:
        med = {t: [r[name]["median_ms"] for r in runs if r["library"] == t] for t in ("parent", "new")}
        spread = max((r[name]["max_ms"] - r[name]["min_ms"]) / r[name]["median_ms"] for r in runs if r["library"] == "parent")
        ratio = (sum(med["new"]) / len(med["new"])) / (sum(med["parent"]) / len(med["parent"]))
        doc[name] = {"parent_median_ms": med["parent"], "new_median_ms": med["new"], "new_over_parent": round(ratio, 4),
                     "allowed_new_over_parent": round(1 + max(0.10, spread), 4), "within_expectation": ratio <= 1 + max(0.10, spread)}
    doc["same_results"] = all(r["cost_sum"] == runs[0]["cost_sum"] and r["grad_abs_sum"] == runs[0]["grad_abs_sum"] for r in runs)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--parent", default=None, help="another build of libmocopci_hip.so to compare the length-free calls with")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    doc = {"B": B, "N": N, "M": N, "reps": a.reps}
    if a.parent:
        doc["against_parent"] = against_parent(a.parent, a.reps)   # before this process opens the GPU
    assert torch.cuda.is_available(), "needs a GPU"
    doc["device"] = torch.cuda.get_device_name(0)
    doc.update(measure(a.reps))
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
