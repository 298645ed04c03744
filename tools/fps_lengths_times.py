"""Device times of the length-aware furthest point sampling against the length-free fresh sampling (device events after warm-up).

B = 8, m = 2048, at N = 8192 and at N = 2048, on the LiDAR-like box of mocopci_amd.synth (80 x 80 x 6, 5 % exact duplicates).
In one process, alternating per repetition:
    (a) mcp_furthest_point_sampling_fresh  |  (b) mcp_furthest_point_sampling_lengths, every length full  |  (c) ..., every length N / 2
Medians of --reps (15) single calls with min and max, and the ratios b/a and c/b.  (a) is the Morton-pruned kernel from N = 1024
up; the length-aware kernels are the unpruned register-resident form, so b/a above 1 is expected here and is what this tool
records -- it is not held to a margin.  Recorded with the numbers:
  * (b) returns the indices of (a) bit for bit;
  * halved lengths skip whole register slices (not mask them): c/b should sit below 1 by more than (b)'s own spread.

--parent LIB: additionally times mcp_furthest_point_sampling_fresh of another build of the library (the parent commit's) and of this
one, in fresh processes in the order parent, new, parent, new (each child loads its library through MCP_HIP_LIB and binds only that
entry point).  The kernels behind it are unchanged, so the new median should sit within max(10 %, the parent's own
(max - min) / median) of the parent's.
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
from mocopci_amd import _lib, synth  # noqa: E402

B, M = 8, 2048
SIZES = (8192, 2048)
FRESH = "mcp_furthest_point_sampling_fresh"


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


def lidar_cloud(n):
    return synth.make_batch(1, B, n)[0].permute(0, 2, 1).contiguous().cuda()


def measure(n, reps):
    lib = _lib.load()
    xyz = lidar_cloud(n)
    p, i, st = _lib.fptr, _lib.iptr, _lib.stream
    lens = {"full": torch.full((B,), n, dtype=torch.int32, device=xyz.device), "half": torch.full((B,), n // 2, dtype=torch.int32, device=xyz.device)}
    out = {name: torch.empty((B, M), dtype=torch.int32, device=xyz.device) for name in ("fresh", "full", "half")}
    runs = {"fresh": lambda: _lib.check(lib.mcp_furthest_point_sampling_fresh(B, n, M, p(xyz), i(out["fresh"]), None, None, 0, st()))}
    for name in ("full", "half"):
        runs["lengths_" + name] = (lambda name=name: _lib.check(
            lib.mcp_furthest_point_sampling_lengths(B, n, M, p(xyz), i(lens[name]), i(out[name]), None, None, 0, st())))
    r = alternate(runs, reps)
    r["full_lengths_bits_equal_fresh"] = bool(torch.equal(out["fresh"], out["full"]))
    r["half_lengths_stay_below_the_length"] = bool(int(out["half"].max()) < n // 2)
    r["full_over_fresh"] = round(r["lengths_full"]["median_ms"] / r["fresh"]["median_ms"], 4)
    r["half_over_full"] = round(r["lengths_half"]["median_ms"] / r["lengths_full"]["median_ms"], 4)
    spread = (r["lengths_full"]["max_ms"] - r["lengths_full"]["min_ms"]) / r["lengths_full"]["median_ms"]
    r["spread_of_lengths_full"] = round(spread, 4)
    r["half_faster_than_full_by_more_than_the_spread"] = r["half_over_full"] < 1 - spread
    return r


def child(reps):
    """The length-free entry point of whichever library MCP_HIP_LIB names, bound directly: an older build has no more."""
    lib = ctypes.CDLL(_lib.SO_PATH)
    getattr(lib, FRESH).argtypes = _lib.SIGNATURES[FRESH]
    getattr(lib, FRESH).restype = ctypes.c_int
    p, i, st = _lib.fptr, _lib.iptr, _lib.stream
    doc = {}
    for n in SIZES:
        xyz = lidar_cloud(n)
        idx = torch.empty((B, M), dtype=torch.int32, device=xyz.device)

        def run():
            rc = getattr(lib, FRESH)(B, n, M, p(xyz), i(idx), None, None, 0, st())
            assert rc == 0, rc

        doc[str(n)] = dict(alternate({FRESH: run}, reps)[FRESH], index_sum=int(idx.long().sum()))
    print(json.dumps(doc), flush=True)


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
    for n in map(str, SIZES):
        med = {t: [r[n]["median_ms"] for r in runs if r["library"] == t] for t in ("parent", "new")}
        spread = max((r[n]["max_ms"] - r[n]["min_ms"]) / r[n]["median_ms"] for r in runs if r["library"] == "parent")
        ratio = (sum(med["new"]) / len(med["new"])) / (sum(med["parent"]) / len(med["parent"]))
        doc[n] = {"parent_median_ms": med["parent"], "new_median_ms": med["new"], "new_over_parent": round(ratio, 4),
                  "allowed_new_over_parent": round(1 + max(0.10, spread), 4), "within_expectation": ratio <= 1 + max(0.10, spread),
                  "same_results": all(r[n]["index_sum"] == runs[0][n]["index_sum"] for r in runs)}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--parent", default=None, help="another build of libmocopci_hip.so to compare the length-free call with")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    doc = {"B": B, "m": M, "N": list(SIZES), "reps": a.reps}
    if a.parent:
        doc["against_parent"] = against_parent(a.parent, a.reps)   # before this process opens the GPU
    assert torch.cuda.is_available(), "needs a GPU"
    doc["device"] = torch.cuda.get_device_name(0)
    for n in SIZES:
        doc[str(n)] = measure(n, a.reps)
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
