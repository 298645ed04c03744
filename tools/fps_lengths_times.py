"""Device times of the length-aware furthest point sampling, pruned and unpruned, against the length-free fresh sampling (device
events after warm-up).

B = 8 on the LiDAR-like box of mocopci_amd.synth (80 x 80 x 6, 5 % exact duplicates), at (N, m) = (2048, 512), (8192, 2048),
(16384, 2048) and (65536, 2048).  In one process, alternating per repetition, single launches:
    (a) mcp_furthest_point_sampling_fresh
    (b) mcp_furthest_point_sampling_lengths_unpruned, every length full     (resident up to 16384, streaming beyond)
    (c) mcp_furthest_point_sampling_lengths, every length full              (the form mcp_fps_lengths_form names: spatial / tiled)
    (d) mcp_furthest_point_sampling_lengths, every length N / 2
    (e) mcp_furthest_point_sampling_lengths_unpruned, every length N / 2
Medians of --reps (15) calls with min and max.  Every call gets the workspace its own query asks for.  Recorded with the numbers:
  * (b) and (c) return the indices of (a) bit for bit, (d) those of (e);
  * c/a against max(1.10, (a)'s own (max - min) / median): the allowance for full lengths against the length-free kernel;
  * c < b and d < e: the pruned form has to win in every shape class the dispatch sends to it, or the class goes back.

--parent LIB: additionally times mcp_furthest_point_sampling_fresh of another build of the library (the parent commit's) and of this
one, in fresh processes in the order parent, new, parent, new (each child loads its library through MCP_HIP_LIB and binds only the
entry points it calls).  The kernels behind it are unchanged, so the new median should sit within max(10 %, the parent's own
(max - min) / median) of the parent's.  --parent-root DIR --bench N: also runs the default `python bench.py` line N times in a
checkout of the parent commit (DIR, library built) and N times in this one, alternated (parent first); the new median must be no lower than the parent's median minus the parent's spread (max - min).  --parent-out FILE
writes that comparison on its own.
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

B = 8
SHAPES = ((2048, 512), (8192, 2048), (16384, 2048), (65536, 2048))
FRESH, FRESH_WS = "mcp_furthest_point_sampling_fresh", "mcp_fps_workspace_bytes"
PRUNED, UNPRUNED = "mcp_furthest_point_sampling_lengths", "mcp_furthest_point_sampling_lengths_unpruned"
FORMS = {0: "resident", 1: "spatial", 2: "tiled", 3: "streaming"}


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


def scratch(nbytes, device):
    return torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=device)


def measure(n, m, reps):
    lib = _lib.load()
    xyz = lidar_cloud(n)
    dev = xyz.device
    p, i, st = _lib.fptr, _lib.iptr, _lib.stream
    lens = {"full": torch.full((B,), n, dtype=torch.int32, device=dev), "half": torch.full((B,), n // 2, dtype=torch.int32, device=dev)}
    need = {"fresh": lib.mcp_fps_workspace_bytes(B, n, m), UNPRUNED: lib.mcp_fps_lengths_workspace_bytes(B, n, m),
            PRUNED: lib.mcp_fps_lengths_pruned_workspace_bytes(B, n, m)}
    ws = {k: scratch(v, dev) for k, v in need.items()}
    rows = {"a_fresh": None, "b_unpruned_full": (UNPRUNED, "full"), "c_pruned_full": (PRUNED, "full"), "d_pruned_half": (PRUNED, "half"),
            "e_unpruned_half": (UNPRUNED, "half")}
    out = {name: torch.empty((B, m), dtype=torch.int32, device=dev) for name in rows}
    runs = {"a_fresh": lambda: _lib.check(lib.mcp_furthest_point_sampling_fresh(B, n, m, p(xyz), i(out["a_fresh"]), None, ws["fresh"].data_ptr(),
                                                                                need["fresh"], st()))}
    for name, spec in rows.items():
        if spec:
            runs[name] = (lambda name=name, entry=spec[0], which=spec[1]: _lib.check(
                getattr(lib, entry)(B, n, m, p(xyz), i(lens[which]), i(out[name]), None, ws[entry].data_ptr(), need[entry], st())))
    r = alternate(runs, reps)
    med = {k[0]: r[k]["median_ms"] for k in rows}
    r["pruned_form"] = FORMS.get(lib.mcp_fps_lengths_form(B, n, m, need[PRUNED]), "unsupported")
    r["unpruned_form"] = "resident" if n <= 16384 else "streaming"
    r["full_lengths_bits_equal_fresh"] = bool(torch.equal(out["a_fresh"], out["b_unpruned_full"]) and torch.equal(out["a_fresh"], out["c_pruned_full"]))
    r["half_lengths_pruned_bits_equal_unpruned"] = bool(torch.equal(out["d_pruned_half"], out["e_unpruned_half"]))
    r["half_lengths_stay_below_the_length"] = bool(int(out["d_pruned_half"].max()) < n // 2)
    spread_a = (r["a_fresh"]["max_ms"] - r["a_fresh"]["min_ms"]) / r["a_fresh"]["median_ms"]
    r["c_over_a"] = round(med["c"] / med["a"], 4)
    r["c_over_a_allowed"] = round(max(1.10, spread_a), 4)
    r["c_over_a_within_allowance"] = r["c_over_a"] <= r["c_over_a_allowed"]
    r["c_over_b"] = round(med["c"] / med["b"], 4)
    r["d_over_e"] = round(med["d"] / med["e"], 4)
    r["d_over_c"] = round(med["d"] / med["c"], 4)
    r["pruned_wins_full"] = med["c"] < med["b"]
    r["pruned_wins_half"] = med["d"] < med["e"]
    return r


def child(reps):
    """The length-free entry point of whichever library MCP_HIP_LIB names, bound directly: an older build has no more."""
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name, restype in ((FRESH, ctypes.c_int), (FRESH_WS, ctypes.c_size_t)):
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = restype
    p, i, st = _lib.fptr, _lib.iptr, _lib.stream
    doc = {}
    for n, m in SHAPES:
        xyz = lidar_cloud(n)
        idx = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
        need = getattr(lib, FRESH_WS)(B, n, m)
        ws = scratch(need, xyz.device)

        def run():
            rc = getattr(lib, FRESH)(B, n, m, p(xyz), i(idx), None, ws.data_ptr(), need, st())
            assert rc == 0, rc

        doc[str(n)] = dict(alternate({FRESH: run}, reps)[FRESH], index_sum=int(idx.long().sum()))
    print(json.dumps(doc), flush=True)


def bench_line(root):
    """The default bench.py line of the checkout at `root`, with that checkout's own package and library."""
    env = {k: v for k, v in os.environ.items() if k != "MCP_HIP_LIB"}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py")], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    if res.returncode != 0:
        raise RuntimeError(f"bench.py failed ({res.returncode}): {res.stderr[-2000:]}")
    return json.loads([ln for ln in res.stdout.strip().splitlines() if ln.startswith("{")][-1])


def against_parent(parent, reps, bench_runs, parent_root):
    new = os.path.join(ROOT, "mocopci_amd", "libmocopci_hip.so")
    runs = []
    for tag, path in (("parent", parent), ("new", new), ("parent", parent), ("new", new)):
        env = dict(os.environ, MCP_HIP_LIB=os.path.abspath(path))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True,
                             text=True, timeout=300)
        if res.returncode != 0:
            raise RuntimeError(f"{tag} run failed ({res.returncode}): {res.stderr[-2000:]}")
        runs.append(dict(json.loads(res.stdout.strip().splitlines()[-1]), library=tag))
        print(f"timed {FRESH} of the {tag} library", file=sys.stderr, flush=True)
    doc = {"order": [r["library"] for r in runs], "runs": runs}
    for n in (str(s[0]) for s in SHAPES):
        med = {t: [r[n]["median_ms"] for r in runs if r["library"] == t] for t in ("parent", "new")}
        spread = max((r[n]["max_ms"] - r[n]["min_ms"]) / r[n]["median_ms"] for r in runs if r["library"] == "parent")
        ratio = (sum(med["new"]) / len(med["new"])) / (sum(med["parent"]) / len(med["parent"]))
        doc[n] = {"parent_median_ms": med["parent"], "new_median_ms": med["new"], "new_over_parent": round(ratio, 4),
                  "allowed_new_over_parent": round(1 + max(0.10, spread), 4), "within_expectation": ratio <= 1 + max(0.10, spread),
                  "same_results": all(r[n]["index_sum"] == runs[0][n]["index_sum"] for r in runs)}
    if bench_runs:
        lines = {"parent": [], "new": []}
        for _ in range(bench_runs):
            for tag, root in (("parent", os.path.abspath(parent_root)), ("new", ROOT)):
                lines[tag].append(bench_line(root))
                print(f"bench.py with the {tag} library: {lines[tag][-1]['value']}", file=sys.stderr, flush=True)
        val = {t: sorted(ln["value"] for ln in lines[t]) for t in lines}
        median = {t: val[t][len(val[t]) // 2] for t in val}
        spread = val["parent"][-1] - val["parent"][0]
        doc["bench"] = {"command": "python bench.py", "order": ["parent", "new"] * bench_runs, "metric": lines["new"][0].get("metric"),
                        "unit": lines["new"][0].get("unit"), "parent_values": [ln["value"] for ln in lines["parent"]],
                        "new_values": [ln["value"] for ln in lines["new"]], "parent_median": median["parent"], "new_median": median["new"],
                        "parent_spread": spread, "new_median_at_least_parent_median_minus_spread": median["new"] >= median["parent"] - spread}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--parent", default=None, help="another build of libmocopci_hip.so to compare the length-free call with")
    ap.add_argument("--bench", type=int, default=0, help="with --parent-root: runs of the default bench.py line per checkout, alternated")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built (bench.py binds every entry "
                    "point of its own header, so each bench line runs in its own checkout)")
    ap.add_argument("--parent-out", default=None, help="with --parent: writes the comparison with the parent to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    doc = {"B": B, "shapes_N_m": [list(s) for s in SHAPES], "reps": a.reps}
    if a.parent:
        doc["against_parent"] = against_parent(a.parent, a.reps, a.bench if a.parent_root else 0, a.parent_root)   # before this process opens the GPU
        if a.parent_out:
            with open(a.parent_out, "w") as fh:
                fh.write(json.dumps(doc["against_parent"], indent=1) + "\n")
    assert torch.cuda.is_available(), "needs a GPU"
    doc["device"] = torch.cuda.get_device_name(0)
    for n, m in SHAPES:
        doc[str(n)] = measure(n, m, a.reps)
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
