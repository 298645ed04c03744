"""Device times of the pruned KNN search under per-cloud lengths (device events after warm-up; medians of --reps (25) single
launches with min and max, the rows of one shape alternating per repetition in one process).

Shapes (B, Q, N, K, distance form, query lengths, reference lengths):
  scan_as_reference   8 x  8192 x 40960, K = 1 direct, every rlen 34000     a prediction against a whole scan
  scan_as_query       8 x 40960 x  8192, K = 1 direct, every qlen 34000     the reverse direction
  scan_as_reference_k32  the first shape at K = 32 expansion (the walk kernel with 16 tile bounds per lane)
  half_k1             8 x  8192 x  8192, K = 1 direct, both lengths 4096
  full_k32, half_k32  8 x  8192 x  8192, K = 32 expansion, both lengths 8192 / 4096
  min_k1, min_k32     8 x  1024 x  2048, the smallest shape of the size rule, about half lengths (513 / 1000); K = 1 direct, K = 32 expansion
  mid_k1, mid_k32     8 x  2048 x  4096 likewise (1030 / 2000)
  full_k16           48 x  2048 x  2048, K = 16 expansion, both lengths 2048: round 3's kernel in its K <= 16 class, the shape
                      tools/knn_ab.py quotes
Rows per shape:
  a  exhaustive_lengths   mcp_knn_lengths (HipBackend.knn_bruteforce with the lengths): the baseline, code this search does not share
  b  pruned_with_builds   HipBackend.knn with the lengths outside a cloud_scope: both clouds sorted under their lengths + the search
  c  pruned_search        mcp_knn_pruned_lengths alone on clouds built beforehand
  c_full                  the same with every length full
  d  plain_pruned         mcp_knn_pruned on length-free clouds (every row valid)
Recorded with the numbers:
  * b_wins: b's median is below a's by more than a's own max - min -- the condition for keeping the pruned route for the shape class;
  * c_full against d: at most max(10 %, d's (max - min) / median) above d's median, and bit-identical results;
  * half lengths against full lengths (reported only);
  * a, b, c agree bit for bit.
`--plain-only` measures row d alone (it also runs with a library that lacks the length entry points: MCP_HIP_LIB selects the
library, as everywhere); `--plain-runs P1 N1 P2 N2` merges four such documents, taken in fresh processes in the order parent, new,
parent, new, and records whether the new library's d stays within max(10 %, the parent's spread) of the parent's.
Prints one JSON document; `--out FILE` writes it there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import _lib, ops  # noqa: E402

SHAPES = [
    ("scan_as_reference", 8, 8192, 40960, 1, 1, None, 34000),
    ("scan_as_query", 8, 40960, 8192, 1, 1, 34000, None),
    ("half_k1", 8, 8192, 8192, 1, 1, 4096, 4096),
    ("full_k32", 8, 8192, 8192, 32, 0, 8192, 8192),
    ("half_k32", 8, 8192, 8192, 32, 0, 4096, 4096),
    ("scan_as_reference_k32", 8, 8192, 40960, 32, 0, None, 34000),
    ("min_k1", 8, 1024, 2048, 1, 1, 513, 1000),
    ("min_k32", 8, 1024, 2048, 32, 0, 513, 1000),
    ("mid_k1", 8, 2048, 4096, 1, 1, 1030, 2000),
    ("mid_k32", 8, 2048, 4096, 32, 0, 1030, 2000),
    ("full_k16", 48, 2048, 2048, 16, 0, 2048, 2048),
]
LENGTH_ENTRY_POINTS = ("mcp_build_cloud_lengths", "mcp_morton_codes_lengths", "mcp_tile_boxes_lengths", "mcp_knn_pruned_lengths")
DEV = "cuda:0"


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
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(reps):
        for name, fn in runs.items():
            times[name].append(timed(fn))
    return {name: stats(v) for name, v in times.items()}


def clouds(Q, N, B, gen):
    extent = torch.tensor([40.0, 40.0, 3.0])
    return (((torch.rand(B, Q, 3, generator=gen) * 2 - 1) * extent).to(DEV), ((torch.rand(B, N, 3, generator=gen) * 2 - 1) * extent).to(DEV))


def lengths(v, B):
    return None if v is None else torch.full((B,), v, dtype=torch.int32, device=DEV)


def outputs(B, Q, K):
    return torch.empty((B, Q, K), dtype=torch.int32, device=DEV), torch.empty((B, Q, K), dtype=torch.float32, device=DEV)


def plain_run(be, query, ref, K, mode, out):
    B, Q, _ = query.shape
    N = ref.shape[1]
    qs, qperm, _ = be._build_cloud(query)
    rs, rperm, boxes = be._build_cloud(ref)
    f, i = _lib.fptr, _lib.iptr
    return lambda: ops._call("mcp_knn_pruned", query, B, Q, N, K, mode, f(qs), i(qperm), f(rs), i(rperm), f(boxes), i(out[0]), f(out[1]))


def measure(name, B, Q, N, K, mode, qlen, rlen, reps, gen, plain_only):
    be = ops.backend()
    query, ref = clouds(Q, N, B, gen)
    r = {"shape": name, "B": B, "Q": Q, "N": N, "K": K, "dist_form": "direct" if mode else "expansion", "qlen": qlen, "rlen": rlen, "reps": reps}
    out_d = outputs(B, Q, K)
    runs = {"plain_pruned": plain_run(be, query, ref, K, mode, out_d)}
    if plain_only:
        r.update(alternate(runs, reps))
        return r
    ql, rl = lengths(qlen, B), lengths(rlen, B)
    fq, fr = lengths(Q, B), lengths(N, B)
    f, i = _lib.fptr, _lib.iptr
    res = {}

    def exhaustive():
        res["a"] = be.knn_bruteforce(query, ref, K, mode=mode, return_dist=True, query_lengths=ql, ref_lengths=rl)

    def with_builds():
        res["b"] = be.knn(query, ref, K, mode=mode, return_dist=True, query_lengths=ql, ref_lengths=rl)

    def search_alone(tag, ql_, rl_):
        qs, qperm, _ = be._build_cloud(query, ql_)
        rs, rperm, boxes = be._build_cloud(ref, rl_)
        out = res[tag] = outputs(B, Q, K)
        return lambda: ops._call("mcp_knn_pruned_lengths", query, B, Q, N, K, mode, f(qs), i(qperm), f(rs), i(rperm), f(boxes),
                                 None if ql_ is None else i(ql_), None if rl_ is None else i(rl_), i(out[0]), f(out[1]))

    runs = {"exhaustive_lengths": exhaustive, "pruned_with_builds": with_builds, "pruned_search": search_alone("c", ql, rl),
            "pruned_search_full_lengths": search_alone("c_full", fq, fr), **runs}
    assert be.prunes_with_lengths(Q, N, K), "row b would not take the pruned route: set the thresholds low for the measurement"
    r.update(alternate(runs, reps))
    a, b, d = r["exhaustive_lengths"], r["pruned_with_builds"], r["plain_pruned"]
    r["b_over_a"] = round(b["median_ms"] / a["median_ms"], 4)
    r["b_wins"] = b["median_ms"] < a["median_ms"] - (a["max_ms"] - a["min_ms"])
    spread = (d["max_ms"] - d["min_ms"]) / d["median_ms"]
    r["c_full_over_d"] = round(r["pruned_search_full_lengths"]["median_ms"] / d["median_ms"], 4)
    r["allowed_c_full_over_d"] = round(1 + max(0.10, spread), 4)
    r["c_full_within_bound"] = r["c_full_over_d"] <= r["allowed_c_full_over_d"]
    r["c_over_c_full"] = round(r["pruned_search"]["median_ms"] / r["pruned_search_full_lengths"]["median_ms"], 4)
    same = lambda x, y: bool(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]))
    r["c_full_bits_equal_d"] = same(res["c_full"], out_d)
    r["a_b_c_bits_equal"] = same(res["a"], res["b"]) and same(res["a"], res["c"])
    return r


def merge_plain_runs(doc, paths):
    """paths: parent, new, parent, new -- one --plain-only document each, from fresh processes in that order."""
    docs = [json.load(open(p)) for p in paths]
    rows = []
    for k in range(len(docs[0]["shapes"])):
        runs = [d["shapes"][k]["plain_pruned"] for d in docs]
        parent, new = runs[0::2], runs[1::2]
        pm, nm = sorted(x["median_ms"] for x in parent), sorted(x["median_ms"] for x in new)
        p_med, n_med = sum(pm) / len(pm), sum(nm) / len(nm)
        spread = (max(x["max_ms"] for x in parent) - min(x["min_ms"] for x in parent)) / p_med
        rows.append({"shape": docs[0]["shapes"][k]["shape"], "order": ["parent", "new", "parent", "new"], "runs": runs,
                     "parent_median_ms": round(p_med, 4), "new_median_ms": round(n_med, 4), "new_over_parent": round(n_med / p_med, 4),
                     "allowed_new_over_parent": round(1 + max(0.10, spread), 4), "within_bound": n_med / p_med <= 1 + max(0.10, spread)})
    doc["plain_pruned_new_library_against_parent"] = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--plain-runs", nargs=4, default=None, metavar="JSON")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.plain_only:   # a library from before the length entry points binds without them
        for name in LENGTH_ENTRY_POINTS:
            _lib.SIGNATURES.pop(name, None)
    gen = torch.Generator().manual_seed(7)
    doc = {"device": torch.cuda.get_device_name(0), "library": _lib.SO_PATH if a.plain_only else "in-tree",
           "shapes": [measure(*s, a.reps, gen, a.plain_only) for s in SHAPES]}
    if a.plain_runs:
        merge_plain_runs(doc, a.plain_runs)
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
