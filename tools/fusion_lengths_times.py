#!/usr/bin/env python3
"""What per-cloud lengths cost and save in the fusion layer, at the step's own shape (24 x 8192 points: the three calls of
MoCoPCI.fusion at B = 8), this tree against a checkout of its parent commit (built, with its library in place).

    python tools/fusion_lengths_times.py --parent DIR [--rounds 3] [--windows 4] [--calls 5] > profiles/fusion_lengths_times.json

The two trees are two libraries, so each runs in a process of its own (`--child`, which imports the package of the tree it is given);
the driver starts them one after the other, parent and this tree taking turns `rounds` times, and keeps every window.  A window is
`calls` back-to-back calls between two device events; a figure is microseconds per call.  Per tree, route and length pattern:
rounds x windows windows (>= 50 calls at the defaults, after a warm-up of every route), of which the median and the quartiles are
reported; `spread` is the parent's own (q3 - q1) / q1 on the dense pattern of the route, with a floor of 2 %.  `now_over_parent` is
this tree's median over the parent's for the same route and pattern (for the kept-score backward: over the parent's only backward
under lengths, the re-evaluating one), `now_over_parent_dense` / `now_over_own_dense` over the call without lengths in the parent's /
this tree's own processes -- the same code in both, yet not always the same figure: what ran before a window differs between the
trees (the parent's backward routes spend ~0.2 s per call in the scatter), so a saving is best read inside one tree.

Routes: fusion_mlp(lengths=) forward (no autograd); forward + backward; the backward of fusion_bn(lengths=) alone (retain_graph),
with the kept scores and, where the tree has the switch (HipBackend.FUSION_BN_KEEP_SCORES_WITH_LENGTHS), re-evaluating the layer --
the parent has the re-evaluating one only.  Length patterns: `none` (no lengths: the dense call), (a) `full` every length n, (b) `half`
every length n / 2, (c) `eighths`: of the three elements that make up each XCD's eighth of the points one is full and two hold n / 4
-- the deal is static per eighth, so the fullest eighth sets the time.  The lists are the two searches' of random clouds, cut to the
live rows; padded rows of the lists hold 0, as the searches leave them.  Last, in this tree: the segmented scatter of grad_nb under
(b) with the padded list rows as they are (all on row 0) against spread over the rows (grad.spread_padded_rows) -- why both autograd
functions spread them (ops._scatter_lists); the parent scatters them as they are, in both of its backward routes."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def child(a):
    sys.path.insert(0, a.child)
    import torch
    from mocopci_amd import grad, ops
    assert os.path.abspath(os.path.dirname(os.path.dirname(ops.__file__))) == os.path.abspath(a.child)
    be = ops.backend()
    B, N = a.clouds, a.n
    g = torch.Generator().manual_seed(0)
    r = lambda *shape, scale=1.0: ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)
    p1 = r(B, N, 3)
    p2 = p1 + r(B, N, 3, scale=0.05)
    conv = [r(64, 4, scale=0.8), r(64, scale=0.2), r(64, 64, scale=0.2), r(64, scale=0.2), r(128, 64, scale=0.2), r(128, scale=0.2)]
    aff = [t for c in (64, 64, 128) for t in (1.0 + r(c, scale=0.2), r(c, scale=0.2))]
    gout = r(B, N, 3)
    eighths = [N if e % 3 == 0 else N // 4 for e in range(B)]
    patterns = {"none": None, "full": [N] * B, "half": [N // 2] * B, "eighths": eighths}
    lens = {k: None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV) for k, v in patterns.items()}

    def lists(l):
        """the two searches' lists; with lengths: of the live prefixes, padded rows 0"""
        kw = {} if l is None else dict(query_lengths=l, ref_lengths=l)
        return be.knn(p1, p1, 32, **kw), be.knn(p1, p2, 32, **kw)
    idx = {k: lists(l) for k, l in lens.items()}
    kw = lambda k: {} if lens[k] is None else dict(lengths=lens[k])

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.calls

    routes = {}
    for k in lens:   # (no leaf asks for a gradient: the forward kernel alone)
        routes[("fusion_mlp forward", k)] = lambda k=k: be.fusion_mlp(p1, p2, idx[k], *conv, **kw(k))
    leaves = [t.clone().requires_grad_(True) for t in (p1, p2, *conv)]
    for k in lens:
        routes[("fusion_mlp forward + backward", k)] = lambda k=k: torch.autograd.grad(be.fusion_mlp(leaves[0], leaves[1], idx[k], *leaves[2:], **kw(k)), leaves, gout)
    bleaves = [t.clone().requires_grad_(True) for t in (p1, p2, *conv, *aff)]
    switch = hasattr(type(be), "FUSION_BN_KEEP_SCORES_WITH_LENGTHS")
    # without lengths the route always keeps its scores; with lengths the parent always re-evaluates the layer
    settings = [("kept scores", None, ["none"])] + ([("kept scores", True, list(lens)[1:]), ("re-evaluated", False, list(lens)[1:])] if switch
                                                   else [("re-evaluated", None, list(lens)[1:])])
    out = {}
    for name, keep, which in settings:
        for k in which:
            if keep is not None:
                type(be).FUSION_BN_KEEP_SCORES_WITH_LENGTHS = keep
            graph = be.fusion_bn(bleaves[0], bleaves[1], idx[k], bleaves[2:8], bleaves[8:], 1e-3, **kw(k))[0]
            routes[("fusion_bn backward, " + name, k)] = lambda graph=graph: torch.autograd.grad(graph, bleaves, gout, retain_graph=True)
    if switch:
        type(be).FUSION_BN_KEEP_SCORES_WITH_LENGTHS = True
    for fn in routes.values():   # warm every route
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.windows):
        for key, fn in routes.items():
            out.setdefault(" | ".join(key), []).append(round(timed(fn), 2))
    res = {"windows_us": out}
    if a.scatter:
        live = grad.live_points(lens["half"], B, N, DEV)
        rows = torch.where(live.view(B, N, 1, 1), r(B, N, 64, 3), torch.zeros((), device=DEV))
        whole = torch.cat(idx["half"], dim=-1)
        forms = {"padded_rows_on_row_0": whole, "padded_rows_spread": grad.spread_padded_rows(whole, live, N)}
        run = lambda l: ops._group_rows_grad(rows, l, N)
        sc = {"equal_bits": bool(torch.equal(*(run(l) for l in forms.values())))}
        for k, l in forms.items():
            run(l)
            torch.cuda.synchronize()
            sc[k + "_us"] = [round(timed(lambda: run(l)), 2) for _ in range(a.windows)]
        res["scatter"] = sc
    res["device"] = torch.cuda.get_device_name(0)
    print("RESULT " + json.dumps(res))


def figures(v):
    q1, _, q3 = statistics.quantiles(v, n=4)
    return {"min_us": round(min(v), 2), "q1_us": round(q1, 2), "median_us": round(statistics.median(v), 2), "q3_us": round(q3, 2), "max_us": round(max(v), 2),
            "windows": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--child", help="(internal) the tree to measure in this process")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--clouds", type=int, default=24)
    ap.add_argument("--scatter", action="store_true")
    ap.add_argument("--raw", help="also write every window to this file, before the report is formed")
    ap.add_argument("--from-raw", help="form the report from a file that --raw wrote (no GPU needed)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    trees = {"parent": os.path.abspath(a.parent or "."), "now": HERE}
    windows, scatter, device = {t: {} for t in trees}, None, None
    if a.from_raw:
        raw = json.load(open(a.from_raw))
        windows, scatter, device = raw["windows_us"], raw["scatter"], raw.get("device")
    for rnd in range(0 if a.from_raw else a.rounds):
        for tree, root in trees.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--windows", str(a.windows), "--calls", str(a.calls), "--n", str(a.n),
                   "--clouds", str(a.clouds)] + (["--scatter"] if tree == "now" and rnd == 0 else [])
            done = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
            if done.returncode != 0:   # a failed process ends the measurement: nothing more is started on the GPU
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                return 1
            res = json.loads(next(l for l in done.stdout.splitlines() if l.startswith("RESULT "))[7:])
            device = res["device"]
            scatter = res.get("scatter", scatter)
            for k, v in res["windows_us"].items():
                windows[tree].setdefault(k, []).extend(v)
    if a.raw:
        json.dump({"windows_us": windows, "scatter": scatter, "device": device}, open(a.raw, "w"))
    report = {"clouds": a.clouds, "n": a.n, "rounds": a.rounds, "windows_per_round": a.windows, "calls_per_window": a.calls, "device": device, "routes": {}}
    for key in windows["now"]:
        route, pattern = key.split(" | ")
        row = report["routes"].setdefault(route, {})
        row[pattern] = {t: figures(windows[t][key]) for t in trees if key in windows[t]}
    for route, row in report["routes"].items():
        # the parent has one train-mode backward under lengths, the re-evaluating one: both of this tree's are held against it
        base_route = route if "parent" in row.get("half", {}) else "fusion_bn backward, re-evaluated"
        base = report["routes"][base_route]
        dense = report["routes"]["fusion_bn backward, kept scores" if route.startswith("fusion_bn") else route]["none"]["parent"]
        spread = round(max(0.02, (dense["q3_us"] - dense["q1_us"]) / dense["q1_us"]), 4)
        row["parent_spread_of_the_dense_call"] = spread
        for pattern in ("full", "half", "eighths"):
            if pattern in row:
                row[pattern]["now_over_parent"] = round(row[pattern]["now"]["median_us"] / base[pattern]["parent"]["median_us"], 4)
                row[pattern]["now_over_parent_dense"] = round(row[pattern]["now"]["median_us"] / dense["median_us"], 4)
                own = report["routes"]["fusion_bn backward, kept scores" if route.startswith("fusion_bn") else route]["none"]["now"]
                row[pattern]["now_over_own_dense"] = round(row[pattern]["now"]["median_us"] / own["median_us"], 4)
        row["full_not_slower_than_parent_by_more_than_spread"] = row["full"]["now_over_parent"] - 1 <= spread
        row["half_faster_than_parent_by_more_than_spread"] = 1 - row["half"]["now_over_parent"] > spread
    if scatter:
        for k in ("padded_rows_on_row_0_us", "padded_rows_spread_us"):
            scatter[k] = {"median_us": round(statistics.median(scatter[k]), 2), "min_us": min(scatter[k]), "max_us": max(scatter[k])}
        scatter["row_0_over_spread"] = round(scatter["padded_rows_on_row_0_us"]["median_us"] / scatter["padded_rows_spread_us"]["median_us"], 2)
        report["scatter of grad_nb, every length n / 2 (this tree)"] = scatter
    print(json.dumps(report, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
