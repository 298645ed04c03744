"""-m "not gpu": the index, blend and normalisation primitives (csrc/pointnet2_ops.hip, interp3.hip, norm.hip) are held the way the
other units are (test_kernel_variants_cpu.py): every kernel in their device assembly must be named by an entry of
kernel_variants.PRIMITIVE_CASES (the cases of test_primitive_edges_gpu.py) or by ELSEWHERE with its reason; kernel_variants.primitive_launch
must follow the host conditions of the C entries, stated here as literal expectations; and PRIMITIVE_EDGES states, as predicates on the
mirrored launch of a case -- never on its comment -- every loop, block, tile and register boundary the cases must reach."""
import pytest

from tests import kernel_variants as kv
from tests.test_kernel_variants_cpu import emitted_kernels

PRIMITIVE_UNITS = ("pointnet2_ops", "interp3", "norm")
# Kernels of these units whose edge cases live in another file, by name.
ELSEWHERE = {name: "ball query: its four instantiations are held by test_ball_query_lengths_gpu.py"
             for name in ("ball_query_kernel<false>", "ball_query_kernel<true>", "query_and_group_kernel<false>", "query_and_group_kernel<true>")}
ATOMIC_ENTRIES = ("mcp_gather_points_grad", "mcp_group_points_grad", "mcp_three_interpolate_grad", "mcp_group_rows_grad", "mcp_interp3_apply_grad")
CHANNEL_MAJOR = ("mcp_gather_points", "mcp_group_points", "mcp_three_interpolate") + ATOMIC_ENTRIES[:3] + (
    "mcp_group_points_grad_sorted", "mcp_three_interpolate_grad_sorted")
F4 = "HIP_vector_type<float, 4u>"
# every kernel with a capped grid-stride loop -> its cap.  mfa_prepare_kernel's second round needs 65536 x 256 float4 items in each of
# three outputs (over 800 MB) and is left out on purpose.
CAPPED = {f"group_rows_kernel<{F4}, 4>": 8192, "group_rows_kernel<float, 1>": 8192, "group_rows_add_leaky_kernel": 16384,
          "group_rows_grad_kernel": 8192, "group_rows_grad_sorted_kernel<true>": 16384, "group_rows_grad_sorted_kernel<false>": 16384,
          "group_rows_grad_sorted_narrow_kernel": 16384, f"interp3_apply_kernel<{F4}, 4>": 8192, "interp3_apply_kernel<float, 1>": 8192,
          "interp3_apply_grad_kernel": 8192, "interp3_grad_w_kernel": 16384, "interp3_grad_feat_sorted_kernel<true>": 16384,
          "interp3_grad_feat_sorted_kernel<false>": 16384}


def launches():
    """(case, launch) for every kernel launch of every case."""
    return [(c, l) for c in kv.PRIMITIVE_CASES for l in kv.primitive_case_launch(c)["launches"]]


def kernel_of(entry, **kw):
    out = kv.primitive_launch(entry, **kw)
    assert out["status"] == kv.MCP_OK, (entry, kw, out)
    return [l["kernel"] for l in out["launches"]]


def status_of(entry, **kw):
    out = kv.primitive_launch(entry, **kw)
    assert (out["status"] == kv.MCP_OK) == bool(out["launches"])
    return out["status"]


def test_every_primitive_kernel_has_a_case():
    emitted = emitted_kernels(PRIMITIVE_UNITS)
    assert len(emitted) == 32 and "add_layernorm_kernel<16>" in emitted and f"group_rows_kernel<{F4}, 4>" in emitted, sorted(emitted)
    covered = {n for c in kv.PRIMITIVE_CASES for n in c["kernels"]}
    missing = sorted(emitted - covered - set(ELSEWHERE))
    assert not missing, f"kernels of {PRIMITIVE_UNITS} without a case in kernel_variants.PRIMITIVE_CASES: {missing}"
    stale = sorted((covered | set(ELSEWHERE)) - emitted)
    assert not stale, f"cases or ELSEWHERE name kernels the library does not build: {stale}"
    assert not covered & set(ELSEWHERE)


def test_every_case_states_its_entry_kernels_and_edge_and_ids_are_unique():
    ids = [kv.primitive_case_id(c) for c in kv.PRIMITIVE_CASES]
    assert len(set(ids)) == len(ids)
    for c in kv.PRIMITIVE_CASES:
        out = kv.primitive_case_launch(c)
        assert c["kernels"] == tuple(l["kernel"] for l in out["launches"]) and c["status"] == out["status"] and c["edge"], c
        assert bool(c["kernels"]) == (c["status"] == kv.MCP_OK), c
    for e in ATOMIC_ENTRIES:      # the five exported atomic scatters
        assert kv.primitive_cases(e, ok=True), e


def test_the_primitive_mirror_follows_the_c_conditions():
    # the caps: pointnet2_ops.hip:479, :484, :497, :508, :518, :525; interp3.hip:162, :170, :183, :197, :202; norm.hip:113
    for c, l in launches():
        if l["kernel"] in CAPPED:
            assert l["cap"] == CAPPED[l["kernel"]] and l["grid"] == (min(-(-l["items"] // l["per_wg"]), l["cap"]),), (c, l)
        assert l["rounds"] == -(-l["items"] // (l["grid"][0] * l["per_wg"])), (c, l)
        assert (l["rounds"] - 1) * l["grid"][0] * l["per_wg"] + l["last_round"] == l["items"] and 1 <= l["last_wg"] <= l["per_wg"], (c, l)
    loop = kv.primitive_launch("mcp_group_rows", b=1, n=9, c=4, t=8192 * 256)["launches"][0]
    assert (loop["grid"], loop["rounds"], loop["last_round"], loop["last_wg"]) == ((8192,), 1, 8192 * 256, 256)
    loop = kv.primitive_launch("mcp_group_rows", b=1, n=9, c=4, t=8192 * 256 + 257)["launches"][0]
    assert (loop["grid"], loop["rounds"], loop["last_round"], loop["last_wg"]) == ((8192,), 2, 257, 1)
    assert kv.primitive_launch("mcp_mfa_prepare", rows=1, n=1 << 16, c=1024)["launches"][0]["grid"] == (1 << 16,)
    assert kv.primitive_launch("mcp_mfa_prepare", rows=1, n=(1 << 16) + 1, c=1024)["launches"][0]["rounds"] == 2
    # 8 lanes per row / per (point, neighbour): 32 items per workgroup
    narrow = kv.primitive_launch("mcp_group_rows_grad_sorted", b=2, n=33, c=3, t=5)["launches"][0]
    assert (narrow["kernel"], narrow["per_wg"], narrow["items"], narrow["grid"], narrow["last_wg"]) == ("group_rows_grad_sorted_narrow_kernel", 32, 66, (3,), 2)
    gw = kv.primitive_launch("mcp_interp3_apply_grad_sorted", b=2, n=11, s=5, c=8, want=("w",))["launches"]
    assert [(l["kernel"], l["per_wg"], l["items"], l["grid"]) for l in gw] == [("interp3_grad_w_kernel", 32, 66, (3,))]
    # c <= 4: the narrow route, before and whatever the alignment (pointnet2_ops.hip:516)
    for c in (1, 2, 3, 4):
        for aligned in (True, False):
            assert kernel_of("mcp_group_rows_grad_sorted", aligned=aligned, b=1, n=9, c=c, t=5) == ["group_rows_grad_sorted_narrow_kernel"]
    assert kernel_of("mcp_group_rows_grad_sorted", b=1, n=9, c=5, t=5) == ["group_rows_grad_sorted_kernel<false>"]
    assert kernel_of("mcp_group_rows_grad_sorted", b=1, n=9, c=8, t=5) == ["group_rows_grad_sorted_kernel<true>"]
    # the alignment route: float4 only with c % 4 == 0 AND every tested base on 16 bytes
    for entry, shape, vec, scalar, operands in (
            ("mcp_group_rows", dict(b=1, n=9, t=5), f"group_rows_kernel<{F4}, 4>", "group_rows_kernel<float, 1>", ("points", "out")),
            ("mcp_interp3_apply", dict(b=1, n=9, s=5), f"interp3_apply_kernel<{F4}, 4>", "interp3_apply_kernel<float, 1>", ("feat", "out")),
            ("mcp_group_rows_grad_sorted", dict(b=1, n=9, t=5), "group_rows_grad_sorted_kernel<true>", "group_rows_grad_sorted_kernel<false>",
             ("grad_out", "grad_points"))):
        assert kv.PRIM_ALIGNED_OPERANDS[entry] == operands
        assert kernel_of(entry, c=64, **shape) == [vec] and kernel_of(entry, c=66, **shape) == [scalar]
        assert kernel_of(entry, aligned=False, c=64, **shape) == [scalar]
        for o in operands:
            assert kernel_of(entry, off=(o,), c=64, **shape) == [scalar]
        with pytest.raises(ValueError):
            kv.primitive_launch(entry, off=("idx",), c=64, **shape)
    vec_items = kv.primitive_launch("mcp_group_rows", b=2, n=9, t=5, c=64)["launches"][0]["items"]
    assert vec_items == 2 * 5 * 16 and kv.primitive_launch("mcp_group_rows", off=("out",), b=2, n=9, t=5, c=64)["launches"][0]["items"] == 2 * 5 * 64
    # interp3_apply_grad_sorted: grad_w3 first, then grad_feat; each tests its own pair of operands (interp3.hip:161, :168)
    i3 = dict(b=1, n=9, s=5)
    w, ft, ff = "interp3_grad_w_kernel", "interp3_grad_feat_sorted_kernel<true>", "interp3_grad_feat_sorted_kernel<false>"
    assert kernel_of("mcp_interp3_apply_grad_sorted", c=64, **i3) == [w, ft]
    assert kernel_of("mcp_interp3_apply_grad_sorted", c=64, want=("feat",), **i3) == [ft] and kernel_of("mcp_interp3_apply_grad_sorted", c=64, want=("w",), **i3) == [w]
    assert status_of("mcp_interp3_apply_grad_sorted", c=64, want=(), **i3) == kv.MCP_ERR_BAD_ARG
    for off, vec, feat in ((("grad_out",), 0, ff), (("feat",), 0, ft), (("grad_feat",), 1, ff), ((), 1, ft)):
        out = kv.primitive_launch("mcp_interp3_apply_grad_sorted", off=off, c=64, **i3)["launches"]
        assert (out[0]["vec"], out[1]["kernel"]) == (vec, feat), off
    out = kv.primitive_launch("mcp_interp3_apply_grad_sorted", c=35, **i3)["launches"]
    assert (out[0]["vec"], out[0]["passes"], out[1]["kernel"]) == (0, 5, ff)
    assert [kv.primitive_launch("mcp_interp3_apply_grad_sorted", c=c, **i3)["launches"][0]["passes"] for c in (4, 28, 32, 36)] == [1, 1, 1, 2]
    # the PER ladder, c > 1024, the strides (norm.hip:65-72)
    for c, per in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 16), (1024, 16)):
        assert kernel_of("mcp_add_layernorm", rows=3, c=c) == [f"add_layernorm_kernel<{per}>"]
    assert status_of("mcp_add_layernorm", rows=3, c=1025) == kv.MCP_ERR_UNSUPPORTED
    for stride in ("x_stride", "y_stride", "out_stride"):
        assert status_of("mcp_add_layernorm", rows=3, c=65, **{stride: 64}) == kv.MCP_ERR_BAD_ARG
        assert status_of("mcp_add_layernorm", rows=3, c=65, **{stride: 65}) == kv.MCP_OK
    assert status_of("mcp_add_layernorm", rows=3, c=65, y_stride=0, with_y=False) == kv.MCP_OK
    assert status_of("mcp_add_layernorm", rows=3, c=1025, x_stride=64) == kv.MCP_ERR_BAD_ARG      # the argument check comes first
    ln = kv.primitive_launch("mcp_add_layernorm", rows=5, c=65)["launches"][0]
    assert (ln["grid"], ln["last_wg"], ln["registers"], ln["last_register"]) == ((2,), 1, 2, 1)
    # the refusals: c & 3 in mfa_prepare is UNSUPPORTED and comes before the alignment test; add_leaky answers BAD_ARG to both
    assert status_of("mcp_mfa_prepare", rows=2, n=3, c=6) == kv.MCP_ERR_UNSUPPORTED
    assert status_of("mcp_mfa_prepare", aligned=False, rows=2, n=3, c=6) == kv.MCP_ERR_UNSUPPORTED
    assert status_of("mcp_mfa_prepare", rows=2, n=3, c=8) == kv.MCP_OK
    for o in kv.PRIM_ALIGNED_OPERANDS["mcp_mfa_prepare"]:
        assert status_of("mcp_mfa_prepare", off=(o,), rows=2, n=3, c=8) == kv.MCP_ERR_BAD_ARG
    assert status_of("mcp_group_rows_add_leaky", b=1, n=9, c=6, s=2, k=2) == kv.MCP_ERR_BAD_ARG
    for o in ("points", "centre", "out"):
        assert status_of("mcp_group_rows_add_leaky", off=(o,), b=1, n=9, c=8, s=2, k=2) == kv.MCP_ERR_BAD_ARG
    assert kernel_of("mcp_group_rows_add_leaky", b=1, n=9, c=8, s=2, k=2) == ["group_rows_add_leaky_kernel"]
    assert status_of("mcp_group_rows", b=0, n=9, c=8, t=2) == kv.MCP_ERR_BAD_ARG
    # the block kernels: grids and tiles
    gp = kv.primitive_launch("mcp_group_points", b=3, c=17, n=5, npoints=257, nsample=2)["launches"][0]
    assert (gp["grid"], gp["last_wg"], gp["last_chunk"]) == ((3, 3, 3), 2, 1)
    assert kv.primitive_launch("mcp_gather_points", b=3, c=17, n=5, npoints=257)["launches"][0]["grid"] == (2, 3)
    assert kv.primitive_launch("mcp_group_points_grad_sorted", b=3, c=9, n=257, t=5)["launches"][0]["grid"] == (2, 2, 3)
    assert kv.primitive_launch("mcp_three_interpolate_grad_sorted", b=3, c=9, n=5, m=257)["launches"][0]["grid"] == (2, 2, 3)
    nn = kv.primitive_launch("mcp_three_nn", b=3, n=257, m=2049)["launches"][0]
    assert (nn["grid"], nn["last_wg"], nn["tiles"], nn["last_tile"]) == ((2, 3), 1, 3, 1)
    assert kernel_of("mcp_interp3", b=1, n=9, s=5, c=8) == ["interp3_weights_kernel", f"interp3_apply_kernel<{F4}, 4>"]
    with pytest.raises(ValueError):
        kv.primitive_launch("mcp_ball_query", b=1, n=9, m=3)


def _of(entry, ok=True):
    return [(c, kv.primitive_case_launch(c)) for c in kv.primitive_cases(entry, ok=ok)]


def _block_axis(l):
    """The thread-axis count of a block kernel, rebuilt from its grid and the live threads of the last workgroup."""
    return (l["grid"][0] - 1) * kv.PRIM_BLK + l["last_wg"]


def _chunk_axis(l):
    return (l["grid"][1] - 1) * kv.PRIM_CCH + l["last_chunk"]


def test_the_primitive_cases_reach_every_edge_class():
    missing = []

    def need(what, found):
        if not found:
            missing.append(what)
    every = launches()
    # (2) a second grid-stride round that leaves all but one or two workgroups without an item, for every capped loop (add_leaky: one
    # centre of 8 x 64 float4 items past the cap) -- and a one-round case beside it
    for kernel in CAPPED:
        mine = [l for _, l in every if l["kernel"] == kernel]
        need(f"{kernel}: a second round of at most two workgroups", any(l["rounds"] == 2 and l["last_round"] <= 2 * l["per_wg"] for l in mine))
        need(f"{kernel}: a single round", any(l["rounds"] == 1 for l in mine))
    assert [l["rounds"] for _, l in every if l["kernel"] == "mfa_prepare_kernel"] == [1] * 4      # left out on purpose, see CAPPED
    # the determinism runs: every sorted / fixed-order second-round case is run twice
    for c, l in every:
        if l["rounds"] == 2 and c["entry"] not in ATOMIC_ENTRIES:
            need(f"{kv.primitive_case_id(c)}: twice", c.get("twice"))
    # (4) channel-major: BLK -1 / 0 / +1 and one point on the thread axis, CCH -1 / 0 / +1 and 17 channels, (257, 9) together
    for e in CHANNEL_MAJOR:
        ls = [l for _, out in _of(e) for l in out["launches"]]
        chunked = "last_chunk" in ls[0]
        chans = {c["shape"]["c"] for c, _ in _of(e)}
        need(f"{e}: thread axis", {_block_axis(l) for l in ls} >= {1, 255, 256, 257})
        need(f"{e}: channels", chans >= {1, 7, 8, 9, 17} and (not chunked or {_chunk_axis(l) for l in ls} >= {1, 7, 8, 9, 17}))
        need(f"{e}: (257, 9)", any(_block_axis(l) == 257 and c["shape"]["c"] == 9 for c, out in _of(e) for l in out["launches"]))
        assert all(c["shape"]["b"] == 3 for c, _ in _of(e))
    for e in ("mcp_gather_points", "mcp_group_points", "mcp_three_interpolate", "mcp_group_points_grad_sorted", "mcp_three_interpolate_grad_sorted"):
        need(f"{e}: one case on real data against the C oracle", sum(c.get("data") == "real" for c in kv.primitive_cases(e)) == 1)
    for e in ("mcp_group_points_grad_sorted", "mcp_three_interpolate_grad_sorted", "mcp_group_rows_grad_sorted", "mcp_interp3_apply_grad_sorted"):
        need(f"{e}: one case with the segments of ops._scatter_segments", any(c.get("segments") == "ops" for c in kv.primitive_cases(e)))
    # (3) group_rows / interp3_apply: both routes, the scalar one by c % 4 and by each operand's alignment at c = 64, a single item
    for e, twin, operands in (("mcp_group_rows", "group_rows_kernel", ("points", "out")), ("mcp_interp3_apply", "interp3_apply_kernel", ("feat", "out"))):
        cs = _of(e)
        need(f"{e}: channels", {c["shape"]["c"] for c, _ in cs} >= {1, 3, 4, 5, 256})
        need(f"{e}: one item", any(out["launches"][0]["items"] == 1 and c["shape"]["b"] == 1 for c, out in cs))
        need(f"{e}: float4", any(c["kernels"] == (f"{twin}<{F4}, 4>",) for c, _ in cs))
        need(f"{e}: scalar by c % 4", any(c["kernels"] == (f"{twin}<float, 1>",) and c["shape"]["c"] % 4 and not c["off"] for c, _ in cs))
        for o in operands:
            need(f"{e}: scalar by {o}", any(c["kernels"] == (f"{twin}<float, 1>",) and c["shape"]["c"] == 64 and c["off"] == (o,) for c, _ in cs))
    vec, scalar = (next(l for c, l in every if c["entry"] == "mcp_group_rows" and l["kernel"] == k and l["rounds"] == 2)
                   for k in (f"group_rows_kernel<{F4}, 4>", "group_rows_kernel<float, 1>"))
    assert (vec["items"], vec["last_round"], scalar["items"], scalar["last_round"]) == (2097216, 64, 2097165, 13)
    # group_rows_add_leaky
    need("add_leaky: channels", {c["shape"]["c"] for c, _ in _of("mcp_group_rows_add_leaky")} >= {4, 24, 256})
    refused = kv.primitive_cases("mcp_group_rows_add_leaky", ok=False)
    need("add_leaky: c % 4", any(c["shape"]["c"] % 4 and not c["off"] for c in refused))
    need("add_leaky: every operand off", {c["off"] for c in refused if c["shape"]["c"] % 4 == 0} == {("points",), ("centre",), ("out",)})
    assert all(c["status"] == kv.MCP_ERR_BAD_ARG for c in refused)
    # group_rows_grad_sorted
    gs = _of("mcp_group_rows_grad_sorted")
    need("grad_sorted: narrow at c = 1..4", {c["shape"]["c"] for c, _ in gs if c["kernels"] == ("group_rows_grad_sorted_narrow_kernel",)} >= {1, 2, 3, 4})
    need("grad_sorted: <true>", any(c["kernels"] == ("group_rows_grad_sorted_kernel<true>",) for c, _ in gs))
    need("grad_sorted: <false> by c % 4", any(c["kernels"] == ("group_rows_grad_sorted_kernel<false>",) and c["shape"]["c"] % 4 and not c["off"] for c, _ in gs))
    for o in ("grad_out", "grad_points"):
        need(f"grad_sorted: <false> by {o}", any(c["kernels"] == ("group_rows_grad_sorted_kernel<false>",) and c["shape"]["c"] == 64 and c["off"] == (o,) for c, _ in gs))
    assert all(c["shape"]["t"] <= 4000 for c, _ in gs)      # the CPU reference stays cheap
    # interp3_apply_grad_sorted
    i3 = _of("mcp_interp3_apply_grad_sorted")
    need("interp3 sorted: channels", {c["shape"]["c"] for c, _ in i3} >= {1, 4, 28, 32, 36})
    need("interp3 sorted: each gradient alone", {c["shape"].get("want") for c, _ in i3} >= {("feat",), ("w",), None})
    w_launches = [(c, l) for c, out in i3 for l in out["launches"] if l["kernel"] == "interp3_grad_w_kernel"]
    need("interp3 sorted: quads below / at / above one pass of 8 lanes",
         {(l["vec"], c["shape"]["c"] >> 2) for c, l in w_launches} >= {(1, 1), (1, 7), (1, 8), (1, 9)} and {l["passes"] for _, l in w_launches if l["vec"]} >= {1, 2})
    need("interp3 sorted: vec = 0 by c % 4", any(l["vec"] == 0 and c["shape"]["c"] % 4 for c, l in w_launches))
    for o in ("grad_out", "feat"):
        need(f"interp3 sorted: vec = 0 by {o}", any(l["vec"] == 0 and c["shape"]["c"] == 64 and c["off"] == (o,) for c, l in w_launches))
    for o in ("grad_out", "grad_feat"):
        need(f"interp3 sorted: grad_feat <false> by {o}", any("interp3_grad_feat_sorted_kernel<false>" in c["kernels"] and c["shape"]["c"] == 64 and c["off"] == (o,) for c, _ in i3))
    need("interp3 sorted: grad_feat <false> by c % 4", any("interp3_grad_feat_sorted_kernel<false>" in c["kernels"] and c["shape"]["c"] % 4 and not c["off"] for c, _ in i3))
    # the atomic channel-last scatters
    for e in ("mcp_group_rows_grad", "mcp_interp3_apply_grad"):
        need(f"{e}: channels", {c["shape"]["c"] for c, _ in _of(e)} >= {1, 3, 4, 5, 256})
    # three_nn: NN_TILE and BLK
    nn = [out["launches"][0] for _, out in _of("mcp_three_nn")]
    need("three_nn: known points", {(l["tiles"], l["last_tile"]) for l in nn} >= {(1, 1), (1, 2), (1, 3), (1, 4), (1, 1023), (1, 1024), (2, 1), (3, 1)})
    need("three_nn: unknown points", {_block_axis(l) for l in nn} >= {1, 255, 256, 257})
    need("three_nn: ties across a tile boundary", any(c.get("grid") and out["launches"][0]["tiles"] > 1 for c, out in _of("mcp_three_nn")))
    # interp3 / interp3_weights
    for e in ("mcp_interp3", "mcp_interp3_weights"):
        need(f"{e}: n x s", {(_block_axis(out["launches"][0]), c["shape"]["s"]) for c, out in _of(e) if not c.get("coincident")}
             >= {(n, s) for n in (1, 255, 256, 257) for s in (3, 40)})
        need(f"{e}: coincident", [c["coincident"] for c, _ in _of(e) if c.get("coincident")] == [5])
    # add_layernorm: -1 / 0 / +1 around every register of every PER, the row counts around the four waves of a workgroup
    ln = [out["launches"][0] for _, out in _of("mcp_add_layernorm")]
    need("layernorm: channels", {(l["per"], l["registers"], l["last_register"]) for l in ln}
         >= {(1, 1, 1), (1, 1, 63), (1, 1, 64), (2, 2, 1), (2, 2, 63), (2, 2, 64), (4, 3, 1), (4, 4, 63), (4, 4, 64), (16, 5, 1), (16, 16, 63), (16, 16, 64)})
    need("layernorm: rows", {(l["grid"][0], l["last_wg"]) for l in ln} >= {(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (257, 3)})
    need("layernorm: refusals", {c["status"] for c in kv.primitive_cases("mcp_add_layernorm", ok=False)} == {kv.MCP_ERR_UNSUPPORTED, kv.MCP_ERR_BAD_ARG})
    # mfa_prepare
    mf = kv.primitive_cases("mcp_mfa_prepare", ok=True)
    need("mfa_prepare: shapes", {c["shape"]["rows"] for c in mf} >= {1, 5} and {c["shape"]["n"] for c in mf} >= {1, 33} and {c["shape"]["c"] for c in mf} >= {4, 64})
    bad = kv.primitive_cases("mcp_mfa_prepare", ok=False)
    need("mfa_prepare: c = 6", any(c["status"] == kv.MCP_ERR_UNSUPPORTED and c["shape"]["c"] == 6 for c in bad))
    need("mfa_prepare: an unaligned operand", any(c["status"] == kv.MCP_ERR_BAD_ARG and c["off"] for c in bad))
    assert not missing, missing
