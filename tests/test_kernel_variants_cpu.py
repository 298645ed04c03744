"""-m "not gpu": every kernel instantiation of the dense-layer units (linear, mlp, attention) and of the fused point-layer units
(fusion, cross, pointconv, ptblock) has a parity case.  The device assembly lists the instantiations the compiler actually emitted;
each one except the weight-packing kernels and the entries of NOT_LAUNCHED must be what kernel_variants.expected_kernel names for at
least one entry of kernel_variants.CASES (the cases of test_kernel_variants_gpu.py and test_fused_variants_gpu.py).  A template
instantiation added later without a case fails here, on a machine without a GPU.

The backward units of the fused point layers (fusion_grad, cross_grad, cross256_grad, pointconv_grad, ptblock_grad) are held the same
way: every kernel they emit must be in kernel_variants.expected_grad_kernels of at least one entry of GRAD_CASES (the cases of
test_fused_grad_variants_gpu.py) or in GRAD_NOT_LAUNCHED with its reason, and GRAD_EDGES states, as predicates on the mirrored launch
(kernel_variants.grad_launch_grid at 256 compute units), every edge of their persistent loops that the cases must reach.

The train-mode fusion layer (fusion_bn: forward and backward passes in one unit) likewise: every kernel it emits must be in
kernel_variants.expected_bn_kernels of at least one entry of BN_CASES (the cases of test_fusion_bn_variants_gpu.py, which hold the unit
to float64 at its loop edges) or in BN_NOT_LAUNCHED, and BN_EDGES states the edges of its two grid caps on kernel_variants.bn_launch_grid.

The weight-gradient kernel of the per-point Linear (linear_grad) too: every linear_wgrad_kernel instantiation must be what
kernel_variants.wgrad_launch names for an entry of WGRAD_CASES (the cases of test_linear_grad_edges_gpu.py), and WGRAD_EDGES states the
staging forms, stage counts and tile splits the cases must reach.  The narrow-head attention backward (attention_grad) has no variants
to pick from -- one kernel per head width -- so ATTN_GRAD_EDGES only states which query / key counts
kernel_variants.ATTN_GRAD_COUNTS must hold, as predicates on kernel_variants.attention_small_grad_launch.

The wide-head attention in a training graph (attention_wide_grad: 43 instantiations over head width, dropout, per-element lengths and
the forward's key split): every kernel must be in kernel_variants.attention_wide_train_kernels of the crossed grid WIDE_GRAD_COUNTS or of
an entry of WIDE_GUARD_CASES / WIDE_TRAIN_CASES (the cases of test_attention_wide_grad_edges_gpu.py), WIDE_TRAIN_REQUIRED states which
explicit cases must be there, and WIDE_GRAD_EDGES states, as predicates on kernel_variants.attention_wide_grad_launch, the tile, block
and stage boundaries the grid must hold.  The EMD backward and the interpolation weights' backward (emd_grad: 7 kernels, interp3_grad: 1)
are held by EMD_GRAD_CASES / INTERP3_GRAD_CASES (the cases of test_emd_interp3_grad_edges_gpu.py), each of which names the kernels it
launches.  With these, every backward unit of the library has a mirror, a registry test and cases on its own loop edges."""
import os
import re
import shutil
import subprocess

import pytest

from tests import kernel_variants as kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mocopci_amd", "csrc")
UNITS = ("linear", "mlp", "attention", "fusion", "cross", "pointconv", "ptblock")
# Emitted kernels that the shipped dispatch cannot launch, by name, each with its reason.  Empty today: fusion_kernel (the f32-input
# MFMA form of fusion.hip, launched only under -DMCP_AB) is not compiled into the shipped library at all.
NOT_LAUNCHED = {}
GRAD_UNITS = ("fusion_grad", "cross_grad", "cross256_grad", "pointconv_grad", "ptblock_grad")
GRAD_NOT_LAUNCHED = {}   # the same for the backward units: every kernel they emit is launched by some backward call
BN_UNITS = ("fusion_bn",)
BN_NOT_LAUNCHED = {}     # and for the train-mode fusion layer: all 13 kernels are launched by a forward or a backward entry point


def emitted_kernels(units=UNITS):
    """Demangled kernel names of the units' device assembly, without namespace, return type and arguments."""
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("no hipcc: the device assembly cannot be generated on this machine")
    if not shutil.which("c++filt"):
        pytest.skip("no c++filt to demangle the kernel names")
    subprocess.check_call(["make", "-C", CSRC, "-j3", "-s"] + [f"isa/{u}.s" for u in units])
    mangled = []
    for u in units:
        with open(os.path.join(CSRC, "isa", f"{u}.s")) as f:
            mangled += re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), re.M)
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    names = set()
    for line in out[:len(mangled)]:
        line = re.sub(r"^void\s+", "", line.strip()).replace("(anonymous namespace)::", "")
        depth, end = 0, len(line)
        for i, ch in enumerate(line):       # cut the argument list: the first '(' outside the template brackets
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                end = i
                break
        names.add(line[:end])
    return names


def test_expected_kernel_mirrors_the_dispatch_rules():
    # spot checks of the C conditions the mirror encodes (linear.hip:415-435, :554; mlp.hip:214-220; attention_wide_fwd.h: wide_keys_split)
    e = kv.expected_kernel
    assert e("linear", rows=131072, ks=(256,), n=32) == "linear_kernel<1, 4, 8>"
    assert e("linear", rows=131071, ks=(256,), n=32) == "linear_kernel<1, 4, 4>"
    assert e("linear", rows=131072, ks=(224,), n=32) == "linear_kernel<1, 1, 8>"
    assert e("linear", rows=20000, ks=(36, 36), n=70) == "linear_kernel<3, 2, 4>"    # 2 + 2 chunks
    assert e("linear", rows=20000, ks=(72,), n=70) == "linear_kernel<3, 1, 4>"       # 3 chunks
    assert e("linear", rows=200000, ks=(64,), n=250) == "linear_kernel<8, 1, 4>"
    assert e("linear", rows=200000, ks=(64,), n=512) == "linear_kernel<4, 1, 8>"
    assert e("linear", rows=6000, ks=(128,), n=96, policy_rows=196608) == "linear_kernel<3, 2, 4>"
    assert e("linear", rows=6000, ks=(128,), n=96) == "linear_splitk_kernel<1>"
    assert e("linear", rows=6000, ks=(96,), n=96) == "linear_kernel<3, 1, 4>"        # 3 chunks: no split-K
    assert e("mlp2", rows=32767, cin=128, hidden=512, cout=97) == "mlp2_kernel<128, 4, 4>"
    assert e("mlp2", rows=32768, cin=64, hidden=512, cout=64) == "mlp2_kernel<64, 2, 8>"
    assert e("attention", bf=16, nq=256, nk=256, heads=4, hd=256) == "attention_wide_ksplit_kernel<256>"
    assert e("attention", bf=16, nq=512, nk=256, heads=4, hd=256) == "attention_wide_kernel<256>"
    assert e("attention", bf=2, nq=100, nk=127, heads=1, hd=256) == "attention_wide_kernel<256>"
    for bad in (dict(op="linear", rows=20000, ks=(64,), n=130), dict(op="mlp2", rows=100, cin=128, hidden=512, cout=64),
                dict(op="attention", bf=1, nq=1, nk=1, heads=1, hd=128)):
        with pytest.raises(ValueError):
            kv.expected_kernel(**bad)


def test_expected_kernel_mirrors_the_fused_dispatch_rules():
    # pointconv_tile.h: pc_agg_run, pc_linear_run; mcp_cross_volume (cross.hip); fusion.hip:291, :318; ptblock.hip:188, :197
    e = kv.expected_kernel
    agg = lambda total, d, **kw: e("pointconv_agg", b=1, s=total, d=d, **kw)
    assert agg(16384, 32) == "pointconv_agg_lowlevel_kernel<256>"
    assert agg(16385, 32) == "pointconv_agg_kernel<256, 32>"
    assert e("pointconv_agg", b=5, s=3277, d=32) == "pointconv_agg_kernel<256, 32>"      # b * s = 16385
    assert e("pointconv_agg", b=4, s=4096, d=32) == "pointconv_agg_lowlevel_kernel<256>"  # b * s = 16384
    assert agg(16385, 32, aligned=False) == "pointconv_agg_lowlevel_kernel<256>"          # s_points off a 16-byte boundary
    assert agg(16385, 5) == agg(16385, 34) == "pointconv_agg_lowlevel_kernel<256>"        # d % 4
    assert agg(200000, 4) == "pointconv_agg_kernel<256, 32>"
    assert agg(16385, 36) == agg(16385, 64) == "pointconv_agg_kernel<256, 16>"
    assert agg(16385, 68) == agg(16385, 256) == agg(16385, 512) == "pointconv_agg_kernel<256, 8>"
    assert agg(8192, 256) == agg(100, 512) == "pointconv_agg_lowlevel_kernel<1024>"
    assert agg(8193, 256) == agg(8192, 252) == "pointconv_agg_lowlevel_kernel<256>"
    assert agg(8192, 258, aligned=False) == "pointconv_agg_lowlevel_kernel<1024>"
    assert agg(16384, 258) == agg(20000, 258) == "pointconv_agg_lowlevel_kernel<256>"
    assert e("pointconv_linear", d=32, c_out=32) == "pointconv_linear_kernel<32, 1>"
    assert e("pointconv_linear", d=64, c_out=64) == "pointconv_linear_kernel<64, 2>"
    assert e("cross", d=64) == "cross_kernel<64, 1>" and e("cross", d=128) == "cross_kernel<128, 1>"
    assert e("cross", d=256) == "cross256_stream_kernel"
    assert e("fusion", b=2, n=1500) == "fusion_split_kernel" and e("ptblock") == "ptblock_kernel"
    for bad in (dict(op="pointconv_linear", d=32, c_out=64), dict(op="pointconv_linear", d=128, c_out=128), dict(op="cross", d=32),
                dict(op="cross", d=64, k=16), dict(op="fusion", b=1, n=1, nb=32), dict(op="ptblock", c=128), dict(op="pointconv_agg", b=1, s=1, d=4, k=16)):
        with pytest.raises(ValueError):
            kv.expected_kernel(**bad)
    # the grids beside the dispatch: fusion.hip:304, launch_cross256 and launch_cross (cross.hip), pointconv_tile.h: pc_agg_run, pc_linear_run, ptblock.hip:193-194
    g = kv.launch_grid
    assert g("fusion", b=2, n=1500)[0] == 750 and g("fusion", b=3, n=5483)[0] == 4096 and g("fusion", b=1, n=1)[0] == 1
    assert g("cross", d=64, b=2, n1=2048)[0] == 128 and g("cross", d=64, b=40, n1=2048)[0] == 768
    assert g("cross", d=128, b=2, n1=512)[0] == 16 and g("cross", d=128, b=40, n1=2048)[0] == 256
    assert g("cross", d=256, b=2, n1=256)[0] == 128 and g("cross", d=256, b=2, n1=37)[0] == 19 and g("cross", d=256, b=8, n1=512)[0] == 256
    assert g("pointconv_agg", b=2, s=8192, d=32)[::2] == (2048, 8) and g("pointconv_agg", b=5, s=3277, d=32)[::2] == (513, 32)
    assert g("pointconv_agg", b=5, s=3277, d=64)[::2] == (1025, 16) and g("pointconv_agg", b=5, s=3277, d=128)[::2] == (2049, 8)
    assert g("pointconv_linear", b=2, s=8200, d=64, c_out=64)[0] == 513
    assert g("ptblock", b=2, n=2048) == (128, 2048, 4) and g("ptblock", b=3, n=8183) == (768, 12275, 4) and g("ptblock", b=1, n=1)[0] == 1


def _by_xcd(case):
    """(dealt by XCD, units per eighth, units per workgroup step) of a case's launch: mcp_units_by_xcd (common.h), cross_kernel's own deal (cross.hip)."""
    grid, units, per = kv.launch_grid(**case)
    xcd = grid % 8 == 0 and not (case["op"] == "cross" and case["d"] == 256)
    if not xcd:
        return False, units, grid * per
    if case["op"] == "cross":
        return True, (units + 7) // 8, grid // 8 * per
    return True, ((units + per - 1) // per + 7) // 8 * per, grid // 8 * per


def test_the_fused_cases_reach_the_loop_edges_their_comments_name():
    """The edges of the persistent loops that the issue behind these cases lists, checked on the mirrored grid arithmetic."""
    def some(op, pred, **match):
        return any(pred(c, *_by_xcd(c), *kv.launch_grid(**c)) for c in kv.cases(op) if all(c.get(k) == v for k, v in match.items()))
    ragged_xcd = lambda c, xcd, chunk, step, grid, units, per: xcd and units % chunk and units % 8
    rounds = lambda c, xcd, chunk, step, grid, units, per: (chunk if xcd else units) > step
    no_xcd = lambda c, xcd, chunk, step, grid, units, per: grid > 1 and not xcd
    for d in (64, 128):
        assert some("cross", lambda c, xcd, chunk, *_: ragged_xcd(c, xcd, chunk, *_) and chunk % c["n1"], d=d)       # (a)
        assert some("cross", lambda c, xcd, chunk, step, grid, *_: xcd and grid == kv.CROSS_GRID_CAP[d] and step >= c["n1"] and chunk > 2 * step, d=d)  # (b)
        assert some("cross", no_xcd, d=d)                                                                         # (c)
        assert some("cross", lambda c, xcd, chunk, step, grid, units, per: units < per, d=d)                      # (d)
        assert some("cross", lambda c, *_: c["n1"] != c["n2"], d=d)                                               # (e)
    assert some("cross", lambda c, xcd, chunk, step, grid, units, per: grid == 256 and units > 2 * step and units % per and step >= c["n1"], d=256)
    assert some("cross", lambda c, xcd, chunk, step, grid, units, per: 1 < grid < 256 and units % per, d=256)
    assert some("cross", lambda c, xcd, chunk, step, grid, units, per: units < per, d=256)
    assert some("fusion", lambda c, *a: rounds(c, *a) and c["b"] * c["n"] > 4 * 4096) and some("fusion", ragged_xcd) and some("fusion", no_xcd)
    assert {c["b"] * c["n"] for c in kv.cases("fusion")} >= {1, 3, 5}
    assert some("fusion", lambda c, *_: c.get("same")) and some("fusion", lambda c, *_: c.get("dup"))
    odd = lambda c: (c["b"] * c["n"]) % 2 == 1
    assert some("ptblock", lambda c, *_: odd(c) and c["b"] == 1 and c["n"] > 1) and some("ptblock", lambda c, *_: odd(c) and c["b"] == 3)
    assert some("ptblock", lambda c, *_: c["b"] * c["n"] == 1)
    assert some("ptblock", lambda c, xcd, chunk, step, grid, units, per: grid == kv.PTBLOCK_GRID_CAP and odd(c) and units % chunk and chunk > step)
    # fewer workgroups than steps, and a step count that is no multiple of 8: the eighths are rounded up to whole steps
    assert some("ptblock", lambda c, xcd, chunk, step, grid, units, per: xcd and grid < kv.PTBLOCK_GRID_CAP and -(-units // per) % 8 and units % chunk)
    assert some("ptblock", lambda c, *_: c.get("packed")) and some("ptblock", lambda c, *_: c.get("logits") == 80.0)
    assert some("ptblock", lambda c, *_: c.get("same"))
    stream = lambda ppb: f"pointconv_agg_kernel<256, {ppb}>"
    names = lambda **m: {kv.expected_kernel(**c) for c in kv.cases("pointconv_agg") if all(c.get(k) == v for k, v in m.items())}
    totals = {c["b"] * c["s"]: kv.expected_kernel(**c) for c in kv.cases("pointconv_agg") if c["d"] == 32 and c.get("aligned", True)}
    assert totals[16384] == "pointconv_agg_lowlevel_kernel<256>" and totals[16385] == stream(32)
    assert names(d=32) >= {stream(32)} and names(d=4) == {stream(32)} and names(d=36) == names(d=64) == {stream(16)}
    assert names(d=128) == names(d=256, b=1) == {stream(8)} and "pointconv_agg_lowlevel_kernel<1024>" in names(d=256)
    assert names(aligned=False) == names(d=5) == {"pointconv_agg_lowlevel_kernel<256>"}
    streaming = [c for c in kv.cases("pointconv_agg") if "lowlevel" not in kv.expected_kernel(**c)]
    assert all(kv.launch_grid(**c)[1] % kv.launch_grid(**c)[2] for c in streaming)          # a last workgroup with fewer than PPB points
    assert {kv.launch_grid(**c)[0] % 8 == 0 for c in streaming} == {True, False}
    assert {c["s"] == c["n"] for c in streaming} == {True, False}
    for name in ("pointconv_linear_kernel<32, 1>", "pointconv_linear_kernel<64, 2>"):
        mine = [c for c in kv.cases("pointconv_linear") if kv.expected_kernel(**c) == name]
        assert {c["b"] * c["s"] > 16384 for c in mine} == {True, False} and all((c["b"] * c["s"]) % 32 for c in mine)
    for op in ("fusion", "cross", "pointconv_agg", "pointconv_linear", "ptblock"):
        assert some(op, lambda c, *_: c.get("extent")), op                                  # coordinates of a real cloud's extent


def test_every_case_names_a_kernel_and_ids_are_unique():
    ids = [kv.case_id(c) for c in kv.CASES]
    assert len(set(ids)) == len(ids)


def test_every_dense_kernel_instantiation_has_a_parity_case():
    emitted = emitted_kernels()
    assert any(n.startswith("linear_kernel<") for n in emitted), sorted(emitted)   # the demangling worked
    assert "ptblock_kernel" in emitted and "cross_kernel<64, 1>" in emitted, sorted(emitted)
    unknown = sorted(set(NOT_LAUNCHED) - emitted)
    assert not unknown, f"NOT_LAUNCHED names kernels the library does not build: {unknown}"
    wanted = {n for n in emitted if not n.split("<")[0].endswith("_pack_kernel") and n not in NOT_LAUNCHED}
    covered = {kv.expected_kernel(**c) for c in kv.CASES}
    missing = sorted(wanted - covered)
    assert not missing, f"kernel instantiations without a parity case in tests/kernel_variants.py CASES: {missing}"
    stale = sorted(covered - wanted)
    assert not stale, f"cases name kernels the library does not build: {stale}"


# ---- the backward units of the fused point layers ------------------------------------------------------------------------------------
CUS = 256   # compute units of the MI355X: the grid cap of every backward kernel


def test_the_backward_mirror_follows_the_c_conditions():
    # grad_grid / plan: fusion_grad.hip:440-445, grad_grid (cross_grad.hip), plan (cross256_grad.hip), pointconv_grad.hip:204-208,
    # ptblock_grad.hip:417-421; the deals: mcp_units_by_xcd (common.h), cross_grad_kernel's deal() (cross_grad.hip); the rounds of
    # cross256_grad_z_kernel, the slices of cross256_grad_w_kernel, the point loop of cross256_grad_dx_kernel
    g, e = kv.grad_launch_grid, kv.expected_grad_kernels
    fus = lambda total, **kw: g("fusion", b=1, n=total, **kw)["points"]
    assert fus(1024)["workgroups"] == 256 and fus(1024)["by_xcd"] and fus(1020)["workgroups"] == 255 and not fus(1020)["by_xcd"]
    assert fus(100000)["workgroups"] == 256 and fus(100000, cus=304)["workgroups"] == 304 and fus(2000, cus=304)["workgroups"] == 304
    assert fus(29)["workgroups"] == 8 and fus(29)["by_xcd"] and fus(28)["workgroups"] == 7
    r = fus(1025)   # steps 257, eighths of 33 steps = 132 points; workgroup 8 j + x starts at 132 x + 4 j and strides 128
    assert r["dealt"][7][0] == [924, 925, 926, 927] and r["dealt"][7 + 8 * 25] == [[1024]] and r["dealt"][7 + 8 * 26] == []
    assert r["dealt"][0] == [[0, 1, 2, 3], [128, 129, 130, 131]] and r["dealt"][8 * 2] == [[8, 9, 10, 11]]
    assert fus(5)["dealt"] == [[[0, 1, 2, 3]], [[4]]]
    x128 = lambda total, **kw: g("cross", d=128, b=1, n1=total, **kw)
    roles = lambda t: [(v["workgroups"], v["by_xcd"]) for v in x128(t).values()]
    assert roles(400) == [(100, False), (64, False), (64, False)]      # base 100: the own-row roles cannot go by XCD
    assert roles(384) == [(96, True), (64, True), (64, True)] and roles(288) == [(72, True), (64, True), (64, True)]
    assert roles(272) == [(68, False), (64, False), (64, False)] and roles(40) == [(10, False)] * 3 and roles(3) == [(1, False)] * 3
    assert roles(32) == [(8, True)] * 3 and roles(5000) == [(128, True), (64, True), (64, True)]
    assert [v["workgroups"] for v in x128(5000, cus=304).values()] == [152, 76, 76]
    assert x128(400)["own0"]["dealt"][1] == [[4, 5, 6, 7], [260, 261, 262, 263]]
    assert g("cross", d=64, b=1, n1=5000)["all"]["workgroups"] == 256 and g("cross", d=64, b=2, n1=31)["all"]["by_xcd"]
    x256 = lambda total, **kw: g("cross", d=256, b=1, n1=total, **kw)
    sizes = lambda t: tuple(x256(t)[k]["workgroups"] for k in ("z", "w", "dx"))
    assert sizes(3) == (1, 1, 3) and sizes(8) == (2, 1, 8) and sizes(9) == (3, 2, 9) and sizes(511) == (128, 64, 511)
    assert sizes(513) == (129, 64, 512) and sizes(1025) == (256, 64, 512) and tuple(x256(5000, cus=304)[k]["workgroups"] for k in ("z", "w", "dx")) == (256, 64, 512)
    assert not x256(1024)["z"]["by_xcd"] and x256(1025)["z"]["dealt"][0] == [[0, 1, 2, 3], [1024]]
    w = x256(1025)["w"]["dealt"]    # slices of 17 points in stages of 4
    assert w[0] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16]] and w[60] == [[1020, 1021, 1022, 1023], [1024]] and w[61] == w[63] == []
    assert x256(1025)["dx"]["dealt"][0] == [[0], [512], [1024]] and x256(1025)["dx"]["dealt"][1] == [[1], [513]]
    agg = lambda total, **kw: g("pointconv_agg", b=1, s=total, **kw)["pairs"]
    assert (agg(2048)["workgroups"], agg(2048)["units"]) == (256, 1024) and (agg(2049)["workgroups"], agg(2049)["units"]) == (256, 1025)
    assert agg(9)["dealt"] == [[[0, 1, 2, 3]], [[4]]] and agg(1)["dealt"] == [[[0]]] and agg(2040)["workgroups"] == 255
    ptb = lambda total, **kw: g("ptblock", b=1, n=total, **kw)["pairs"]
    assert (ptb(2049)["workgroups"], ptb(2049)["units"]) == (256, 1025) and ptb(1)["dealt"] == [[[0]]] and ptb(122)["workgroups"] == 16 and ptb(122)["by_xcd"]
    assert e("cross", d=128) == {"cross_grad_kernel<128>", "transposed_image_kernel", "cross_grad_reduce_kernel"}
    assert e("cross", d=64) == {"cross_grad_kernel<64>", "cross_grad_reduce_kernel"} and len(e("cross", d=256)) == 4
    assert e("fusion", b=1, n=1) == {"fusion_grad_kernel", "fusion_grad_reduce_kernel"} and "ptblock_transposed_images_kernel" in e("ptblock")
    for bad in (dict(op="cross", d=32), dict(op="pointconv_agg", b=1, s=1, d=5), dict(op="pointconv_agg", b=1, s=1, d=260), dict(op="fusion", b=1, n=1, nb=32)):
        with pytest.raises(ValueError):
            e(**bad)


def test_the_backward_mirror_deals_every_unit_to_exactly_one_workgroup_of_each_role():
    for c in kv.GRAD_CASES:
        for name, role in kv.grad_launch_grid(cus=CUS, **c).items():
            flat = sorted(u for wg in role["dealt"] for rnd in wg for u in rnd)
            assert flat == list(range(role["units"])), (kv.grad_case_id(c), name)
            assert len(role["dealt"]) == role["workgroups"] and all(len(rnd) <= role["per"] for wg in role["dealt"] for rnd in wg)


def _rounds(role):
    return max(len(wg) for wg in role["dealt"])


def _idle(role):
    return sum(1 for wg in role["dealt"] if not wg)


def _want(role):
    return -(-role["units"] // role["per"])


def _ragged_eighth(role):
    """Dealt by XCD with a last eighth shorter than the others."""
    chunk = -(-_want(role) // 8) * role["per"]
    return role["by_xcd"] and role["units"] % chunk != 0


def _dead_waves(role):
    """Some workgroup takes a step with fewer units than waves."""
    return any(len(rnd) < role["per"] for wg in role["dealt"] for rnd in wg)


def _points(c):
    return c["b"] * c[{"fusion": "n", "cross": "n1", "pointconv_agg": "s", "ptblock": "n"}[c["op"]]]


def _ladder(role_name, units_are_pairs=False):
    """The edges every one-role kernel shares."""
    R = lambda g: g[role_name]
    return {
        "by XCD below the cap with a ragged last eighth": lambda c, g: R(g)["workgroups"] < CUS and _ragged_eighth(R(g)) and (not units_are_pairs or _points(c) % 2 == 1 or c["op"] == "ptblock"),
        "first total above the cap: a second round that few workgroups take, and workgroups that receive nothing":
            lambda c, g: R(g)["workgroups"] == CUS and _want(R(g)) == CUS + 1 and _rounds(R(g)) == 2 and _idle(R(g)) > 0,
        "three or more rounds at the cap with a ragged last eighth": lambda c, g: R(g)["workgroups"] == CUS and _rounds(R(g)) >= 3 and _ragged_eighth(R(g)),
    }


GRAD_EDGES = {
    ("fusion", None): {
        "one point": lambda c, g: _points(c) == 1,
        "three points: one workgroup with a dead wave": lambda c, g: _points(c) == 3 and g["points"]["workgroups"] == 1,
        "five points: the second of two workgroups has one live wave": lambda c, g: g["points"]["dealt"] == [[[0, 1, 2, 3]], [[4]]],
        "round-robin below the cap, a grid that is no multiple of 8, more than one batch element":
            lambda c, g: 8 < g["points"]["workgroups"] < CUS and g["points"]["workgroups"] % 8 and c["b"] >= 2 and not c.get("same"),
        "same and dup at a small total": lambda c, g: c.get("same") and c.get("dup") and _points(c) <= 64,
        "coordinates of a real cloud's extent": lambda c, g: c.get("extent"),
        **_ladder("points"),
    },
    ("cross", 64): {
        "three points: one workgroup with a dead wave": lambda c, g: _points(c) == 3,
        "round-robin below the cap": lambda c, g: 1 < g["all"]["workgroups"] < CUS and not g["all"]["by_xcd"] and c["b"] >= 2,
        "coordinates of a real cloud's extent": lambda c, g: c.get("extent"),
        **_ladder("all"),
    },
    ("cross", 128): {
        "three points: three workgroups, one per role": lambda c, g: _points(c) == 3 and [r["workgroups"] for r in g.values()] == [1, 1, 1],
        "all roles round-robin with equal grids": lambda c, g: len({r["workgroups"] for r in g.values()}) == 1 and g["data"]["workgroups"] > 1 and not any(r["by_xcd"] for r in g.values()),
        "data role by XCD below its cap, own-row roles at their cap by XCD, a ragged eighth":
            lambda c, g: g["data"]["by_xcd"] and g["data"]["workgroups"] < CUS // 2 and g["own0"]["workgroups"] == g["own2"]["workgroups"] == CUS // 4
            and g["own0"]["by_xcd"] and g["own2"]["by_xcd"] and _ragged_eighth(g["data"]),
        "data role round-robin forces the own-row roles round-robin through their base":
            lambda c, g: not g["data"]["by_xcd"] and g["own0"]["workgroups"] % 8 == 0 and g["own0"]["workgroups"] >= 8 and not g["own0"]["by_xcd"] and not g["own2"]["by_xcd"],
        "all roles at their cap by XCD with different round counts (3 or more) and a ragged eighth":
            lambda c, g: [r["workgroups"] for r in g.values()] == [CUS // 2, CUS // 4, CUS // 4] and all(r["by_xcd"] for r in g.values())
            and 3 <= _rounds(g["data"]) < _rounds(g["own0"]) == _rounds(g["own2"]) and _ragged_eighth(g["data"]),
        "coordinates of a real cloud's extent": lambda c, g: c.get("extent"),
    },
    ("cross", 256): {
        "three points: a dead wave in z, one slice of w, total below DX_GRID": lambda c, g: _points(c) == 3 and g["w"]["workgroups"] == 1 and g["dx"]["workgroups"] == 3,
        "z below its cap with a ragged last workgroup": lambda c, g: 1 < g["z"]["workgroups"] < kv.X256_Z_GRID_CAP and len(g["z"]["dealt"][-1][-1]) < 4,
        "z: the first total above 4 x 256": lambda c, g: g["z"]["units"] == 4 * kv.X256_Z_GRID_CAP + 1 and _rounds(g["z"]) == 2,
        "z: three rounds with dead waves in the last": lambda c, g: _rounds(g["z"]) == 3 and _dead_waves(g["z"]) and c["n1"] < 4 * kv.X256_Z_GRID_CAP,
        "w: a last slice shorter than the others, with a partial stage": lambda c, g: g["w"]["workgroups"] > 1 and [len(s) for s in g["w"]["dealt"] if s][-1:] != [len(g["w"]["dealt"][0])]
            and len([s for s in g["w"]["dealt"] if s][-1][-1]) < kv.X256_W_PTS,
        "w: slices that receive nothing": lambda c, g: _idle(g["w"]) > 0,
        "dx: total below DX_GRID": lambda c, g: 1 < g["dx"]["units"] < kv.X256_DX_GRID,
        "dx: total above DX_GRID, workgroups with different point counts": lambda c, g: g["dx"]["units"] > kv.X256_DX_GRID and len({len(wg) for wg in g["dx"]["dealt"]}) > 1,
        "coordinates of a real cloud's extent": lambda c, g: c.get("extent"),
    },
    ("pointconv_agg", None): {
        "one centre: the tail alone": lambda c, g: _points(c) == 1,
        "nine centres: the second of two workgroups has the half pair": lambda c, g: _points(c) == 9 and g["pairs"]["dealt"] == [[[0, 1, 2, 3]], [[4]]],
        "an odd tail with more than one batch element at the cap": lambda c, g: _points(c) % 2 == 1 and c["b"] >= 2 and g["pairs"]["workgroups"] == CUS,
        "S = N": lambda c, g: c["s"] == c["n"],
        "S < N": lambda c, g: c["s"] < c["n"],
        "d = 32": lambda c, g: c["d"] == 32,
        "d = 64": lambda c, g: c["d"] == 64,
        "d = 128": lambda c, g: c["d"] == 128,
        "coordinates of a real cloud's extent": lambda c, g: c.get("extent"),
        **_ladder("pairs", units_are_pairs=True),
    },
    ("ptblock", None): {
        "one point: the tail alone": lambda c, g: _points(c) == 1,
        "an odd total in one batch element": lambda c, g: _points(c) % 2 == 1 and c["b"] == 1 and c["n"] > 1,
        "an odd total in three batch elements: pairs straddle them": lambda c, g: _points(c) % 2 == 1 and c["b"] == 3 and c["n"] % 2 == 1,
        "q, k, v packed with row stride 192": lambda c, g: c.get("packed"),
        "a uniform softmax": lambda c, g: c.get("same"),
        "logits of 80": lambda c, g: c.get("logits") == 80.0,
        "coordinates of a real cloud's extent": lambda c, g: c.get("extent"),
        **_ladder("pairs", units_are_pairs=True),
    },
}


def grad_cases_reaching(key, edge):
    op, d = key
    mine = [c for c in kv.grad_cases(op) if d is None or c["d"] == d]
    return [kv.grad_case_id(c) for c in mine if GRAD_EDGES[key][edge](c, kv.grad_launch_grid(cus=CUS, **c))]


def test_the_backward_cases_reach_the_loop_edges():
    """Every edge of GRAD_EDGES is reached by at least one case on the mirrored launch at 256 compute units; n1 != n2 in every cross case."""
    missing = [f"{key}: {edge}" for key, edges in GRAD_EDGES.items() for edge in edges if not grad_cases_reaching(key, edge)]
    assert not missing, missing
    assert all(c["n1"] != c["n2"] for c in kv.grad_cases("cross"))
    assert {c["op"] for c in kv.GRAD_CASES} == {key[0] for key in GRAD_EDGES}
    ids = [kv.grad_case_id(c) for c in kv.GRAD_CASES]
    assert len(set(ids)) == len(ids)


def test_every_backward_kernel_of_the_fused_layers_has_a_parity_case():
    emitted = emitted_kernels(GRAD_UNITS)
    assert "cross_grad_kernel<128>" in emitted and "fusion_grad_kernel" in emitted, sorted(emitted)   # the demangling worked
    unknown = sorted(set(GRAD_NOT_LAUNCHED) - emitted)
    assert not unknown, f"GRAD_NOT_LAUNCHED names kernels the library does not build: {unknown}"
    wanted = emitted - set(GRAD_NOT_LAUNCHED)
    covered = set().union(*(kv.expected_grad_kernels(**c) for c in kv.GRAD_CASES))
    missing = sorted(wanted - covered)
    assert not missing, f"backward kernels without a parity case in tests/kernel_variants.py GRAD_CASES: {missing}"
    stale = sorted(covered - wanted)
    assert not stale, f"backward cases name kernels the library does not build: {stale}"


# ---- the fusion layer on batch statistics: two grid caps in one call --------------------------------------------------------------------
def test_the_batch_statistics_mirror_follows_the_c_conditions():
    # fwd_grid, fusion_bn.hip:377-382; bwd_grid :1179-1184 with per_cu 2 (B1, B4: :1326, :1351) and 1 (B2, B3: :1337, :1344); the deal: mcp_units_by_xcd (common.h)
    g, e = kv.bn_launch_grid, kv.expected_bn_kernels
    sizes = lambda total, **kw: tuple((r["workgroups"], r["by_xcd"]) for r in g(b=1, n=total, **kw).values())
    assert sizes(1) == ((1, False), (1, False)) and sizes(5) == ((2, False), (2, False)) and sizes(61) == ((16, True), (16, True))
    assert sizes(1024) == ((256, True), (256, True)) and sizes(1025) == ((257, False), (256, True)) and sizes(2048) == ((512, True), (256, True))
    assert sizes(2049) == ((512, True), (256, True)) and sizes(100000) == ((512, True), (256, True)) and sizes(100000, cus=304) == ((608, True), (304, True))
    at1402 = g(b=2, n=701)   # the one shape test_grad_gpu.py runs: only B2 / B3 exceed their cap, nothing is dealt by XCD in the wide passes, nobody idles
    assert sizes(1402) == ((351, False), (256, True)) and not any(not wg for r in at1402.values() for wg in r["dealt"])
    n = g(b=5, n=205)["narrow"]    # 257 steps, eighths of 33 steps = 132 points; workgroup 8 j + x starts at 132 x + 4 j and strides 128
    assert n["dealt"][0] == [[0, 1, 2, 3], [128, 129, 130, 131]] and n["dealt"][7 + 8 * 25] == [[1024]] and n["dealt"][7 + 8 * 26] == [] and n["dealt"][255] == []
    w = g(b=3, n=683)["wide"]      # 513 steps, eighths of 65 steps = 260 points; workgroup 8 j + x starts at 260 x + 4 j and strides 256
    assert w["dealt"][0] == [[0, 1, 2, 3], [256, 257, 258, 259]] and w["dealt"][8] == [[4, 5, 6, 7]] and w["dealt"][7] == [[1820, 1821, 1822, 1823]]
    assert w["dealt"][7 + 8 * 57] == [[2048]] and w["dealt"][7 + 8 * 58] == [] and w["dealt"][511] == []
    assert g(b=1, n=5)["wide"]["dealt"] == [[[0, 1, 2, 3]], [[4]]]
    assert len(e(b=1, n=1)) == 13 and len(e(b=1, n=1, forward_only=True)) == 6
    with pytest.raises(ValueError):
        e(b=1, n=1, nb=32)


def test_the_batch_statistics_mirror_deals_every_point_to_exactly_one_workgroup_of_each_role():
    for c in kv.BN_CASES:
        for name, role in kv.bn_launch_grid(cus=CUS, **c).items():
            flat = sorted(u for wg in role["dealt"] for rnd in wg for u in rnd)
            assert flat == list(range(c["b"] * c["n"])), (kv.bn_case_id(c), name)
            assert len(role["dealt"]) == role["workgroups"] and all(len(rnd) <= role["per"] for wg in role["dealt"] for rnd in wg)


def _bn_ladder(role_name, cap, rounds):
    """The edges of one grid cap: the role's passes all launch min(ceil(total / 4), cap) workgroups."""
    R = lambda g: g[role_name]
    return {
        f"{role_name}: a launch with fewer points than a workgroup has waves": lambda c, g: R(g)["units"] < R(g)["per"],
        f"{role_name}: a round-robin grid of more than one workgroup": lambda c, g: R(g)["workgroups"] > 1 and not R(g)["by_xcd"],
        f"{role_name}: by XCD below the cap with a ragged last eighth": lambda c, g: R(g)["workgroups"] < cap and _ragged_eighth(R(g)),
        f"{role_name}: the first total above the cap, with workgroups that receive nothing and must still write a zero partial row":
            lambda c, g: R(g)["workgroups"] == cap and _want(R(g)) == cap + 1 and _idle(R(g)) > 0 and _rounds(R(g)) == 2,
        f"{role_name}: {rounds} or more rounds at the cap with a ragged last eighth":
            lambda c, g: R(g)["workgroups"] == cap and _rounds(R(g)) >= rounds and _ragged_eighth(R(g)),
    }


BN_EDGES = {
    **_bn_ladder("wide", 2 * CUS, 2),
    **_bn_ladder("narrow", CUS, 4),
    "only B2 / B3 above their cap: idle workgroups there, a round-robin grid in the wide passes of the same call":
        lambda c, g: _idle(g["narrow"]) > 0 and not g["wide"]["by_xcd"] and g["wide"]["workgroups"] == CUS + 1,
    "the wide passes above their cap with idle workgroups while B2 / B3 run three rounds": lambda c, g: _idle(g["wide"]) > 0 and _rounds(g["narrow"]) == 3,
    "one point": lambda c, g: c["b"] * c["n"] == 1,
    "five points: the second of two workgroups has one live wave": lambda c, g: g["wide"]["dealt"] == g["narrow"]["dealt"] == [[[0, 1, 2, 3]], [[4]]],
    "round-robin below both caps with more than one batch element": lambda c, g: not g["wide"]["by_xcd"] and g["wide"]["workgroups"] < CUS and c["b"] >= 2 and not c.get("same"),
    "same and dup at a small total": lambda c, g: c.get("same") and c.get("dup") and c["b"] * c["n"] <= 64,
    "coordinates of a real cloud's extent": lambda c, g: c.get("extent"),
    "a conv output far from its bias, forward only": lambda c, g: c.get("far") and c.get("forward_only"),
}


def bn_cases_reaching(edge):
    return [kv.bn_case_id(c) for c in kv.BN_CASES if BN_EDGES[edge](c, kv.bn_launch_grid(cus=CUS, **c))]


def test_the_batch_statistics_cases_reach_the_loop_edges():
    """Every edge of BN_EDGES is reached by at least one case on the mirrored launch at 256 compute units."""
    missing = [edge for edge in BN_EDGES if not bn_cases_reaching(edge)]
    assert not missing, missing
    ids = [kv.bn_case_id(c) for c in kv.BN_CASES]
    assert len(set(ids)) == len(ids)
    assert sum(1 for c in kv.BN_CASES if not c.get("forward_only")) >= 9      # the backward runs at every case but `far`


def test_every_kernel_of_the_batch_statistics_fusion_layer_has_a_parity_case():
    emitted = emitted_kernels(BN_UNITS)
    assert "fusion_bn_fwd_kernel<0, true>" in emitted and "sum_partials_kernel" in emitted, sorted(emitted)   # the demangling worked
    unknown = sorted(set(BN_NOT_LAUNCHED) - emitted)
    assert not unknown, f"BN_NOT_LAUNCHED names kernels the library does not build: {unknown}"
    wanted = emitted - set(BN_NOT_LAUNCHED)
    covered = set().union(*(kv.expected_bn_kernels(**c) for c in kv.BN_CASES))
    missing = sorted(wanted - covered)
    assert not missing, f"fusion_bn kernels without a parity case in tests/kernel_variants.py BN_CASES: {missing}"
    stale = sorted(covered - wanted)
    assert not stale, f"cases name kernels the library does not build: {stale}"


# ---- the weight gradient of the per-point Linear: variants, staging forms, stage counts -----------------------------------------------
WGRAD_UNITS = ("linear_grad",)
WGRAD_NOT_LAUNCHED = {}   # every linear_wgrad_kernel instantiation is picked by some tile count; the reduce kernel runs in every call


def test_the_wgrad_mirror_follows_the_c_conditions():
    # supported(), linear_grad.hip:122-125; wgs_of :126-129; the dispatch :145-149, :162-166; the staging forms :45
    L, ok = kv.wgrad_launch, kv.wgrad_supported
    assert [L(4096, n, k)["variant"] for n, k in ((32, 32), (64, 64), (64, 65), (128, 64), (128, 65), (256, 128), (256, 129), (256, 256))] == [1, 1, 2, 2, 4, 8, 16, 16]
    assert L(1, 32, 32)["workgroups"] == 1 and L(8192, 32, 32)["workgroups"] == 256 and L(8193, 32, 32)["stages_per_wg"] == 2
    assert L(8193, 32, 32)["idle"] == 127 and L(16384, 32, 32)["idle"] == 0 and L(16385, 32, 32)["idle"] == 85     # 513 stages, 3 each: 171 busy
    assert L(196608, 64, 536)["stages_per_wg"] == 24 and L(196608, 64, 536)["tiles_per_wave"] == [9, 9, 8, 8]
    assert L(33, 32, 32)["tail_rows"] == 1 and L(64, 32, 32)["tail_rows"] == 32
    assert not ok(100, 257, 32) and ok(100, 256, 256) and not ok(100, 256, 257) and not ok(0, 32, 32)
    assert ok(100, 32, 1216) and not ok(100, 32, 1217) and kv.wgrad_max_k(32) == 1216     # the LDS limit: 32 (np + kp + 8) 4 <= 160 KB
    assert kv.wgrad_max_k(64) == 1024 and kv.wgrad_max_k(256) == 256            # the tile limit: 2 x 32 and 8 x 8 tiles on four waves of 16
    st = lambda **kw: (lambda r: (r["gz_vec"], r["gz_why"], r["x_vec"], r["x_why"]))(L(4096, 64, 64, **kw))
    assert st() == (True, (), True, ())
    assert st(gz_stride=68) == (True, (), True, ()) and st(gz_stride=66) == (False, ("stride",), True, ())
    assert st(x_offset_floats=4) == (True, (), True, ()) and st(x_stride=68, x_offset_floats=1) == (True, (), False, ("base",))
    assert L(4096, 3, 32)["gz_why"] == ("width", "stride") and L(4096, 3, 32, gz_stride=4)["gz_why"] == ("width",)
    for bad in ((100, 512, 32), (100, 32, 1248)):
        with pytest.raises(ValueError):
            L(*bad)
    with pytest.raises(ValueError):
        L(100, 64, 64, gz_stride=60)


WGRAD_EDGES = {
    **{f"tiles-per-wave variant {v}": (lambda v: lambda c, g: g["variant"] == v)(v) for v in (1, 2, 4, 8, 16)},
    **{f"{op} staged as float4": (lambda op: lambda c, g: g[f"{op}_vec"])(op) for op in ("gz", "x")},
    **{f"{op} staged element-wise because of its {why} alone": (lambda op, why: lambda c, g: g[f"{op}_why"] == (why,))(op, why)
       for op in ("gz", "x") for why in ("width", "stride", "base")},
    "a single row": lambda c, g: c["rows"] == 1,
    "a single-stage launch": lambda c, g: g["stages"] == 1,
    "two stages, the second with one live row": lambda c, g: g["stages"] == 2 and g["tail_rows"] == 1,
    "exactly 256 full stages": lambda c, g: g["stages"] == kv.WGRAD_MAX_WGS and g["tail_rows"] == kv.WGRAD_ROWS and g["stages_per_wg"] == 1,
    "two stages per workgroup with idle workgroups": lambda c, g: g["stages_per_wg"] == 2 and g["idle"] > 0,
    "n below one tile": lambda c, g: c["n"] < 32,
    "k below one tile": lambda c, g: c["k"] is not None and c["k"] < 32,
    "padded tiles on both axes": lambda c, g: c["n"] % 32 and c["k"] is not None and c["k"] % 32 and g["tiles"] > 1,
    "every thread owns a bias column": lambda c, g: c["n"] == 64 * kv.WGRAD_WAVES,
    "the 16-variant full (64 tiles)": lambda c, g: g["variant"] == 16 and g["tiles"] == 64 and g["tiles_per_wave"] == [16] * 4,
    "the 16-variant uneven (34 tiles: 9 / 9 / 8 / 8)": lambda c, g: g["variant"] == 16 and g["tiles_per_wave"] == [9, 9, 8, 8],
    "a column block of a wider gz written into a block of a larger dW / db": lambda c, g: c["block"] is not None and c["gz"] is not None and c["gz"][1] == c["block"][1] > 0,
    "LDS above the 64 KB default": lambda c, g: g["lds_bytes"] > kv.WGRAD_LDS_DEFAULT,
    "the largest k at its n: LDS just under the 160 KB opt-in": lambda c, g: c["k"] is None and g["lds_bytes"] + 32 * 32 * 4 > kv.WGRAD_LDS_BYTES >= g["lds_bytes"],
}


def wgrad_cases_reaching(edge):
    return [kv.wgrad_case_id(c) for c in kv.WGRAD_CASES if WGRAD_EDGES[edge](c, kv.wgrad_launch(*kv.wgrad_shape(c)))]


def test_the_wgrad_cases_reach_every_variant_staging_form_and_stage_count():
    missing = [edge for edge in WGRAD_EDGES if not wgrad_cases_reaching(edge)]
    assert not missing, missing
    ids = [kv.wgrad_case_id(c) for c in kv.WGRAD_CASES]
    assert len(set(ids)) == len(ids)
    assert all(c["rows"] * (c["n"] + (c["k"] or kv.wgrad_max_k(c["n"]))) <= 4 << 20 for c in kv.WGRAD_CASES)   # small: seconds on the device


def test_every_wgrad_kernel_instantiation_has_a_parity_case():
    emitted = emitted_kernels(WGRAD_UNITS)
    assert "linear_wgrad_reduce_kernel" in emitted and "linear_wgrad_kernel<16>" in emitted, sorted(emitted)   # the demangling worked
    wanted = emitted - set(WGRAD_NOT_LAUNCHED) - {"linear_wgrad_reduce_kernel"}
    covered = {kv.wgrad_launch(*kv.wgrad_shape(c))["kernel"] for c in kv.WGRAD_CASES}
    missing = sorted(wanted - covered)
    assert not missing, f"linear_wgrad_kernel instantiations without a case in tests/kernel_variants.py WGRAD_CASES: {missing}"
    stale = sorted(covered - wanted)
    assert not stale, f"cases name kernels the library does not build: {stale}"


# ---- the narrow-head attention backward: the counts that sit on the kernels' own boundaries ------------------------------------------
def _attn_edges(role, side):
    """Edges of one kernel: its stationary side in wave tiles of 32 and workgroup blocks of 128, its streamed side in stages of 64."""
    T, B = kv.ATTN_GRAD_TILE, kv.ATTN_GRAD_BLOCK
    R = lambda g: g[role]
    return {
        f"{role}: one {side} row": lambda nq, nk, g: R(g)["workgroups"] == 1 and R(g)["last_tile"] == 1 and (nq if side == "query" else nk) == 1,
        f"{role}: a last wave tile with {T - 1} live rows": lambda nq, nk, g: R(g)["last_tile"] == T - 1,
        f"{role}: a full single tile": lambda nq, nk, g: R(g)["workgroups"] == 1 and R(g)["last_tile"] == T and (nq if side == "query" else nk) == T,
        f"{role}: a second wave with one live row": lambda nq, nk, g: (nq if side == "query" else nk) == T + 1,
        f"{role}: a last workgroup block one row short": lambda nq, nk, g: (nq if side == "query" else nk) == B - 1,
        f"{role}: one full workgroup block": lambda nq, nk, g: (nq if side == "query" else nk) == B,
        f"{role}: a second workgroup that holds one row": lambda nq, nk, g: R(g)["workgroups"] == 2 and (nq if side == "query" else nk) == B + 1,
        f"{role}: one streamed row": lambda nq, nk, g: R(g)["stages"] == 1 and R(g)["last_stage"] == 1,
        **{f"{role}: one stage with {n} rows": (lambda n: lambda nq, nk, g: R(g)["stages"] == 1 and R(g)["last_stage"] == n)(n) for n in (T - 1, T, T + 1, 2 * T - 1)},
        **{f"{role}: {s} stages, the last with {n} rows": (lambda s, n: lambda nq, nk, g: R(g)["stages"] == s and R(g)["last_stage"] == n)(s, n)
           for s, n in ((1, 64), (2, 1), (2, 63), (2, 64), (3, 1), (4, 1))},     # 3 stages: buffer 0 a second time; 4: buffer 1 a second time
    }


ATTN_GRAD_EDGES = {**_attn_edges("attention_stats_kernel", "query"), **_attn_edges("attention_dq_kernel", "query"), **_attn_edges("attention_dkv_kernel", "key")}


def test_the_attention_backward_grid_holds_every_boundary_class():
    """ATTN_GRAD_COUNTS, crossed with itself, puts a count on and on both sides of every boundary of the three kernels."""
    assert kv.attention_small_grad_launch(129, 193) == {
        "attention_stats_kernel": dict(workgroups=2, last_tile=1, stages=4, last_stage=1), "attention_dq_kernel": dict(workgroups=2, last_tile=1, stages=4, last_stage=1),
        "attention_dkv_kernel": dict(workgroups=2, last_tile=1, stages=3, last_stage=1)}
    assert kv.attention_small_grad_launch(128, 64)["attention_dkv_kernel"] == dict(workgroups=1, last_tile=32, stages=2, last_stage=64)
    grid = [(nq, nk, kv.attention_small_grad_launch(nq, nk)) for nq in kv.ATTN_GRAD_COUNTS for nk in kv.ATTN_GRAD_COUNTS]
    missing = [edge for edge, pred in ATTN_GRAD_EDGES.items() if not any(pred(*p) for p in grid)]
    assert not missing, missing
    # the counts the issue behind these tests lists, on both sides (the key-stationary kernel streams the queries)
    assert set(kv.ATTN_GRAD_COUNTS) >= {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193}


# ---- the wide-head attention in a training graph: 43 instantiations, tiles of 32 rows, blocks of 128 or 32, stages of 32 ----------------
WIDE_TRAIN_UNITS = ("attention_wide_grad",)
WIDE_TRAIN_NOT_LAUNCHED = {}   # every instantiation is picked by some (head width, drop_p > 0, lengths given, key split) of the two entry pairs
WIDE_BF, WIDE_HEADS = 2, 2     # BF, HEADS of test_attention_wide_grad_edges_gpu.py's grid


def test_the_wide_attention_mirror_follows_the_c_conditions():
    # wide_keys_split, attention_wide_fwd.h:393-395; launch_forward, attention_wide_grad.hip:55-72; GradCfg :77-90 (SPLIT :79, RPW :86);
    # the backward's grids :404-407; the stage counts :215, :333, attention_wide_fwd.h:122, :294-296
    split, names, L = kv.wide_keys_split, kv.attention_wide_train_kernels, kv.attention_wide_grad_launch
    assert split(2, 37, 128, 1) and not split(2, 37, 127, 1) and split(16, 256, 256, 3) and not split(16, 512, 256, 4)
    assert split(63, 128, 128, 4) and not split(64, 128, 128, 4) and split(64, 128, 128, 3)      # 63 * 4 * 4 = 1008 < 1024 <= 64 * 4 * 4
    assert names(2, 2, 256, 33, 128) == {"attention_wide_ksplit_lse_kernel<256, false>", "attention_wide_dsum_kernel<256>",
                                          "attention_wide_dq_kernel<256, false>", "attention_wide_dkv_kernel<256, false>"}
    assert "attention_wide_lse_kernel<256, true, AttnLengths>" in names(2, 2, 256, 33, 127, drop=True, lengths=True)
    assert "attention_wide_ksplit_lse_kernel<256, true, AttnLengths>" in names(2, 1, 256, 37, 130, drop=True, lengths=True)
    assert "attention_wide_lse_kernel<64, true>" in names(2, 2, 64, 33, 200, drop=True)           # widths 32 / 64 never split the keys
    assert "attention_wide_lse_kernel<256, false, AttnLengths>" in names(64, 4, 256, 128, 128, lengths=True)
    with pytest.raises(ValueError):
        names(2, 2, 128, 33, 65)
    g = L(64, 129, 97)
    assert g["attention_wide_dq_kernel"] == dict(block=128, workgroups=2, last_tile=1, stages=4, last_stage=1)
    assert g["attention_wide_dkv_kernel"] == dict(block=128, workgroups=1, last_tile=1, stages=5, last_stage=1)
    assert g["attention_wide_lse_kernel"] == dict(block=128, workgroups=2, last_tile=1, stages=4, last_stage=1)
    assert g["attention_wide_dsum_kernel"] == dict(workgroups=33, last_block_lanes=64)             # 2 * 129 * 2 rows of 16 lanes = 8256 = 32 * 256 + 64
    g = L(256, 33, 161)
    assert g["attention_wide_dq_kernel"] == dict(block=32, workgroups=2, last_tile=1, stages=6, last_stage=1)
    assert g["attention_wide_dkv_kernel"] == dict(block=32, workgroups=6, last_tile=1, stages=2, last_stage=1)
    assert g["attention_wide_ksplit_lse_kernel"] == dict(block=32, workgroups=2, last_tile=1, stages=6, last_stage=1, stages_per_wave=[2, 2, 1, 1], idle_waves=0)
    assert "attention_wide_lse_kernel" in L(256, 33, 127) and L(256, 33, 127)["attention_wide_lse_kernel"]["block"] == 128
    assert L(256, 1, 1)["attention_wide_dsum_kernel"] == dict(workgroups=1, last_block_lanes=256)   # 4 rows of 64 lanes
    assert L(32, 1, 1)["attention_wide_dsum_kernel"] == dict(workgroups=1, last_block_lanes=32)
    assert kv.wide_ksplit_waves(31) == dict(stages_per_wave=[1, 0, 0, 0], idle_waves=3) and kv.wide_ksplit_waves(0)["idle_waves"] == 4
    assert kv.wide_ksplit_waves(33)["stages_per_wave"] == [1, 1, 0, 0] and kv.wide_ksplit_waves(130)["stages_per_wave"] == [2, 1, 1, 1]


def _wide_edges(role, side, block):
    """Edges of one backward kernel: its stationary side in tiles of 32 and workgroup blocks of `block` rows, its streamed side in stages of 32."""
    T = kv.WIDE_TILE
    n = (lambda nq, nk: nq) if side == "query" else (lambda nq, nk: nk)
    R = lambda g: g[role]
    on = lambda g: R(g)["block"] == block
    tag = f"{role}, block {block}"
    return {
        f"{tag}: one {side} row": lambda nq, nk, g: on(g) and n(nq, nk) == 1 and R(g)["workgroups"] == 1 and R(g)["last_tile"] == 1,
        f"{tag}: a last wave tile with {T - 1} live rows": lambda nq, nk, g: on(g) and R(g)["last_tile"] == T - 1,
        f"{tag}: a last wave tile with one live row behind full ones": lambda nq, nk, g: on(g) and R(g)["last_tile"] == 1 and n(nq, nk) > 1,
        f"{tag}: one full tile": lambda nq, nk, g: on(g) and n(nq, nk) == T,
        f"{tag}: a block one row short": lambda nq, nk, g: on(g) and n(nq, nk) == block - 1,
        f"{tag}: one full block": lambda nq, nk, g: on(g) and n(nq, nk) == block and R(g)["workgroups"] == 1,
        f"{tag}: a second workgroup that holds one row": lambda nq, nk, g: on(g) and n(nq, nk) == block + 1 and R(g)["workgroups"] == 2 and R(g)["last_tile"] == 1,
        f"{tag}: one streamed row (no prefetch)": lambda nq, nk, g: on(g) and R(g)["stages"] == 1 and R(g)["last_stage"] == 1,
        **{f"{tag}: one stage of {r} rows": (lambda r: lambda nq, nk, g: on(g) and R(g)["stages"] == 1 and R(g)["last_stage"] == r)(r) for r in (T - 1, T)},
        **{f"{tag}: {s} stages, the last with one row": (lambda s: lambda nq, nk, g: on(g) and R(g)["stages"] == s and R(g)["last_stage"] == 1)(s) for s in (2, 3, 4)},
    }


def _ksplit(g):
    return g.get("attention_wide_ksplit_lse_kernel", {}).get("stages_per_wave")


WIDE_GRAD_EDGES = {
    **{k: v for block in (128, 32) for role, side in (("attention_wide_dq_kernel", "query"), ("attention_wide_dkv_kernel", "key"))
       for k, v in _wide_edges(role, side, block).items()},
    "key-split forward: all four waves with one stage": lambda nq, nk, g: _ksplit(g) == [1, 1, 1, 1],
    "key-split forward: wave 0 with a second stage": lambda nq, nk, g: _ksplit(g) == [2, 1, 1, 1],
    "key-split forward: waves 0 and 1 with a second stage": lambda nq, nk, g: _ksplit(g) == [2, 2, 1, 1],
    "width 256, query-stationary forward with three stages": lambda nq, nk, g: g["attention_wide_dq_kernel"]["block"] == 32 and g.get("attention_wide_lse_kernel", {}).get("stages") == 3,
    "dsum: a last block of fewer than 256 lanes": lambda nq, nk, g: g["attention_wide_dsum_kernel"]["last_block_lanes"] < 256,
    "dsum: more than one block, the last one full": lambda nq, nk, g: g["attention_wide_dsum_kernel"] == dict(workgroups=g["attention_wide_dsum_kernel"]["workgroups"], last_block_lanes=256)
        and g["attention_wide_dsum_kernel"]["workgroups"] > 1,
}


def test_the_wide_attention_grid_holds_every_boundary_class():
    """WIDE_GRAD_COUNTS, crossed with itself at the three head widths, puts a count on and on both sides of every boundary."""
    grid = [(nq, nk, kv.attention_wide_grad_launch(hd, nq, nk, WIDE_BF, WIDE_HEADS)) for hd in kv.WIDE_HEAD_WIDTHS for nq in kv.WIDE_GRAD_COUNTS
            for nk in kv.WIDE_GRAD_COUNTS]
    missing = [edge for edge, pred in WIDE_GRAD_EDGES.items() if not any(pred(*p) for p in grid)]
    assert not missing, missing
    assert len(WIDE_GRAD_EDGES) == 4 * 13 + 6
    assert set(kv.WIDE_GRAD_COUNTS) >= {1, 31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 161}


def _lens(c, side):
    """The lengths of one side of a case with `full` for the padded count."""
    return {"full" if v == c["nq" if side == "qlen" else "nk"] else v for v in (c[side] or ())}


def _is(kind, hd=None, form=None, **shape):
    def pred(c):
        names = kv.wide_case_kernels(c)
        return (c["kind"] == kind and (hd is None or c["hd"] == hd) and all(c[k] == v for k, v in shape.items())
                and (form is None or any("ksplit" in n for n in names) == (form == "ksplit")))
    return pred


# what the explicit cases must hold, one entry per case the sections (b) to (f) of the issue behind them ask for: each is met by
# exactly one case, so taking any case away fails here
WIDE_TRAIN_REQUIRED = {
    **{f"dropout at width {hd}, {nq} x {nk}": _is("dropout", hd, nq=nq, nk=nk, bf=2, heads=2, drop=True) for hd in kv.WIDE_HEAD_WIDTHS for nq, nk in ((33, 65), (129, 63), (1, 129), (128, 64))},
    **{f"dropout, key-split forward (one head, 37 queries) with stages {per} and a partial last stage":
       (lambda per: lambda c: _is("dropout", 256, "ksplit", drop=True, heads=1, nq=37)(c) and c["nk"] % 32 and kv.wide_ksplit_waves(c["nk"])["stages_per_wave"] == per)(per)
       for per in ([2, 1, 1, 1], [2, 2, 1, 1])},
    **{f"dropout with lengths at width {hd}, {form}, a length of {v} on the {side[0]} side":
       (lambda hd, form, side, v: lambda c: _is("dropout-lengths", hd, form, drop=True)(c) and v in _lens(c, side))(hd, form, side, v)
       for hd, form in ((32, "qs"), (64, "qs"), (256, "qs"), (256, "ksplit")) for side in ("qlen", "klen") for v in (0, 1, 31, 33, "full")},
    "dropout with lengths, key-split forward: a key length that leaves three waves without a stage":
        lambda c: _is("dropout-lengths", 256, "ksplit")(c) and any(kv.wide_ksplit_waves(v)["idle_waves"] == 3 for v in c["klen"]),
    **{f"strides at width {hd}": _is("strides", hd, drop=False, qlen=None) for hd in kv.WIDE_HEAD_WIDTHS},
    "strides with dropout and lengths": lambda c: c["kind"] == "strides" and c["drop"] and c["qlen"] is not None and c["klen"] is not None,
    "large logits at width 256 on partial tiles": lambda c: _is("logits", 256, nq=33, nk=65)(c) and c["factor"] == 6.0,
}
WIDE_GUARD_REQUIRED = {
    **{f"guard rows at width {hd}, {form}, {'lengths' if lengths else 'plain'}":
       (lambda hd, form, lengths: lambda c: _is("guard", hd, form, drop=False)(c) and c["nq"] % 32 and c["nk"] % 32 and (c["qlen"] is not None) == lengths
        and (not lengths or all(0 < a < c["nq"] for a in c["qlen"]) and all(0 < k < c["nk"] for k in c["klen"])))(hd, form, lengths)
       for hd, form in ((32, "qs"), (64, "qs"), (256, "qs"), (256, "ksplit")) for lengths in (False, True)},
}


def test_the_wide_attention_cases_are_the_ones_the_sections_ask_for():
    for required, cases in ((WIDE_TRAIN_REQUIRED, kv.WIDE_TRAIN_CASES), (WIDE_GUARD_REQUIRED, kv.WIDE_GUARD_CASES)):
        missing = [what for what, pred in required.items() if not any(pred(c) for c in cases)]
        assert not missing, missing
        needed = [kv.wide_case_id(c) for c in cases if not any(pred(c) and sum(1 for o in cases if pred(o)) == 1 for pred in required.values())]
        assert not needed, f"cases no requirement depends on alone: {needed}"
    ids = [kv.wide_case_id(c) for c in kv.WIDE_GUARD_CASES + kv.WIDE_TRAIN_CASES]
    assert len(set(ids)) == len(ids)
    assert all(c["bf"] * c["nq"] * c["nk"] * c["heads"] <= 1 << 17 for c in kv.WIDE_GUARD_CASES + kv.WIDE_TRAIN_CASES)   # small: milliseconds on the device


def test_every_wide_attention_training_kernel_has_a_case():
    emitted = emitted_kernels(WIDE_TRAIN_UNITS)
    assert len(emitted) == 43 and "attention_wide_dsum_kernel<256>" in emitted, sorted(emitted)   # the demangling worked
    wanted = emitted - set(WIDE_TRAIN_NOT_LAUNCHED)
    grid = set().union(*(kv.attention_wide_train_kernels(WIDE_BF, WIDE_HEADS, hd, nq, nk) for hd in kv.WIDE_HEAD_WIDTHS for nq in kv.WIDE_GRAD_COUNTS
                         for nk in kv.WIDE_GRAD_COUNTS))
    covered = grid.union(*(kv.wide_case_kernels(c) for c in kv.WIDE_GUARD_CASES + kv.WIDE_TRAIN_CASES))
    missing = sorted(wanted - covered)
    assert not missing, f"wide attention kernels without a case in tests/kernel_variants.py (grid, WIDE_GUARD_CASES, WIDE_TRAIN_CASES): {missing}"
    stale = sorted(covered - wanted)
    assert not stale, f"cases name kernels the library does not build: {stale}"
    # dropout with lengths is reached by the dropout-lengths cases alone: 3 forward + 3 dq + 3 dkv + the key-split forward
    both = {n for n in wanted if "true, AttnLengths" in n}
    assert len(both) == 10 and both <= set().union(*(kv.wide_case_kernels(c) for c in kv.wide_cases("dropout-lengths")))


# ---- the EMD backward and the interpolation weights' backward ----------------------------------------------------------------------------
EMD_GRAD_UNITS, INTERP3_GRAD_UNITS = ("emd_grad",), ("interp3_grad",)


def test_every_emd_and_interp3_backward_kernel_has_a_case():
    for units, cases, count, probe in ((EMD_GRAD_UNITS, kv.EMD_GRAD_CASES, 7, "emd_grad_kernel<2, true>"),
                                       (INTERP3_GRAD_UNITS, kv.INTERP3_GRAD_CASES, 1, "interp3_weights_grad_kernel")):
        emitted = emitted_kernels(units)
        assert len(emitted) == count and probe in emitted, sorted(emitted)   # the demangling worked
        covered = {n for c in cases for n in c["kernels"]}
        missing = sorted(emitted - covered)
        assert not missing, f"{units[0]} kernels without a case in tests/kernel_variants.py: {missing}"
        stale = sorted(covered - emitted)
        assert not stale, f"cases name kernels the library does not build: {stale}"


def test_the_emd_and_interp3_cases_sit_on_the_kernels_boundaries():
    # emd_grad.hip:24 (64 lane points, tiles of 512 in wave slices of 64), :175 (eighths of m), :199 (8 rows, 256 lanes), :138 (1024 lanes);
    # interp3_grad.hip:13 (256 points per workgroup)
    lean = {(c["n"], c["m"]) for c in kv.emd_cases("lean")}
    assert lean == {(1, 1), (1, 513), (513, 1), (63, 65), (64, 64), (65, 63), (64, 512), (511, 64), (512, 513), (577, 129)}
    for lanes, streamed in (({n for n, _ in lean}, {m for _, m in lean}), ({m for _, m in lean}, {n for n, _ in lean})):   # grad1, grad2
        assert lanes >= {1, 63, 64, 65} and streamed >= {1, 63, 64, 65, 512, 513}, (lanes, streamed)
    lens = [(c["n"], c["m"], c["len1"], c["len2"]) for c in kv.emd_cases("lean-lengths")]
    assert lens == [(63, 65, (63, 63), (65, 65)), (512, 513, (512, 512), (513, 513)), (64, 65, (31, 64), (65, 1))]
    match = {(c["n"], c["m"]) for c in kv.emd_cases("match")}
    assert match == {(1, 1), (3, 5), (64, 7), (65, 8), (255, 9), (256, 16), (257, 17), (1023, 1), (1024, 3), (1025, 15)}
    assert {m for _, m in match} >= {1, 7, 8, 9} and {n for n, _ in match} >= {1, 255, 256, 257, 1023, 1024, 1025}
    plain = {(c["n"], c["s"]) for c in kv.INTERP3_GRAD_CASES if not c["coincident"]}
    assert plain == {(n, s) for n in (1, 255, 256, 257, 513) for s in (3, 40)}
    assert [(c["n"], c["s"], c["coincident"]) for c in kv.INTERP3_GRAD_CASES if c["coincident"]] == [(257, 40, 5)]
