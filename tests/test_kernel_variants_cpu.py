"""-m "not gpu": every kernel instantiation of the dense-layer units (linear, mlp, attention) and of the fused point-layer units
(fusion, cross, pointconv, ptblock) has a parity case.  The device assembly lists the instantiations the compiler actually emitted;
each one except the weight-packing kernels and the entries of NOT_LAUNCHED must be what kernel_variants.expected_kernel names for at
least one entry of kernel_variants.CASES (the cases of test_kernel_variants_gpu.py and test_fused_variants_gpu.py).  A template
instantiation added later without a case fails here, on a machine without a GPU.

fusion_bn.hip is not among the units: its 13 kernels are mostly backward passes, which have no parity cases of this form; its
forward is compared with float64 by tests/test_grad_gpu.py."""
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


def emitted_kernels():
    """Demangled kernel names of the units' device assembly, without namespace, return type and arguments."""
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("no hipcc: the device assembly cannot be generated on this machine")
    if not shutil.which("c++filt"):
        pytest.skip("no c++filt to demangle the kernel names")
    subprocess.check_call(["make", "-C", CSRC, "-j3", "-s"] + [f"isa/{u}.s" for u in UNITS])
    mangled = []
    for u in UNITS:
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
    # pointconv.hip:466-482, :495-520; cross.hip:489-497; fusion.hip:291, :318; ptblock.hip:188, :197
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
    # the grids beside the dispatch: fusion.hip:304, cross.hip:439, :459-462, pointconv.hip:471, :475, :499, ptblock.hip:193-194
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
    """(dealt by XCD, units per eighth, units per workgroup step) of a case's launch: common.h:101-111, cross.hip:197-204."""
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
