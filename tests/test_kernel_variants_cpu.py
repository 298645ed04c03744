"""-m "not gpu": every kernel instantiation of the dense-layer units (linear, mlp, attention) has a parity case.  The device assembly
lists the instantiations the compiler actually emitted; each one except the weight-packing kernels must be what
kernel_variants.expected_kernel names for at least one entry of kernel_variants.CASES (the cases of test_kernel_variants_gpu.py).
A template instantiation added later without a case fails here, on a machine without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from tests import kernel_variants as kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mocopci_amd", "csrc")
UNITS = ("linear", "mlp", "attention")


def emitted_kernels():
    """Demangled kernel names of the three units' device assembly, without namespace, return type and arguments."""
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


def test_every_case_names_a_kernel_and_ids_are_unique():
    ids = [kv.case_id(c) for c in kv.CASES]
    assert len(set(ids)) == len(ids)


def test_every_dense_kernel_instantiation_has_a_parity_case():
    emitted = emitted_kernels()
    assert any(n.startswith("linear_kernel<") for n in emitted), sorted(emitted)   # the demangling worked
    wanted = {n for n in emitted if not n.endswith("_pack_kernel")}
    covered = {kv.expected_kernel(**c) for c in kv.CASES}
    missing = sorted(wanted - covered)
    assert not missing, f"kernel instantiations without a parity case in tests/kernel_variants.py CASES: {missing}"
    stale = sorted(covered - wanted)
    assert not stale, f"cases name kernels the library does not build: {stale}"
