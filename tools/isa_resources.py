"""Static resources of every kernel of one unit, from two device-assembly files of it (make -C mocopci_amd/csrc isa/UNIT.s at two
commits): the compiler's own figures per kernel -- vector, accumulator and scalar registers, static LDS, scratch bytes per lane,
spilled scalar / vector registers, waves per SIMD the registers allow.  A kernel of the second file whose last template argument is
`false` is compared with the kernel of the first file that lacks that argument (a compile-time flag added since); kernels that end
in `true`, and kernels the first file does not have at all (a new unit: pass an empty file), are listed on their own.

    python tools/isa_resources.py PARENT.s NOW.s > profiles/NAME_resources.txt

`--same-names PARENT.s NOW.s`: both files hold the same kernels (a refactor).  Every kernel is compared name to name, with its static
instruction count (the lines of its body that are neither labels, directives nor comments) and that count's movement."""
import re
import subprocess
import sys

FIELDS = ("vgpr", "agpr", "sgpr", "lds", "scratch", "sspill", "vspill", "occ")


def parse(path):
    txt, out = open(path).read(), {}
    for m in re.finditer(r"\.set (\S+)\.has_indirect_call, \d+\n\t\.section\t\.AMDGPU\.csdata.*?\n; Kernel info:\n(.*?); WaveLimiterHint", txt, re.S):
        g = lambda k: re.search(r"; " + k + r":\s*(\S+)", m.group(2)).group(1)
        out[m.group(1)] = dict(vgpr=g("NumVgprs"), agpr=g("NumAgprs"), sgpr=g("TotalNumSgprs"), lds=g("LDSByteSize"), scratch=g("ScratchSize"),
                               occ=g("Occupancy"))
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", txt, re.S):
        if m.group(1) in out:
            out[m.group(1)]["sspill"] = re.search(r"\.sgpr_spill_count:\s*(\d+)", m.group(2)).group(1)
            out[m.group(1)]["vspill"] = re.search(r"\.vgpr_spill_count:\s*(\d+)", m.group(2)).group(1)
    names = list(out)
    if not names:   # an empty file: c++filt without arguments would wait for its standard input
        return {}
    plain =subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    short = [re.sub(r"\(.*", "", x.replace("void ", "").replace("(anonymous namespace)::", "")) for x in plain]
    return dict(zip(short, (out[n] for n in names)))


def with_instruction_counts(path):
    """parse(path) with an `insns` figure per kernel"""
    res, txt = parse(path), open(path).read()
    for name, v in res.items():
        v["insns"] = None
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)}
    plain = subprocess.run(["c++filt"] + list(bodies), capture_output=True, text=True, check=True).stdout.split("\n")
    for mangled, full in zip(bodies, plain):
        short = re.sub(r"\(.*", "", full.replace("void ", "").replace("(anonymous namespace)::", ""))
        lines = (x.strip() for x in bodies[mangled].split("\n"))
        if short in res:
            res[short]["insns"] = sum(1 for x in lines if x and not x.startswith((";", ".")) and not x.endswith(":"))
    return res


def same_names(parent_path, now_path):
    parent, now = with_instruction_counts(parent_path), with_instruction_counts(now_path)
    assert set(parent) == set(now), sorted(set(parent) ^ set(now))
    fields = FIELDS + ("insns",)
    row = lambda v: "".join(f"{v[k]:>9}" for k in fields)
    print(f"{'kernel':<44}{'':8}" + "".join(f"{k:>9}" for k in fields))
    moved = 0
    for n in sorted(now):
        same = all(parent[n][k] == now[n][k] for k in FIELDS)
        moved += not same
        d = 100.0 * (now[n]["insns"] - parent[n]["insns"]) / parent[n]["insns"]
        print(f"{n:<44}{'parent':<8}{row(parent[n])}\n{'':<44}{'now':<8}{row(now[n])}   {'unchanged' if same else 'MOVED'}, instructions {d:+.2f} %")
    print(f"\n{len(now)} kernels, {moved} with a resource figure that moved")


def main():
    if sys.argv[1] == "--same-names":
        return same_names(sys.argv[2], sys.argv[3])
    parent, now = parse(sys.argv[1]), parse(sys.argv[2])
    stripped = lambda n: re.sub(r"<false>$", "", re.sub(r", false>$", ">", n))
    base = lambda n: n if n in parent else stripped(n)   # a kernel that had the argument already keeps its name
    row = lambda v: "".join(f"{v[k]:>9}" for k in FIELDS)
    head = f"{'kernel':<44}{'':8}" + "".join(f"{k:>9}" for k in FIELDS)
    moved, flagged = 0, 0
    # `true` kernels the parent has too are compared; a kernel the parent lacks under either name (a new unit) is listed on its own
    new = [n for n in sorted(now) if n not in parent and (n.endswith("true>") or base(n) not in parent)]
    print("FLAG = false: parent against now\n" + head)
    for n in sorted(now):
        if n in new:
            continue
        same = all(parent[base(n)][k] == now[n][k] for k in FIELDS)
        moved += not same
        print(f"{base(n):<44}{'parent':<8}{row(parent[base(n)])}\n{'':<44}{'now':<8}{row(now[n])}   {'unchanged' if same else 'MOVED'}")
    print(f"\n{len(now) - len(new)} kernels, {moved} moved\n\nFLAG = true: new kernels\n" + head)
    for n in new:
        bad = any(now[n][k] != "0" for k in ("scratch", "sspill", "vspill"))
        flagged += bad
        print(f"{n:<44}{'':<8}{row(now[n])}{'   SPILLS' if bad else ''}")
    print(f"\n{len(new)} kernels, {flagged} with scratch or spilled registers")


if __name__ == "__main__":
    main()
