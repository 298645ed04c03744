"""Static resources of every kernel of one unit, from two device-assembly files of it (make -C mocopci_amd/csrc isa/UNIT.s at two
commits): the compiler's own figures per kernel -- vector, accumulator and scalar registers, static LDS, scratch bytes per lane,
spilled scalar / vector registers, waves per SIMD the registers allow.  A kernel of the second file whose last template argument is
`false` is compared with the kernel of the first file that lacks that argument (a compile-time flag added since); kernels that end
in `true`, and kernels the first file does not have at all (a new unit: pass an empty file), are listed on their own.

    python tools/isa_resources.py PARENT.s NOW.s > profiles/NAME_resources.txt"""
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


def main():
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
