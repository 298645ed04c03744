#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc --cuda-device-only -S) kernel by kernel: the instruction stream of every kernel with
local labels renumbered in order of appearance, and the resource figures of its .amdhsa_kernel block.

    tools/isa_kernel_diff.py BEFORE.s AFTER.s     # prints one line per kernel: same / differs (+ resources), exit 1 on a difference
    tools/isa_kernel_diff.py FILE.s               # prints the resource table of one file
"""
import re
import subprocess
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = []
    for line in out[:len(names)]:
        line = re.sub(r"^void\s+", "", line.strip()).replace("(anonymous namespace)::", "")
        depth, end = 0, len(line)
        for i, ch in enumerate(line):
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                end = i
                break
        short.append(line[:end])
    return short


def kernels(path):
    """{short name: (instruction lines, {figure: value})}"""
    text = open(path).read()
    mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    res = {}
    for m, name in zip(mangled, demangle(mangled)):
        body = text[text.index(f"\n{m}:") + 1:]
        body = body[:body.index(".Lfunc_end")]
        labels, lines = {}, []
        for raw in body.split("\n")[1:]:
            line = raw.split(";")[0].strip()
            if not line or line.startswith("."):
                lab = re.match(r"^(\.LBB\w+):", line)
                if lab:
                    labels.setdefault(lab.group(1), f"L{len(labels)}")
                    lines.append(labels[lab.group(1)] + ":")
                continue
            lines.append(line)
        lines = [re.sub(r"\.LBB\w+", lambda mo: labels.setdefault(mo.group(0), f"L{len(labels)}"), l) for l in lines]
        block = text[text.index(f".amdhsa_kernel {m}"):]
        block = block[:block.index(".end_amdhsa_kernel")]
        figs = {f: int(v) for f in FIGURES for v in re.findall(rf"\.amdhsa_{f}\s+(\d+)", block)}
        res[name] = (lines, figs)
    return res


def table(ks):
    for name in sorted(ks):
        lines, f = ks[name]
        print(f"  {name}: instructions {sum(1 for l in lines if not l.endswith(':'))}  vgpr {f.get('next_free_vgpr')} (accum_offset {f.get('accum_offset')})  "
              f"sgpr {f.get('next_free_sgpr')}  scratch {f.get('private_segment_fixed_size')} B  static LDS {f.get('group_segment_fixed_size')} B")


def main(argv):
    if len(argv) == 2:
        table(kernels(argv[1]))
        return 0
    before, after = kernels(argv[1]), kernels(argv[2])
    bad = 0
    for name in sorted(set(before) | set(after)):
        if name not in before or name not in after:
            print(f"{name}: only in {'AFTER' if name in after else 'BEFORE'}")
            bad += 1
            continue
        same = before[name][0] == after[name][0]
        print(f"{name}: {'same instruction stream' if same else 'DIFFERS'}; resources {'same' if before[name][1] == after[name][1] else 'DIFFER'} {after[name][1]}")
        if not same or before[name][1] != after[name][1]:
            print(f"    before: {len(before[name][0])} lines {before[name][1]}")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
