#!/usr/bin/env python3
"""Are the kernels two builds have in common the same machine code?

    python tools/isa_same_kernels.py PARENT/isa/attention.s mocopci_amd/csrc/isa/attention.s [more pairs ...]

For every kernel (a symbol with an .amdhsa_kernel descriptor) of the first file of a pair, the function body and the descriptor are
compared with the second file's kernel of the same name.  Two things may differ and are normalised away: the symbol's own mangled
name (a template that gained an empty trailing parameter pack mangles with J E among its template arguments and DpT<n>_ behind its
parameter types) and the numbers of local labels
(.LBB<n>_<m>, .Lfunc_end<n>), which count functions of the unit.  Kernels only the second file has (the length forms) are listed,
not compared.  Exit status 1 if a common kernel differs or one is missing."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        name, desc = m.group(1), m.group(2)
        b = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M)
        body = b.group(0) if b else ""
        key = re.sub(r"DpT\d*_$", "", re.sub(r"JE(?=EE)", "", name))   # an empty trailing pack
        norm = (body + "\n" + desc).replace(name, "SYM")
        norm = re.sub(r"\.LBB\d+_", ".LBB_", norm)
        norm = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", norm)
        norm = "\n".join(l.split(";")[0].rstrip() for l in norm.splitlines())   # comments name source lines and block numbers
        out[key] = norm
    return out


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        print(__doc__)
        return 2
    bad = 0
    for a, b in zip(argv[0::2], argv[1::2]):
        ka, kb = kernels(a), kernels(b)
        for name in sorted(ka):
            if name not in kb:
                print(f"MISSING  {b}: {name}")
                bad += 1
            elif ka[name] != kb[name]:
                print(f"DIFFERS  {b}: {name}")
                bad += 1
            else:
                print(f"same     {b}: {name} ({ka[name].count(chr(10))} lines)")
        for name in sorted(set(kb) - set(ka)):
            print(f"new      {b}: {name}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
