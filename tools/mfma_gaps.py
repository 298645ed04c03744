#!/usr/bin/env python3
"""Static census of the gaps between consecutive MFMAs of one kernel in a device-assembly file.

    python tools/mfma_gaps.py mocopci_amd/csrc/isa/fusion.s fusion_split_kernel

Prints the number of MFMAs, the number of MFMA -> MFMA transitions with no vector instruction between them, the histogram of vector
instructions per gap (a gap ends at the next MFMA; a label or branch in between is reported, not hidden), the largest gap, and the vector
and LDS instructions of the kernel in total.  "Vector instruction" is every v_* that is not an MFMA; s_nop / s_waitcnt are listed apart."""
import collections
import re
import sys


def body(path, kernel):
    lines, out, on = open(path).read().splitlines(), [], False
    for ln in lines:
        if not on:
            on = bool(re.match(r"^\S*%s\S*:" % re.escape(kernel), ln))
            continue
        if ln.startswith(".Lfunc_end"):
            break
        out.append(ln)
    return out


def main():
    path, kernel = sys.argv[1], sys.argv[2]
    gaps, cur, seen, valu, lds, nops, broken = [], None, 0, 0, 0, 0, 0
    crossed = False
    for ln in body(path, kernel):
        t = ln.strip()
        if not t or t.startswith((";", ".")) and not re.match(r"^\.L\w+:", t):
            continue
        if re.match(r"^\.?\w+:", t):
            crossed = True
            continue
        op = t.split()[0]
        if op.startswith("v_mfma"):
            seen += 1
            if cur is not None:
                gaps.append((cur, crossed))
            cur, crossed = 0, False
            continue
        if op.startswith(("s_branch", "s_cbranch")):
            crossed = True
        if op.startswith("v_"):
            valu += 1
            if cur is not None:
                cur += 1
        elif op.startswith("ds_"):
            lds += 1
        elif op == "s_nop":
            nops += 1
    straight = [g for g, c in gaps if not c]
    broken = [g for g, c in gaps if c]
    hist = collections.Counter(straight)
    print(f"{kernel} in {path}")
    print(f"MFMAs {seen}, MFMA->MFMA transitions {len(gaps)} ({len(broken)} of them across a label or branch: {sorted(broken)})")
    print(f"transitions with zero vector instructions: {hist.get(0, 0)} of {len(straight)} straight-line ones")
    print("vector instructions per straight-line gap: " + ", ".join(f"{k}: {hist[k]}" for k in sorted(hist)))
    print(f"largest straight-line gap: {max(straight) if straight else 0}")
    print(f"vector instructions in the kernel {valu}, LDS instructions {lds}, s_nop {nops}")


if __name__ == "__main__":
    main()
