#!/bin/bash
# tools/build_variant.sh <name> [extra hipcc flags...] -- a second build of the library (A/B or diagnostic defines) as
# tools/ab/lib<name>.so, objects under build/<name>/; the product library (mocopci_amd/libmocopci_hip.so) is not touched.
# Select it at run time with MCP_HIP_LIB=tools/ab/lib<name>.so (mocopci_amd/_lib.py).
# The Makefile builds it: every unit gets the product's own per-file flags, the extra flags behind them.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$root/tools/ab"
make -C "$root/mocopci_amd/csrc" -s -j8 O="$root/build/$name" OUT="$root/tools/ab/lib$name.so" EXTRA="$*"
echo "built tools/ab/lib$name.so"
