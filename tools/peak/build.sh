#!/bin/bash
# builds the matrix-pipe measurement helper into build/libmfma_peak.so (gfx950)
set -e
cd "$(dirname "$0")/../.."
mkdir -p build
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -o build/libmfma_peak.so tools/peak/mfma_peak.hip
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -o build/libsync_latency.so tools/peak/sync_latency.hip
# the MFMA gap probe: a program of its own, built with the library's flags (FLAGS of mocopci_amd/csrc/Makefile); its device assembly is
# kept as profiles/mfma_gap_probe.s, the record that every gap holds exactly F fillers and no packed-fp32 instruction
LIBFLAGS="-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -fno-vectorize -Wall -Wno-unused-function -mllvm -amdgpu-mfma-vgpr-form"
/opt/rocm/bin/hipcc $LIBFLAGS -o build/mfma_gap_probe tools/peak/mfma_gap_probe.hip
/opt/rocm/bin/hipcc $LIBFLAGS --cuda-device-only -S -o profiles/mfma_gap_probe.s tools/peak/mfma_gap_probe.hip
