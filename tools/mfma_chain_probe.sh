#!/bin/bash
# GPU box: interleaved against chained MFMA issue order, registers only (tools/mfma_chain_probe.hip).
# Usage: tools/mfma_chain_probe.sh [FILE_FOR_THE_TABLE [ITERATIONS]] — the table goes to stdout and, if named, to the file.
# The binary tools/mfma_chain_probe (git-ignored) is built where hipcc is and reused when it is already there:
#   hipcc --offload-arch=gfx950 -O3 -o tools/mfma_chain_probe tools/mfma_chain_probe.hip
set -u -o pipefail
TABLE=${1:-/dev/null}
[ -x tools/mfma_chain_probe ] || /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -o tools/mfma_chain_probe tools/mfma_chain_probe.hip || exit 1
timeout -k 10 240 tools/mfma_chain_probe ${2:-160000} 2>&1 | tee "$TABLE"
