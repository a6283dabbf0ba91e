#!/bin/bash
# Per-kernel register / occupancy report of one HIP source (hipcc remarks, the flags of the build):  tools/kernel_resources.sh <file.hip> [grep-filter]
FLAGS=$(PYTHONPATH="$(dirname "$0")/.." python -c 'import msod_amd; from msod_amd import _lib; print(" ".join(_lib.HIPCC_FLAGS))') || exit 1
hipcc $FLAGS -c -o /dev/null "$1" -Rpass-analysis=kernel-resource-usage 2>&1 \
 | grep -E "Function Name|  VGPRs:|AGPRs:|ScratchSize|Occupancy" \
 | sed -E 's/.*remark: +//; s/ \[-Rpass.*//' | paste - - - - - | c++filt | grep -E "${2:-.}"
