#!/bin/bash
# Build libcft_hip.so for gfx950 (or CFT_OUT) with the package's own recipe, _lib.build(): needs python with torch, like the package.
# Arguments are extra flags of every compile and of the link.  Exits non-zero (and removes a stale library) on any compile error.
set -e
cd "$(dirname "$0")/.."
OUT=${CFT_OUT:-multispectral-object-detection_amd/libcft_hip.so}
rm -f "$OUT"
python -c 'import os, sys, msod_amd; from msod_amd import _lib; _lib.build(verbose=True, out=os.environ.get("CFT_OUT") or None, extra_flags=sys.argv[1:])' "$@"
ls -la "$OUT"
