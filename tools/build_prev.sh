#!/bin/bash
# Builds the library of a previous commit next to the current one for same-box A/B runs:
#   tools/build_prev.sh [rev]   ->  lightmotif_amd/csrc/liblightmotif_hip_prev.so
# (select it at run time with LM_HIP_LIBRARY=lightmotif_amd/csrc/liblightmotif_hip_prev.so)
# The revision is checked out into a work directory and built by ITS OWN lightmotif_amd/build.py, so this script knows
# nothing about translation units.  Needs git: run it where the repository is, the library it makes travels with the tree.
set -euo pipefail
REV=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=$ROOT/gpurun_out/prev_src
rm -rf "$W"
mkdir -p "$W"
git -C "$ROOT" archive "$REV" | tar -x -C "$W"
(cd "$W" && python -m lightmotif_amd.build --force)
cp "$W/lightmotif_amd/csrc/liblightmotif_hip.so" "$ROOT/lightmotif_amd/csrc/liblightmotif_hip_prev.so"
echo "built $ROOT/lightmotif_amd/csrc/liblightmotif_hip_prev.so from $(git -C "$ROOT" rev-parse --short "$REV")"
