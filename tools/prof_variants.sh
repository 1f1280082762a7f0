#!/bin/bash
# The variant calls under the profiler (needs an MI355X), each in a run of its own, merged into profiles/variants_bench.json
# (written before by `python tools/variants_bench.py`):
#   kernel times    rocprofv3 --kernel-trace --stats around the dense leg and around the hits leg
#   LDS counters    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE around the dense leg, counters only
#   bash tools/prof_variants.sh [DIR for the profiler's files and logs; default: a fresh temporary directory]
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$(mktemp -d)}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
cd /tmp && export TMPDIR=/tmp
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/dense" -o v -- \
    python "$ROOT/tools/variants_bench.py" --only dense --runs 5 > "$OUT/dense.log" 2>&1 || { tail -5 "$OUT/dense.log"; exit 1; }
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/hits" -o v -- \
    python "$ROOT/tools/variants_bench.py" --only hits --runs 2 > "$OUT/hits.log" 2>&1 || { tail -5 "$OUT/hits.log"; exit 1; }
timeout -k 10 240 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d "$OUT/pmc" -o v -- \
    python "$ROOT/tools/variants_bench.py" --only dense --runs 3 > "$OUT/pmc.log" 2>&1 || { tail -5 "$OUT/pmc.log"; exit 1; }
python "$ROOT/tools/variants_bench.py" --merge-kernel-stats "$OUT/dense" --merge-kernel-stats "$OUT/hits" --merge-pmc "$OUT/pmc"
