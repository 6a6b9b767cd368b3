#!/bin/bash
# the coverage report at BASELINE cfg 3 from files (tools/motif_coverage_probe.py): the two commands, the host-side set algebra over
# motif_sites records against the set kernel, one kernel trace; output under ${OUT_DIR:-runs}/motif_coverage.  Every GPU step under its
# own time limit, nothing is started after a step that failed.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_DIR:-runs}/motif_coverage
BP=${1:-100000000}
mkdir -p $OUT
BASE=/dev/shm
[ -d $BASE ] && [ -w $BASE ] || BASE=${TMPDIR:-/tmp}
TMP=$(mktemp -d $BASE/nm_cov_XXXXXX) || exit 1
trap 'rm -rf "$TMP"' EXIT
timeout -k 10 420 python tools/motif_coverage_probe.py files $TMP --total-bp $BP > $OUT/files.json 2> $OUT/files.log \
 && timeout -k 10 300 python tools/motif_coverage_probe.py engine $TMP > $OUT/engine.json 2> $OUT/engine.log \
 && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o coverage -- python tools/motif_coverage_probe.py trace $TMP > $OUT/trace.json 2> $OUT/trace.log
rc=$?
echo "rc=$rc"
tail -n 3 $OUT/files.json $OUT/engine.json $OUT/trace.json 2>/dev/null | cut -c1-1500
find $OUT/trace -name "*kernel_stats.csv" | head -1 | xargs -r head -12 | cut -c1-220
find $OUT/trace -name "*.db" -delete 2>/dev/null
exit $rc
