#!/bin/bash
# runs of same-state motif sites at BASELINE cfg 3 from files (tools/motif_runs_probe.py): the command cold and again, and one kernel
# trace of runs_kernel's count and fill passes and of the stitch beside sites_kernel's count pass on the same candidates, then on the
# one-letter background candidates; output under ${OUT_DIR:-runs}/motif_runs.  Every GPU step under its own time limit, nothing is
# started after a step that failed.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_DIR:-runs}/motif_runs
BP=${1:-100000000}
mkdir -p $OUT
BASE=/dev/shm
NEED_KB=$((BP / 1000 * 90))                                             # one pileup of about 75 bytes per bp, the assembly, the outputs
[ -d $BASE ] && [ -w $BASE ] && [ "$(df -k --output=avail $BASE | tail -1)" -gt $NEED_KB ] || BASE=${TMPDIR:-/tmp}
TMP=$(mktemp -d $BASE/nm_runs_XXXXXX) || exit 1
trap 'rm -rf "$TMP"' EXIT
timeout -k 10 420 python tools/motif_runs_probe.py files $TMP --total-bp $BP > $OUT/files.json 2> $OUT/files.log \
 && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o runs -- python tools/motif_runs_probe.py trace $TMP > $OUT/trace.json 2> $OUT/trace.log
rc=$?
echo "rc=$rc base=$BASE"
tail -n 3 $OUT/files.json $OUT/trace.json 2>/dev/null | cut -c1-6000
[ $rc -ne 0 ] && tail -n 15 $OUT/files.log $OUT/trace.log 2>/dev/null | cut -c1-400
find $OUT/trace -name "*kernel_stats.csv" | head -1 | xargs -r grep -E "Name|runs_|sites_kernel" | cut -c1-260
# the passes of the traced kernels in time order with their summed time, in microseconds (no GPU: the trace is read against calls.json)
CSV=$(find $OUT/trace -name "*kernel_trace.csv" | head -1)
[ $rc -eq 0 ] && [ -n "$CSV" ] && python tools/motif_runs_probe.py table $TMP --trace-csv "$CSV" | tee $OUT/table.json
find $OUT/trace -name "*.db" -delete 2>/dev/null
exit $rc
