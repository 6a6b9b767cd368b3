#!/bin/bash
# per-site read counts at BASELINE cfg 3 from files (tools/motif_pileup_probe.py): the command as a cold process with and without
# --all_occurrences, and one kernel trace of pileup_kernel's count pass beside fractions_kernel and of its fill pass beside
# sites_kernel<.., true> on the same candidates, five repetitions each; output under ${OUT_DIR:-runs}/motif_pileup.  NM_LIB=<path> traces
# another build of the library.  Every GPU step under its own time limit, nothing is started after a step that failed.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_DIR:-runs}/motif_pileup
BP=${1:-100000000}
mkdir -p $OUT
BASE=/dev/shm
NEED_KB=$((BP / 1000 * 120))                                            # one pileup of about 75 bytes per bp, the assembly, the outputs
[ -d $BASE ] && [ -w $BASE ] && [ "$(df -k --output=avail $BASE | tail -1)" -gt $NEED_KB ] || BASE=${TMPDIR:-/tmp}
TMP=$(mktemp -d $BASE/nm_pu_XXXXXX) || exit 1
trap 'rm -rf "$TMP"' EXIT
timeout -k 10 480 python tools/motif_pileup_probe.py files $TMP --total-bp $BP > $OUT/files.json 2> $OUT/files.log \
 && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o pileup -- python tools/motif_pileup_probe.py trace $TMP > $OUT/trace.json 2> $OUT/trace.log
rc=$?
echo "rc=$rc base=$BASE"
tail -n 3 $OUT/files.json $OUT/trace.json 2>/dev/null | cut -c1-4000
[ $rc -ne 0 ] && tail -n 15 $OUT/files.log $OUT/trace.log 2>/dev/null | cut -c1-400
# per kernel the median of its dispatches, in microseconds (no GPU: the trace is read)
CSV=$(find $OUT/trace -name "*kernel_trace.csv" | head -1)
[ $rc -eq 0 ] && [ -n "$CSV" ] && python tools/motif_pileup_probe.py table "$CSV" | tee $OUT/table.json
find $OUT/trace -name "*.db" -delete 2>/dev/null
exit $rc
