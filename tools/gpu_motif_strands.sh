#!/bin/bash
# the both-strand site state at BASELINE cfg 3 from files (tools/motif_strands_probe.py): the command cold and again, the host-side join of
# two motif_sites exports against the strands kernel, one kernel trace of the count pass beside compare_kernel's on the same candidates with
# both slots equal; output under ${OUT_DIR:-runs}/motif_strands.  Every GPU step under its own time limit, nothing is started after a step
# that failed.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_DIR:-runs}/motif_strands
BP=${1:-100000000}
mkdir -p $OUT
BASE=/dev/shm
NEED_KB=$((BP / 1000 * 90))                                             # one pileup of about 75 bytes per bp, the assembly, the outputs
[ -d $BASE ] && [ -w $BASE ] && [ "$(df -k --output=avail $BASE | tail -1)" -gt $NEED_KB ] || BASE=${TMPDIR:-/tmp}
TMP=$(mktemp -d $BASE/nm_st_XXXXXX) || exit 1
trap 'rm -rf "$TMP"' EXIT
timeout -k 10 420 python tools/motif_strands_probe.py files $TMP --total-bp $BP > $OUT/files.json 2> $OUT/files.log \
 && timeout -k 10 240 python tools/motif_strands_probe.py engine $TMP > $OUT/engine.json 2> $OUT/engine.log \
 && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o strands -- python tools/motif_strands_probe.py trace $TMP > $OUT/trace.json 2> $OUT/trace.log
rc=$?
echo "rc=$rc base=$BASE"
tail -n 3 $OUT/files.json $OUT/engine.json $OUT/trace.json 2>/dev/null | cut -c1-2500
[ $rc -ne 0 ] && tail -n 15 $OUT/files.log $OUT/engine.log $OUT/trace.log 2>/dev/null | cut -c1-400
find $OUT/trace -name "*kernel_stats.csv" | head -1 | xargs -r grep -E "Name|strands_kernel|compare_kernel" | cut -c1-260
# every dispatch of the two count kernels: name, duration in ns
find $OUT/trace -name "*kernel_trace.csv" | head -1 | xargs -r python -c '
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "strands_kernel" in r["Kernel_Name"] or "compare_kernel" in r["Kernel_Name"]:
        print(r["Kernel_Name"][:60], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
'
find $OUT/trace -name "*.db" -delete 2>/dev/null
exit $rc
