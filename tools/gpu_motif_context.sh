#!/bin/bash
# the sequence context of motif sites at BASELINE cfg 3 from files (tools/motif_context_probe.py): the command cold and again, and one kernel
# trace of context_kernel (radius 10) in both reductions beside profile_kernel with one target and sites_kernel's count pass on the same
# candidates; output under ${OUT_DIR:-runs}/motif_context.  Every GPU step under its own time limit, nothing is started after a step that failed.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_DIR:-runs}/motif_context
BP=${1:-100000000}
mkdir -p $OUT
BASE=/dev/shm
NEED_KB=$((BP / 1000 * 90))                                             # one pileup of about 75 bytes per bp, the assembly, the outputs
[ -d $BASE ] && [ -w $BASE ] && [ "$(df -k --output=avail $BASE | tail -1)" -gt $NEED_KB ] || BASE=${TMPDIR:-/tmp}
TMP=$(mktemp -d $BASE/nm_cx_XXXXXX) || exit 1
trap 'rm -rf "$TMP"' EXIT
timeout -k 10 420 python tools/motif_context_probe.py files $TMP --total-bp $BP > $OUT/files.json 2> $OUT/files.log \
 && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o context -- python tools/motif_context_probe.py trace $TMP > $OUT/trace.json 2> $OUT/trace.log
rc=$?
echo "rc=$rc base=$BASE"
tail -n 3 $OUT/files.json $OUT/trace.json 2>/dev/null | cut -c1-4000
[ $rc -ne 0 ] && tail -n 15 $OUT/files.log $OUT/trace.log 2>/dev/null | cut -c1-400
find $OUT/trace -name "*kernel_stats.csv" | head -1 | xargs -r grep -E "Name|context_kernel|profile_kernel|sites_kernel" | cut -c1-260
# every dispatch of the three count kernels in order: name, duration in ns (context_kernel: two calls through LDS, then two with wave atomics)
find $OUT/trace -name "*kernel_trace.csv" | head -1 | xargs -r python -c '
import csv, sys
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
for r in rows:
    if any(k in r["Kernel_Name"] for k in ("context_kernel", "profile_kernel", "sites_kernel")):
        print(r["Kernel_Name"][:60], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
'
find $OUT/trace -name "*.db" -delete 2>/dev/null
exit $rc
