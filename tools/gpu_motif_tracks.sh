#!/bin/bash
# motif methylation along contigs at BASELINE cfg 3 from files (tools/motif_tracks_probe.py): the command as a cold process at --window 128,
# 4096 and 65536, and one kernel trace of tracks_kernel at those window sizes beside sites_kernel's count pass on the same candidates;
# output under ${OUT_DIR:-runs}/motif_tracks.  Every GPU step under its own time limit, nothing is started after a step that failed.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_DIR:-runs}/motif_tracks
BP=${1:-100000000}
mkdir -p $OUT
BASE=/dev/shm
NEED_KB=$((BP / 1000 * 90))                                             # one pileup of about 75 bytes per bp, the assembly, the outputs
[ -d $BASE ] && [ -w $BASE ] && [ "$(df -k --output=avail $BASE | tail -1)" -gt $NEED_KB ] || BASE=${TMPDIR:-/tmp}
TMP=$(mktemp -d $BASE/nm_tr_XXXXXX) || exit 1
trap 'rm -rf "$TMP"' EXIT
timeout -k 10 480 python tools/motif_tracks_probe.py files $TMP --total-bp $BP > $OUT/files.json 2> $OUT/files.log \
 && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o tracks -- python tools/motif_tracks_probe.py trace $TMP > $OUT/trace.json 2> $OUT/trace.log
rc=$?
echo "rc=$rc base=$BASE"
tail -n 3 $OUT/files.json $OUT/trace.json 2>/dev/null | cut -c1-4000
[ $rc -ne 0 ] && tail -n 15 $OUT/files.log $OUT/trace.log 2>/dev/null | cut -c1-400
find $OUT/trace -name "*kernel_stats.csv" | head -1 | xargs -r grep -E "Name|tracks_kernel|sites_kernel" | cut -c1-260
# every dispatch of the two count kernels: name, duration in ns
find $OUT/trace -name "*kernel_trace.csv" | head -1 | xargs -r python -c '
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "tracks_kernel" in r["Kernel_Name"] or "sites_kernel" in r["Kernel_Name"]:
        print(r["Kernel_Name"][:60], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
'
find $OUT/trace -name "*.db" -delete 2>/dev/null
exit $rc
