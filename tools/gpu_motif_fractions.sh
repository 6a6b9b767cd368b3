#!/bin/bash
# read-fraction histograms at BASELINE cfg 3 from files (tools/motif_fractions_probe.py): the command as a cold process at --bins 20 and 64 on
# the synthetic pileup and on a bimodal one, and one kernel trace per pileup of fractions_kernel at both bin counts beside sites_kernel's
# count pass on the same candidates; output under ${OUT_DIR:-runs}/motif_fractions.  NM_LIB=<path> traces another build of the library.
# Every GPU step under its own time limit, nothing is started after a step that failed.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_DIR:-runs}/motif_fractions
BP=${1:-100000000}
mkdir -p $OUT
BASE=/dev/shm
NEED_KB=$((BP / 1000 * 170))                                            # two pileups of about 75 bytes per bp, the assembly, the outputs
[ -d $BASE ] && [ -w $BASE ] && [ "$(df -k --output=avail $BASE | tail -1)" -gt $NEED_KB ] || BASE=${TMPDIR:-/tmp}
TMP=$(mktemp -d $BASE/nm_fr_XXXXXX) || exit 1
trap 'rm -rf "$TMP"' EXIT
timeout -k 10 600 python tools/motif_fractions_probe.py files $TMP --total-bp $BP > $OUT/files.json 2> $OUT/files.log \
 && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_uniform -o fractions -- python tools/motif_fractions_probe.py trace $TMP --pileup pileup.bed > $OUT/trace_uniform.json 2> $OUT/trace_uniform.log \
 && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_bimodal -o fractions -- python tools/motif_fractions_probe.py trace $TMP --pileup pileup_bimodal.bed > $OUT/trace_bimodal.json 2> $OUT/trace_bimodal.log
rc=$?
echo "rc=$rc base=$BASE"
tail -n 3 $OUT/files.json $OUT/trace_uniform.json $OUT/trace_bimodal.json 2>/dev/null | cut -c1-6000
[ $rc -ne 0 ] && tail -n 15 $OUT/files.log $OUT/trace_uniform.log $OUT/trace_bimodal.log 2>/dev/null | cut -c1-400
# every dispatch of the two count kernels: name, duration in ns
for t in uniform bimodal; do
    echo "== $t"
    find $OUT/trace_$t -name "*kernel_trace.csv" | head -1 | xargs -r python -c '
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "fractions_kernel" in r["Kernel_Name"] or "sites_kernel" in r["Kernel_Name"]:
        print(r["Kernel_Name"][:70], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
'
done
find $OUT -name "*.db" -delete 2>/dev/null
exit $rc
