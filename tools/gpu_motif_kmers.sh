#!/bin/bash
# the k-mer methylation table at BASELINE cfg 3 from files and on an input with a homopolymer (tools/motif_kmers_probe.py): the command cold, and
# one kernel trace of kmer_kernel at F = 0 .. 10 on both reduction paths and at runs of 4, 16 and 64 chunks beside sites_kernel's count pass on
# the one-letter motifs of the same bins; output under ${OUT_DIR:-runs}/motif_kmers (table.md: the times and ratios).  Every GPU step under
# its own time limit, nothing is started after a step that failed.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_DIR:-runs}/motif_kmers
BP=${1:-100000000}
mkdir -p $OUT
BASE=/dev/shm
NEED_KB=$((BP / 1000 * 90))                                             # one pileup of about 75 bytes per bp, the assembly, the outputs
[ -d $BASE ] && [ -w $BASE ] && [ "$(df -k --output=avail $BASE | tail -1)" -gt $NEED_KB ] || BASE=${TMPDIR:-/tmp}
TMP=$(mktemp -d $BASE/nm_km_XXXXXX) || exit 1
trap 'rm -rf "$TMP"' EXIT
timeout -k 10 420 python tools/motif_kmers_probe.py files $TMP --total-bp $BP > $OUT/files.json 2> $OUT/files.log \
 && timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d $OUT/trace -o kmers -- python tools/motif_kmers_probe.py trace $TMP > $OUT/trace.json 2> $OUT/trace.log
rc=$?
echo "rc=$rc base=$BASE"
tail -n 3 $OUT/files.json $OUT/trace.json 2>/dev/null | cut -c1-4000
[ $rc -ne 0 ] && tail -n 15 $OUT/files.log $OUT/trace.log 2>/dev/null | cut -c1-400
# (no GPU) the dispatches of the two kernels matched to the calls in order
[ $rc -eq 0 ] && find $OUT/trace -name "*kernel_trace.csv" | head -1 | xargs -r python tools/motif_kmers_probe.py table $TMP > $OUT/table.md && cat $OUT/table.md
find $OUT/trace -name "*.db" -delete 2>/dev/null
exit $rc
