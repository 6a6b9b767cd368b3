// Stand-alone dump of the heavy kernels' work lists (nanomotif_amd/csrc/nmscore_worklist.h) for a geometry read from a file, so
// that tests/test_score_tail_pack_host.py can hold them against its own restatement.  No device, no library.
// Build: g++ -O2 -std=c++17 driver.cpp -o worklist_dump; run: ./worklist_dump geometry.txt
// Input (whitespace separated): n_bins seg_chunks n_chunks n_contigs, then per contig in upload order: bin length first_chunk,
// then n_chunks needs_v bytes as 0 / 1.  Output, once for the plain list ("list 0") and once with tails packed ("list 1"):
//     list <pack> <entries> <rows> <segments>
//     entries: ...          strips: ...          segs: x y z w ...          bin_start: ...          bin_len: ...
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <numeric>

#include "../../nanomotif_amd/csrc/nmscore_worklist.h"

using namespace nmdetail;

static void dump(const char *what, const std::vector<uint32_t> &v) {
    printf("%s:", what);
    for (uint32_t x : v) printf(" %" PRIu32, x);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s geometry.txt\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "r");
    if (!in) { perror(argv[1]); return 2; }
    uint32_t n_bins = 0, seg_chunks = 0, n_chunks = 0, n_contigs = 0;
    if (fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &n_bins, &seg_chunks, &n_chunks, &n_contigs) != 4 || !n_bins || !seg_chunks) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<uint32_t> bin(n_contigs), chunk(n_contigs);
    std::vector<uint64_t> len(n_contigs);
    for (uint32_t i = 0; i < n_contigs; ++i)
        if (fscanf(in, "%" SCNu32 " %" SCNu64 " %" SCNu32, &bin[i], &len[i], &chunk[i]) != 3 || bin[i] >= n_bins) { fprintf(stderr, "bad contig %u\n", i); return 2; }
    std::vector<uint8_t> needs_v(n_chunks);
    for (uint32_t ch = 0; ch < n_chunks; ++ch) {
        unsigned v = 0;
        if (fscanf(in, "%u", &v) != 1) { fprintf(stderr, "bad needs_v %u\n", ch); return 2; }
        needs_v[ch] = (uint8_t)v;
    }
    fclose(in);
    std::vector<uint32_t> order(n_contigs);             // as nm_upload_contigs groups them: by bin, upload order inside a bin
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return bin[x] < bin[y]; });
    for (int pack = 0; pack < 2; ++pack) {
        WorkList wl;
        build_work_list(wl, pack == 1, n_bins, n_contigs, order.data(), bin.data(), len.data(), chunk.data(), needs_v.data(), n_chunks, seg_chunks);
        printf("list %d %zu %zu %zu\n", pack, wl.entries.size(), wl.strip_rows.size() / WORK_STRIPS, wl.segs.size());
        dump("entries", wl.entries);
        dump("strips", wl.strip_rows);
        std::vector<uint32_t> flat;
        for (const PlanU4 &s : wl.segs) { flat.push_back(s.x); flat.push_back(s.y); flat.push_back(s.z); flat.push_back(s.w); }
        dump("segs", flat);
        dump("bin_start", wl.bin_start);
        dump("bin_len", wl.bin_len);
    }
    return 0;
}
