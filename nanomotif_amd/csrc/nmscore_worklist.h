// The work lists of the heavy scoring kernels (score_kernel, the non-CF non-PC variants), built once per uploaded assembly.
// A heavy wave scores 64 lane strips of 128 bp of ONE bin; nothing crosses lanes before the LDS counters, so the strips need
// not be consecutive.  A bin's list therefore holds
//     its chunks whose 64 strips all hold sequence, in contig and chunk order:    chunk | need_v << 30
//     then its packed rows, 64 strips taken from the partly filled chunks:        1u << 31 | row
// and strip_rows[row * 64 + lane] is the word index of the strip lane `lane` of that row scores (chunk * 256 + strip * 4),
// or WORK_NO_STRIP for the lanes left over in a bin's last row.  Only strips that hold at least one bp of a contig are listed:
// a contig's last chunk is walked by as many lanes as it has such strips.  The PLAIN list (pack = false) has every chunk that
// holds sequence as an entry and no rows: the second opinion of the tests and the A/B switch NM_SCORE_PACK_TAILS=0.  Neither
// list holds a chunk with nothing but the gap behind a contig in it (one contig in 85 ends less than 96 bp short of a chunk).
// The segment table cuts each bin's list positions into runs of seg_chunks entries, as the chunk table cuts chunks.
// Pure integer work over plain inputs (tools/plan_check/driver.cpp, tests/test_score_tail_pack_host.py).
#pragma once
#include <cstdint>
#include <vector>

#include "nmscore_plan.h"

namespace nmdetail {

constexpr uint32_t WORK_CHUNK_BP = 8192, WORK_STRIP_BP = 128, WORK_STRIPS = 64, WORK_CHUNK_WORDS = 256, WORK_GAP_BP = 96;
constexpr uint32_t WORK_NEED_V = 1u << 30, WORK_PACKED = 1u << 31, WORK_NO_STRIP = 0xFFFFFFFFu;

struct WorkList {
    std::vector<uint32_t> entries;                      // work_list, contiguous per bin
    std::vector<uint32_t> strip_rows;                   // 64 per packed row
    std::vector<PlanU4> segs;                           // {first entry, count <= seg_chunks, bin, 0}
    std::vector<uint32_t> bin_start, bin_len;           // per bin: its entries
};

// strips of chunk q of a contig of `len` bp that hold at least one of its bp
inline uint32_t work_strips_of(uint64_t len, uint64_t q) {
    const uint64_t at = q * WORK_CHUNK_BP;
    if (len <= at) return 0;
    return (uint32_t)std::min<uint64_t>(WORK_STRIPS, (len - at + WORK_STRIP_BP - 1) / WORK_STRIP_BP);
}

// order: the contigs sorted by bin (stable: upload order inside a bin); contig_chunk: first chunk of every contig; needs_v: one
// byte per chunk of the space (n_chunks of them), as needs_v_kernel wrote it.  A space of more than 2^32 words has no u32 strip
// index: its packed list is the plain one.
inline void build_work_list(WorkList &wl, bool pack, uint32_t n_bins, uint32_t n_contigs, const uint32_t *order, const uint32_t *contig_bin,
                            const uint64_t *contig_len, const uint32_t *contig_chunk, const uint8_t *needs_v, uint32_t n_chunks, uint32_t seg_chunks) {
    if ((uint64_t)n_chunks * WORK_CHUNK_WORDS > 0xFFFFFFFFull) pack = false;
    wl.entries.clear();
    wl.strip_rows.clear();
    wl.segs.clear();
    wl.bin_start.assign(n_bins, 0);
    wl.bin_len.assign(n_bins, 0);
    uint32_t oi = 0;
    for (uint32_t b = 0; b < n_bins; ++b) {
        const uint32_t start = (uint32_t)wl.entries.size();
        const size_t row0 = wl.strip_rows.size() / WORK_STRIPS;
        for (; oi < n_contigs && contig_bin[order[oi]] == b; ++oi) {
            const uint32_t i = order[oi];
            const uint64_t nch = (contig_len[i] + WORK_GAP_BP + WORK_CHUNK_BP - 1) / WORK_CHUNK_BP;
            for (uint64_t q = 0; q < nch; ++q) {
                const uint32_t chunk = contig_chunk[i] + (uint32_t)q, strips = work_strips_of(contig_len[i], q);
                if (strips == 0) continue;              // nothing but the gap behind the contig
                if (!pack || strips == WORK_STRIPS) wl.entries.push_back(chunk | (needs_v[chunk] ? WORK_NEED_V : 0u));
                else for (uint32_t s = 0; s < strips; ++s) wl.strip_rows.push_back(chunk * WORK_CHUNK_WORDS + s * 4);
            }
        }
        while (wl.strip_rows.size() % WORK_STRIPS) wl.strip_rows.push_back(WORK_NO_STRIP);
        for (size_t row = row0; row < wl.strip_rows.size() / WORK_STRIPS; ++row) wl.entries.push_back(WORK_PACKED | (uint32_t)row);
        wl.bin_start[b] = start;
        wl.bin_len[b] = (uint32_t)wl.entries.size() - start;
        for (uint32_t k = 0; k < wl.bin_len[b]; k += seg_chunks)
            wl.segs.push_back(PlanU4{start + k, std::min<uint32_t>(seg_chunks, wl.bin_len[b] - k), b, 0});
    }
}

}  // namespace nmdetail
