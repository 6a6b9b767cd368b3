// Coverage of a bin's methylation by a SET of motifs: what share of the confidently methylated positions of a (bin, mod type) lies
// on an occurrence of at least one motif of the set, which motifs are redundant, and where the unexplained positions are.  The
// reference has this only as a log line of find_best_candidates ("x % of sequences remaining", find_motifs_bin.py:801-823), taken
// before pruning and merging and never written to a file.  Coverage is DEFINED by nm_motif_sites (nmsites.hip): candidate j covers
// (contig, position, strand) iff that export, with all three states, writes a record for j there — same eval_strand over the same
// tile, so there is no second matcher.  The count / scan / fill scaffold of nmexport.h, with
//   count  per work item = (set, chunk of the set's bin): load the chunk and the slot's four state planes once, then walk the set's
//          candidates with wave-uniform control flow; per strand two accumulators, multi |= any & a; any |= a, so that
//          cover = any and once = any & ~multi.  Ten set counts per (set, contig) row; a second walk over the same candidates
//          (chunk still in registers, programs through the scalar cache again) gives a & once per candidate: four exclusive
//          counts per (candidate, contig) row.  The number of unexplained records M & ~cover of the work item goes to the item table.
//   fill   cover is computed again and every unexplained position M & ~cover is a record; its code is 0, NM_SITES_MINUS on the reverse strand
// A set runs at the width (word-groups G = 1, 2, 3 either side of the modified base) of its widest candidate, the programs of the
// narrower ones sliced to that width: at most 3 + 1 + 1 + 3 = 8 launches whatever the number of sets and candidates.
#include "nmexport.h"

using namespace nmdetail;

namespace {

struct CovArgs : ExportArgs {
    const uint32_t *set_row0;            // first row of the set in the (set, contig) table
    const uint32_t *set_cand0;           // [n_sets + 1] first candidate of a set
    const unsigned long long *set_planes;    // [n_sets][4] MP UP MM UM of the set's mod slot
    const uint32_t *cand_row0;           // first row of a candidate in the (candidate, contig) table
    unsigned long long *set_table;       // count pass: [row][10]
    unsigned long long *cand_table;      // count pass: [row][4]
};

template <int G, bool FILL>
__global__ __launch_bounds__(256) void coverage_kernel(CovArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<FILL>(a, w)) return;
    const uint32_t s = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.set_planes + (size_t)s * 4)};
    RawChunk<K> raw;
    raw.load(a.seq, stp, w.chunk, lane);
    Tile<K> tile;
    tile.expand(raw);
    const uint32_t c0 = ((cu32p)a.set_cand0)[s], c1 = ((cu32p)a.set_cand0)[s + 1];
    uint32_t anyf[T_WORDS], anyr[T_WORDS], multif[T_WORDS], multir[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) anyf[t] = anyr[t] = multif[t] = multir[t] = 0u;
    for (uint32_t k = c0; k < c1; ++k) {                                // wave-uniform
        uint32_t af[T_WORDS], ar[T_WORDS];                              // (written out, not walk_strands: profiles/r19/export_prologue.md)
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) af[t] = ar[t] = 0xFFFFFFFFu;
        const cu32p prog = (cu32p)(a.programs + (size_t)k * PROG6_DW);
        eval_strand<K>(prog, tile, af);
        eval_strand<K>(prog + K::PDW, tile, ar);
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            if (!FILL) { multif[t] |= anyf[t] & af[t]; multir[t] |= anyr[t] & ar[t]; }
            anyf[t] |= af[t];
            anyr[t] |= ar[t];
        }
    }
    if (!FILL) {
        uint32_t c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, n = 0, once = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            const uint32_t mp = raw.s[0][0][t], up = raw.s[0][1][t] & ~mp, mm = raw.s[0][2][t], um = raw.s[0][3][t] & ~mm;
            c[0] += __popc(mp); c[1] += __popc(mp & anyf[t]); c[2] += __popc(up); c[3] += __popc(up & anyf[t]); c[4] += __popc(anyf[t] & ~(mp | up));
            c[5] += __popc(mm); c[6] += __popc(mm & anyr[t]); c[7] += __popc(um); c[8] += __popc(um & anyr[t]); c[9] += __popc(anyr[t] & ~(mm | um));
            n += __popc(mp & ~anyf[t]) + __popc(mm & ~anyr[t]);
            multif[t] = anyf[t] & ~multif[t];                           // from here on: once
            multir[t] = anyr[t] & ~multir[t];
            once |= multif[t] | multir[t];
        }
        for (int o = 32; o; o >>= 1) {
            n += __shfl_xor(n, o);
#pragma unroll
            for (int j = 0; j < 10; ++j) c[j] += __shfl_xor(c[j], o);
        }
        const uint32_t rank = ((cu32p)a.chunk_rank)[w.chunk];
        if (lane == 0) {
            a.item_cnt[w.item] = n;
            unsigned long long *row = a.set_table + ((size_t)((cu32p)a.set_row0)[s] + rank) * 10;
#pragma unroll
            for (int j = 0; j < 10; ++j)
                if (c[j]) atomicAdd(row + j, (unsigned long long)c[j]);
        }
        if (__ballot(once != 0) == 0) return;                           // no position of the chunk is covered exactly once
        // ---- second walk: every candidate's share of `once` (the accumulators start from it instead of all ones)
        for (uint32_t k = c0; k < c1; ++k) {                            // wave-uniform
            uint32_t af[T_WORDS], ar[T_WORDS];
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) { af[t] = multif[t]; ar[t] = multir[t]; }
            const cu32p prog = (cu32p)(a.programs + (size_t)k * PROG6_DW);
            eval_strand<K>(prog, tile, af);
            eval_strand<K>(prog + K::PDW, tile, ar);
            uint32_t e[4] = {0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) {
                const uint32_t mp = raw.s[0][0][t], up = raw.s[0][1][t] & ~mp, mm = raw.s[0][2][t], um = raw.s[0][3][t] & ~mm;
                e[0] += __popc(af[t] & mp); e[1] += __popc(af[t] & up); e[2] += __popc(ar[t] & mm); e[3] += __popc(ar[t] & um);
            }
            for (int o = 32; o; o >>= 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] += __shfl_xor(e[j], o);
            }
            if (lane == 0) {
                unsigned long long *row = a.cand_table + ((size_t)((cu32p)a.cand_row0)[k] + rank) * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e[j]) atomicAdd(row + j, (unsigned long long)e[j]);
            }
        }
        return;
    }
    emit_records(
        a, w, lane, [&](int t, uint32_t &f, uint32_t &r) { f = raw.s[0][0][t] & ~anyf[t]; r = raw.s[0][2][t] & ~anyr[t]; },
        [](int, uint32_t, bool minus) { return minus ? (uint32_t)NM_SITES_MINUS : 0u; });
}

template <bool FILL>
constexpr ExportKernels<CovArgs> coverage_kernels = {coverage_kernel<1, FILL>, coverage_kernel<2, FILL>, coverage_kernel<3, FILL>};
using CovBatch = ExportBatch<CovArgs>;

// validate the sets, compile the programs, stage the tables and enqueue the count pass (and, with_scan, the prefix + gather).
// set_row_offset / cand_row_offset NULL (the export of records): the tables are laid out here, one row per resident contig.
int coverage_begin(CovBatch &cb, nm_ctx *c, uint32_t n_sets, const uint32_t *set_bin, const uint8_t *set_mod_slot, const uint32_t *set_cand_offset,
                   const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                   const uint64_t *set_row_offset, const uint64_t *cand_row_offset, bool with_scan) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (!set_bin || !set_mod_slot || !set_cand_offset) return fail(NM_EINVAL, "NULL argument");
    if (set_cand_offset[0] != 0) return fail(NM_EINVAL, "set_cand_offset[0] must be 0");
    for (uint32_t s = 0; s < n_sets; ++s)
        if (set_cand_offset[s + 1] < set_cand_offset[s]) return fail(NM_EINVAL, "set_cand_offset does not ascend at set %u", s);
    const uint32_t n_cand = set_cand_offset[n_sets];
    if (n_cand && (!cand_len || !cand_modpos || !cand_mask_offset || !cand_masks)) return fail(NM_EINVAL, "NULL argument");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    const bool tables = set_row_offset != nullptr;
    if (tables && (set_row_offset[0] != 0 || cand_row_offset[0] != 0)) return fail(NM_EINVAL, "set_row_offset[0] and cand_row_offset[0] must be 0");
    std::vector<uint32_t> srow0(n_sets, 0), crow0(n_cand, 0), programs((size_t)n_cand * PROG6_DW, 0);
    std::vector<unsigned long long> planes((size_t)n_sets * 4, 0);
    std::vector<uint8_t> set_width(n_sets, 0);
    const Motifs motifs{cand_len, cand_modpos, cand_mask_offset, cand_masks};
    uint64_t items = 0, srows = 0, crows = 0;
    for (uint32_t s = 0; s < n_sets; ++s) {
        const uint32_t bin = set_bin[s];
        if (bin >= c->n_bins) return fail(NM_EINVAL, "set %u: set_bin %u >= n_bins %u", s, bin, c->n_bins);
        int rc = slot_state_planes(c, "set_mod_slot", s, set_mod_slot[s], planes.data() + (size_t)s * 4);
        if (rc) return rc;
        const uint32_t ncontigs = c->bin_ncontigs[bin];
        // the set's width = the reach class of its widest candidate; every program of the set is sliced to THAT width, not to its own
        uint32_t full[PROG6_DW];
        int width = 0, reach = 0;
        for (uint32_t k = set_cand_offset[s]; k < set_cand_offset[s + 1]; ++k) {
            if ((rc = compile_motif(motifs, k, full, &reach))) return rc;
            width = std::max(width, reach);
        }
        for (uint32_t k = set_cand_offset[s]; k < set_cand_offset[s + 1]; ++k) {
            (void)compile_motif(motifs, k, full, &reach);
            slice_program(full, width + 1, programs.data() + (size_t)k * PROG6_DW);
            if (tables && (cand_row_offset[k + 1] < cand_row_offset[k] || cand_row_offset[k + 1] - cand_row_offset[k] < ncontigs))
                return fail(NM_EINVAL, "candidate %u: cand_row_offset gives fewer rows than the %u resident contigs of bin %u (or descends)", k, ncontigs, bin);
            crow0[k] = (uint32_t)(tables ? cand_row_offset[k] : crows);
            crows = tables ? cand_row_offset[k + 1] : crows + ncontigs;
            if (crows >= 0xFFFFFFFFull) return fail(NM_ERANGE, "more than 2^32 (candidate, contig) rows in one call");
        }
        if (tables && (set_row_offset[s + 1] < set_row_offset[s] || set_row_offset[s + 1] - set_row_offset[s] < ncontigs))
            return fail(NM_EINVAL, "set %u: set_row_offset gives fewer rows than the %u resident contigs of bin %u (or descends)", s, ncontigs, bin);
        srow0[s] = (uint32_t)(tables ? set_row_offset[s] : srows);
        srows = tables ? set_row_offset[s + 1] : srows + ncontigs;
        if (srows >= 0xFFFFFFFFull) return fail(NM_ERANGE, "more than 2^32 (set, contig) rows in one call");
        set_width[s] = (uint8_t)width;
        items += c->bin_nchunks[bin];
        if (items >= 0xFFFFFFF0ull) return fail(NM_ERANGE, "more than 2^32 (set, chunk) work items in one call: send fewer sets");
    }
    CovArgs &a = cb.base;
    return export_begin(cb, c, n_sets, set_bin, set_width.data(), programs,
                        {{&a.set_row0, srow0.data(), srow0.size() * 4},
                         {&a.set_cand0, set_cand_offset, (size_t)(n_sets + 1) * 4},
                         {&a.cand_row0, crow0.data(), crow0.size() * 4},
                         {&a.set_planes, planes.data(), planes.size() * 8}},
                        {{&a.set_table, (size_t)srows * 80}, {&a.cand_table, (size_t)crows * 32}}, coverage_kernels<false>, with_scan);
}

}  // namespace

int nm_motif_coverage_count(nm_ctx *c, uint32_t n_sets, const uint32_t *set_bin, const uint8_t *set_mod_slot, const uint32_t *set_cand_offset,
                            const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                            const uint64_t *set_row_offset, const uint64_t *cand_row_offset, uint64_t *set_total, int64_t *set_counts,
                            int64_t *cand_counts) {
    if (!set_cand_offset || !set_row_offset || !cand_row_offset) return fail(NM_EINVAL, "NULL argument");
    if (n_sets == 0) return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    if (!set_total || !set_counts || (set_cand_offset[n_sets] && !cand_counts)) return fail(NM_EINVAL, "NULL argument");
    CovBatch cb;
    const int rc = coverage_begin(cb, c, n_sets, set_bin, set_mod_slot, set_cand_offset, cand_len, cand_modpos, cand_mask_offset, cand_masks,
                                  set_row_offset, cand_row_offset, false);
    if (rc) return rc;
    const uint64_t srows = set_row_offset[n_sets], crows = cand_row_offset[set_cand_offset[n_sets]];
    if (srows) HIP_TRY(hipMemcpyAsync(set_counts, cb.base.set_table, (size_t)srows * 80, hipMemcpyDeviceToHost, c->stream));
    if (crows) HIP_TRY(hipMemcpyAsync(cand_counts, cb.base.cand_table, (size_t)crows * 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t s = 0; s < n_sets; ++s) {                               // unexplained records = mod_total - mod_explained, both strands
        uint64_t n = 0;
        for (uint64_t r = set_row_offset[s]; r < set_row_offset[s + 1]; ++r)
            n += (uint64_t)(set_counts[r * 10 + 0] - set_counts[r * 10 + 1] + set_counts[r * 10 + 5] - set_counts[r * 10 + 6]);
        set_total[s] = n;
    }
    return NM_OK;
}

int nm_motif_coverage_sites(nm_ctx *c, uint32_t n_sets, const uint32_t *set_bin, const uint8_t *set_mod_slot, const uint32_t *set_cand_offset,
                            const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                            uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                            uint64_t *set_offset, uint64_t *n_written) {
    if (!set_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code))) return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (n_sets == 0) {
        set_offset[0] = 0;
        return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    }
    CovBatch cb;
    const int rc = coverage_begin(cb, c, n_sets, set_bin, set_mod_slot, set_cand_offset, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr, nullptr, true);
    if (rc) return rc;
    return export_window(cb, coverage_kernels<true>, n_sets, first_record, capacity, site_contig, site_pos, site_code, set_offset, n_written);
}
