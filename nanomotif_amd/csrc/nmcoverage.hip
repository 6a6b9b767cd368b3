// Coverage of a bin's methylation by a SET of motifs: what share of the confidently methylated positions of a (bin, mod type) lies
// on an occurrence of at least one motif of the set, which motifs are redundant, and where the unexplained positions are.  The
// reference has this only as a log line of find_best_candidates ("x % of sequences remaining", find_motifs_bin.py:801-823), taken
// before pruning and merging and never written to a file.  Coverage is DEFINED by nm_motif_sites (nmsites.hip): candidate j covers
// (contig, position, strand) iff that export, with all three states, writes a record for j there — same eval_strand over the same
// tile, so there is no second matcher.
//   count  one wave per (set, chunk of the set's bin): load the chunk and the slot's four state planes once, then walk the set's
//          candidates with wave-uniform control flow; per strand two accumulators, multi |= any & a; any |= a, so that
//          cover = any and once = any & ~multi.  Ten set counts per (set, contig) row; a second walk over the same candidates
//          (chunk still in registers, programs through the scalar cache again) gives a & once per candidate: four exclusive
//          counts per (candidate, contig) row.  The number of unexplained records M & ~cover of the work item goes to the item table.
//   scan   one device-wide exclusive prefix (rocPRIM) over the work items, numbered in (set, contig rank, chunk) order = output order
//   fill   cover is computed again and every unexplained position writes its record at its rank; work items whose ranks miss the
//          caller's window are skipped before anything is loaded
// A set runs at the width (word-groups G = 1, 2, 3 either side of the modified base) of its widest candidate, the programs of the
// narrower ones sliced to that width: at most 3 + 1 + 1 + 3 = 8 launches whatever the number of sets and candidates.
#include <rocprim/device/device_scan.hpp>

#include "nmscan_device.h"

using namespace nmdetail;

namespace {

struct CovArgs {
    Planes seq;
    const uint32_t *cls_set;             // sets of this width, in call order
    const uint32_t *cls_item0;           // [n_cls + 1] prefix of their chunk counts
    uint32_t n_cls, n_items;
    const uint32_t *set_item0;           // [n_sets + 1] first work item of a set in the call-wide numbering
    const uint32_t *set_chunk0;          // first chunk of the set's bin
    const uint32_t *set_row0;            // first row of the set in the (set, contig) table
    const uint32_t *set_cand0;           // [n_sets + 1] first candidate of a set
    const unsigned long long *set_planes;    // [n_sets][4] MP UP MM UM of the set's mod slot
    const uint32_t *cand_row0;           // first row of a candidate in the (candidate, contig) table
    const uint32_t *programs;            // [n_cand][PROG6_DW] sliced to the width of the candidate's SET
    const uint32_t *chunk_contig, *chunk_rank, *contig_chunk;
    unsigned long long *item_cnt;        // count pass: unexplained records per work item
    unsigned long long *set_table;       // count pass: [row][10]
    unsigned long long *cand_table;      // count pass: [row][4]
    const unsigned long long *item_off;  // fill pass: exclusive prefix of item_cnt (+ total)
    unsigned long long first, capacity;  // fill pass: the window of ranks that is written
    uint32_t *out_contig, *out_pos;
    uint8_t *out_code;
};

template <int G, bool FILL>
__global__ __launch_bounds__(256) void coverage_kernel(CovArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t it = blockIdx.x * 4 + wave;                          // wave-uniform from here on
    if (it >= a.n_items) return;
    const cu32p item0 = (cu32p)a.cls_item0;
    uint32_t lo = 0, hi = a.n_cls;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (item0[mid] <= it) lo = mid; else hi = mid;
    }
    const uint32_t s = ((cu32p)a.cls_set)[lo], ck = it - item0[lo];
    const uint32_t item = ((cu32p)a.set_item0)[s] + ck, chunk = ((cu32p)a.set_chunk0)[s] + ck;
    unsigned long long off0 = 0;
    if (FILL) {
        off0 = a.item_off[item];
        const unsigned long long off1 = a.item_off[item + 1];
        if (off1 == off0 || off1 <= a.first || off0 >= a.first + a.capacity) return;   // no rank of this item is in the window
    }
    const unsigned long long *pl = a.set_planes + (size_t)s * 4;
    StatePlanes stp[1];
    stp[0].M = nullptr;
    stp[0].U = nullptr;
    stp[0].MP = reinterpret_cast<const uint32_t *>(pl[0]);
    stp[0].UP = reinterpret_cast<const uint32_t *>(pl[1]);
    stp[0].MM = reinterpret_cast<const uint32_t *>(pl[2]);
    stp[0].UM = reinterpret_cast<const uint32_t *>(pl[3]);
    RawChunk<K> raw;
    raw.load(a.seq, stp, chunk, lane);
    Tile<K> tile;
    tile.expand(raw);
    const uint32_t c0 = ((cu32p)a.set_cand0)[s], c1 = ((cu32p)a.set_cand0)[s + 1];
    uint32_t anyf[T_WORDS], anyr[T_WORDS], multif[T_WORDS], multir[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) anyf[t] = anyr[t] = multif[t] = multir[t] = 0u;
    for (uint32_t k = c0; k < c1; ++k) {                                // wave-uniform
        uint32_t af[T_WORDS], ar[T_WORDS];
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
        const uint32_t rank = ((cu32p)a.chunk_rank)[chunk];
        if (lane == 0) {
            a.item_cnt[item] = n;
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
    // ---- fill: rank of the lane's first record = prefix of the item + records of the lanes before it
    uint32_t mine = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) mine += __popc(raw.s[0][0][t] & ~anyf[t]) + __popc(raw.s[0][2][t] & ~anyr[t]);
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    // (ranks are taken relative to the window: one unsigned comparison covers both of its ends)
    unsigned long long at = off0 + (incl - mine) - a.first;
    const uint32_t contig = ((cu32p)a.chunk_contig)[chunk];
    const uint32_t pos0 = (chunk - ((cu32p)a.contig_chunk)[contig]) * (uint32_t)CHUNK_BP + (uint32_t)lane * (T_WORDS * 32);
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        const uint32_t f = raw.s[0][0][t] & ~anyf[t], r = raw.s[0][2][t] & ~anyr[t];
        uint32_t both = f | r;
        while (both) {                                                  // ascending position, '+' before '-'
            const uint32_t b = __builtin_ctz(both), bit = 1u << b;
            both &= both - 1;
            const uint32_t pos = pos0 + t * 32 + b;
            if (f & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos;
                    a.out_code[at] = 0;
                }
                ++at;
            }
            if (r & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos;
                    a.out_code[at] = (uint8_t)NM_SITES_MINUS;
                }
                ++at;
            }
        }
    }
}

// set_offset[s] = rank of set s's first record (s = n_sets: the call's total)
__global__ void coverage_gather_kernel(const unsigned long long *__restrict__ item_off, const uint32_t *__restrict__ set_item0, uint32_t n,
                                       unsigned long long *__restrict__ set_offset) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) set_offset[s] = item_off[set_item0[s]];
}

template <bool FILL>
void launch_width(int g, const CovArgs &a, hipStream_t st) {
    const dim3 grid((a.n_items + 3) / 4), block(256);
    if (g == 2) hipLaunchKernelGGL((coverage_kernel<3, FILL>), grid, block, 0, st, a);
    else if (g == 1) hipLaunchKernelGGL((coverage_kernel<2, FILL>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((coverage_kernel<1, FILL>), grid, block, 0, st, a);
}

// Everything a call needs on the device, in one block: the staged tables, the programs, the item table(s), the two count tables.
struct CovBatch {
    nm_ctx *c = nullptr;
    uint8_t *d = nullptr;
    CovArgs base{};
    uint32_t cls_n[3] = {0, 0, 0}, cls_items[3] = {0, 0, 0};
    const uint32_t *cls_set[3] = {}, *cls_item0[3] = {};
    unsigned long long *d_set_offset = nullptr;
    void *d_scan = nullptr;
    size_t scan_bytes = 0;
    ~CovBatch() {
        if (!c) return;
        (void)hipStreamSynchronize(c->stream);                           // nothing may still read the block
        if (d) (void)dev_free(d);
    }
};

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

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
    std::vector<uint32_t> item0(n_sets + 1, 0), chunk0(n_sets, 0), srow0(n_sets, 0), crow0(n_cand, 0), programs((size_t)n_cand * PROG6_DW, 0);
    std::vector<unsigned long long> planes((size_t)n_sets * 4, 0);
    std::vector<uint32_t> cls_set[3], cls_item0[3];
    uint64_t items = 0, srows = 0, crows = 0;
    for (uint32_t s = 0; s < n_sets; ++s) {
        const uint32_t slot = set_mod_slot[s], bin = set_bin[s];
        if (slot >= NM_MAX_MOD_SLOTS || !c->slots[slot].present || !c->slots[slot].planes[2])
            return fail(NM_ESTATE, "set %u uses mod slot %u with no pileup uploaded", s, slot);
        if (bin >= c->n_bins) return fail(NM_EINVAL, "set %u: bin %u >= n_bins %u", s, bin, c->n_bins);
        const uint32_t ncontigs = c->bin_ncontigs[bin];
        // the set's width = the reach class of its widest candidate; every program of the set is sliced to it
        uint32_t full[PROG6_DW];
        int width = 0;
        for (uint32_t k = set_cand_offset[s]; k < set_cand_offset[s + 1]; ++k) {
            int reach = 0;
            const int rc = compile_program(cand_masks + cand_mask_offset[k], cand_len[k], cand_modpos[k], full, &reach);
            if (rc) return rc;
            width = std::max(width, reach);
        }
        for (uint32_t k = set_cand_offset[s]; k < set_cand_offset[s + 1]; ++k) {
            int reach = 0;
            (void)compile_program(cand_masks + cand_mask_offset[k], cand_len[k], cand_modpos[k], full, &reach);
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
        for (int j = 0; j < 4; ++j) planes[(size_t)s * 4 + j] = (unsigned long long)(uintptr_t)c->slots[slot].planes[2 + j];
        item0[s] = (uint32_t)items;
        chunk0[s] = c->bin_chunk0[bin];
        const uint32_t nch = c->bin_nchunks[bin];
        if (nch) {
            cls_set[width].push_back(s);
            cls_item0[width].push_back(0);                                // (filled in below)
        }
        items += nch;
        if (items >= 0xFFFFFFF0ull) return fail(NM_ERANGE, "more than 2^32 (set, chunk) work items in one call: send fewer sets");
    }
    item0[n_sets] = (uint32_t)items;
    for (int g = 0; g < 3; ++g) {                                         // class-local prefixes of the chunk counts
        uint32_t run = 0;
        for (size_t j = 0; j < cls_set[g].size(); ++j) {
            cls_item0[g][j] = run;
            run += c->bin_nchunks[set_bin[cls_set[g][j]]];
        }
        cls_item0[g].push_back(run);
        cb.cls_n[g] = (uint32_t)cls_set[g].size();
        cb.cls_items[g] = run;
    }
    // per chunk: its contig and the contig's rank in its bin (pad chunks: never touched, no work item covers them)
    std::vector<uint32_t> chunk_contig(c->n_chunks, 0), chunk_rank(c->n_chunks, 0);
    for (uint32_t i = 0; i < c->n_contigs; ++i)
        for (uint32_t q = 0; q < c->contig_nchunks[i]; ++q) {
            chunk_contig[c->contig_chunk[i] + q] = i;
            chunk_rank[c->contig_chunk[i] + q] = c->contig_rank[i];
        }
    HIP_TRY(hipSetDevice(c->device));
    // ---- one device block
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align16(at + bytes); return o; };
    const size_t o_item0 = take((size_t)(n_sets + 1) * 4), o_chunk0 = take((size_t)n_sets * 4), o_srow0 = take((size_t)n_sets * 4);
    const size_t o_cand0 = take((size_t)(n_sets + 1) * 4), o_crow0 = take((size_t)n_cand * 4);
    const size_t o_planes = take((size_t)n_sets * 32), o_prog = take((size_t)n_cand * PROG6_DW * 4);
    const size_t o_cc = take((size_t)c->n_chunks * 4), o_cr = take((size_t)c->n_chunks * 4);
    size_t o_cls_set[3], o_cls_item0[3];
    for (int g = 0; g < 3; ++g) { o_cls_set[g] = take(cls_set[g].size() * 4 + 4); o_cls_item0[g] = take(cls_item0[g].size() * 4); }
    const size_t in_bytes = at;
    const size_t o_cnt = take((size_t)(items + 1) * 8), o_stable = take((size_t)srows * 80 + 8), o_ctable = take((size_t)crows * 32 + 8);
    const size_t zero_bytes = at - o_cnt;
    const size_t o_off = take(with_scan ? (size_t)(items + 1) * 8 : 0), o_soff = take(with_scan ? (size_t)(n_sets + 1) * 8 : 0);
    if (with_scan)
        HIP_TRY(rocprim::exclusive_scan(nullptr, cb.scan_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)items + 1,
                                        rocprim::plus<unsigned long long>(), c->stream));
    const size_t o_scan = take(cb.scan_bytes);
    cb.c = c;
    HIP_TRY(dev_malloc(&cb.d, at));
    std::vector<uint8_t> h(in_bytes, 0);
    auto put = [&](size_t o, const void *src, size_t bytes) { if (bytes) memcpy(h.data() + o, src, bytes); };
    put(o_item0, item0.data(), item0.size() * 4);
    put(o_chunk0, chunk0.data(), chunk0.size() * 4);
    put(o_srow0, srow0.data(), srow0.size() * 4);
    put(o_cand0, set_cand_offset, (size_t)(n_sets + 1) * 4);
    put(o_crow0, crow0.data(), crow0.size() * 4);
    put(o_planes, planes.data(), planes.size() * 8);
    put(o_prog, programs.data(), programs.size() * 4);
    put(o_cc, chunk_contig.data(), chunk_contig.size() * 4);
    put(o_cr, chunk_rank.data(), chunk_rank.size() * 4);
    for (int g = 0; g < 3; ++g) { put(o_cls_set[g], cls_set[g].data(), cls_set[g].size() * 4); put(o_cls_item0[g], cls_item0[g].data(), cls_item0[g].size() * 4); }
    HIP_TRY(hipMemcpyAsync(cb.d, h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                              // (h is pageable memory of this frame)
    HIP_TRY(hipMemsetAsync(cb.d + o_cnt, 0, zero_bytes, c->stream));
    CovArgs &a = cb.base;
    a.seq = seq_planes(c);
    a.set_item0 = reinterpret_cast<const uint32_t *>(cb.d + o_item0);
    a.set_chunk0 = reinterpret_cast<const uint32_t *>(cb.d + o_chunk0);
    a.set_row0 = reinterpret_cast<const uint32_t *>(cb.d + o_srow0);
    a.set_cand0 = reinterpret_cast<const uint32_t *>(cb.d + o_cand0);
    a.cand_row0 = reinterpret_cast<const uint32_t *>(cb.d + o_crow0);
    a.set_planes = reinterpret_cast<const unsigned long long *>(cb.d + o_planes);
    a.programs = reinterpret_cast<const uint32_t *>(cb.d + o_prog);
    a.chunk_contig = reinterpret_cast<const uint32_t *>(cb.d + o_cc);
    a.chunk_rank = reinterpret_cast<const uint32_t *>(cb.d + o_cr);
    a.contig_chunk = c->d_contig_chunk;
    a.item_cnt = reinterpret_cast<unsigned long long *>(cb.d + o_cnt);
    a.set_table = reinterpret_cast<unsigned long long *>(cb.d + o_stable);
    a.cand_table = reinterpret_cast<unsigned long long *>(cb.d + o_ctable);
    a.item_off = reinterpret_cast<const unsigned long long *>(cb.d + o_off);
    for (int g = 0; g < 3; ++g) {
        cb.cls_set[g] = reinterpret_cast<const uint32_t *>(cb.d + o_cls_set[g]);
        cb.cls_item0[g] = reinterpret_cast<const uint32_t *>(cb.d + o_cls_item0[g]);
    }
    cb.d_set_offset = reinterpret_cast<unsigned long long *>(cb.d + o_soff);
    cb.d_scan = cb.d + o_scan;
    for (int g = 0; g < 3; ++g) {
        if (!cb.cls_items[g]) continue;
        CovArgs ag = a;
        ag.cls_set = cb.cls_set[g];
        ag.cls_item0 = cb.cls_item0[g];
        ag.n_cls = cb.cls_n[g];
        ag.n_items = cb.cls_items[g];
        launch_width<false>(g, ag, c->stream);
        HIP_TRY(hipGetLastError());
        c->launches += 1;
    }
    if (with_scan) {
        HIP_TRY(rocprim::exclusive_scan(cb.d_scan, cb.scan_bytes, a.item_cnt, const_cast<unsigned long long *>(a.item_off), 0ull, (size_t)items + 1,
                                        rocprim::plus<unsigned long long>(), c->stream));
        hipLaunchKernelGGL(coverage_gather_kernel, dim3((n_sets + 256) / 256), dim3(256), 0, c->stream, a.item_off, a.set_item0, n_sets + 1, cb.d_set_offset);
        HIP_TRY(hipGetLastError());
        c->launches += 2;
    }
    return NM_OK;
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
    int rc = coverage_begin(cb, c, n_sets, set_bin, set_mod_slot, set_cand_offset, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr, nullptr, true);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(set_offset, cb.d_set_offset, (size_t)(n_sets + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = set_offset[n_sets];
    const uint64_t n = first_record >= total ? 0 : std::min<uint64_t>(capacity, total - first_record);
    if (n == 0) return NM_OK;
    uint8_t *d_out = nullptr;                                             // contig | pos | code of the window's records
    const size_t o_pos = align16((size_t)n * 4), o_code = o_pos + align16((size_t)n * 4);
    HIP_TRY(dev_malloc(&d_out, o_code + (size_t)n));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)dev_free(p); } } guard{d_out, c};
    CovArgs a = cb.base;
    a.first = first_record;
    a.capacity = n;
    a.out_contig = reinterpret_cast<uint32_t *>(d_out);
    a.out_pos = reinterpret_cast<uint32_t *>(d_out + o_pos);
    a.out_code = d_out + o_code;
    for (int g = 0; g < 3; ++g) {
        if (!cb.cls_items[g]) continue;
        CovArgs ag = a;
        ag.cls_set = cb.cls_set[g];
        ag.cls_item0 = cb.cls_item0[g];
        ag.n_cls = cb.cls_n[g];
        ag.n_items = cb.cls_items[g];
        launch_width<true>(g, ag, c->stream);
        HIP_TRY(hipGetLastError());
        c->launches += 1;
    }
    HIP_TRY(hipMemcpyAsync(site_contig, a.out_contig, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_pos, a.out_pos, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_code, a.out_code, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_written = n;
    return NM_OK;
}
