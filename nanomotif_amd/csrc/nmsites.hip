// Batched per-site export: WHERE every candidate of a batch occurs on the contigs of its bin, and in which state
// (methylated / unmethylated / no call) each occurrence is.  The building block in the reference is
// motif_model_contig(..., save_motif_positions=True) (find_motifs_bin.py:1285-1331: index_meth_fwd / index_nonmeth_fwd /
// index_meth_rev / index_nonmeth_rev, found by utils.py:44-67 subseq_indices); nm_hit_positions serves one (motif, contig,
// array) per call, this unit a whole batch of candidates x every contig of their bins x both strands in a fixed number of
// launches:
//   count  one wave per (candidate, chunk of its bin): load the chunk once, evaluate both strands, count the three
//          disjoint classes acc & M, acc & U, acc & ~(M | U) per strand; the number of records the work item will write
//          goes to its slot of the item table, the six class counts into the (candidate, contig) table
//   scan   one device-wide exclusive prefix (rocPRIM) over the work items, which are numbered in (candidate, contig rank,
//          chunk) order: that IS the order of the output, so nothing is sorted
//   fill   the masks are computed again (n_cand x assembly bits are not kept) and every site writes its record at its rank;
//          work items whose ranks miss the caller's window of records are skipped before anything is loaded
// Candidates of different reach (word-groups GN = 1, 2, 3 either side of the modified base) run in one launch per width
// and pass: at most 3 + 1 + 1 + 3 launches whatever the batch holds.
#include <rocprim/device/device_scan.hpp>

#include "nmscan_device.h"

using namespace nmdetail;

namespace {

struct SitesArgs {
    Planes seq;
    const uint32_t *cls_cand;            // candidates of this width, in batch order
    const uint32_t *cls_item0;           // [n_cls + 1] prefix of their chunk counts
    uint32_t n_cls, n_items;
    const uint32_t *cand_item0;          // [n_cand + 1] first work item of a candidate in the batch-wide numbering
    const uint32_t *cand_chunk0;         // first chunk of the candidate's bin
    const uint32_t *cand_row0;           // first row of the candidate in the (candidate, contig) table
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    const uint32_t *programs;            // [n_cand][PROG6_DW] sliced to the candidate's width
    const uint32_t *chunk_contig, *chunk_rank, *contig_chunk;
    uint32_t state_set;                  // NM_SITES_MOD | NM_SITES_NOMOD | NM_SITES_NOCALL
    unsigned long long *item_cnt;        // count pass: records per work item
    unsigned long long *table;           // count pass: [row][6], may be NULL
    const unsigned long long *item_off;  // fill pass: exclusive prefix of item_cnt (+ total)
    unsigned long long first, capacity;  // fill pass: the window of ranks that is written
    uint32_t *out_contig, *out_pos;
    uint8_t *out_code;
};

__device__ __forceinline__ uint32_t pick(uint32_t set, uint32_t m, uint32_t u, uint32_t n) {
    return ((set & 1u) ? m : 0u) | ((set & 2u) ? u : 0u) | ((set & 4u) ? n : 0u);
}

template <int G, bool FILL>
__global__ __launch_bounds__(256) void sites_kernel(SitesArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t it = blockIdx.x * 4 + wave;                          // wave-uniform from here on
    if (it >= a.n_items) return;
    // the candidate this work item belongs to: last entry of the prefix that is <= it (scalar loads, scalar control flow)
    const cu32p item0 = (cu32p)a.cls_item0;
    uint32_t lo = 0, hi = a.n_cls;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (item0[mid] <= it) lo = mid; else hi = mid;
    }
    const uint32_t k = ((cu32p)a.cls_cand)[lo], ck = it - item0[lo];
    const uint32_t item = ((cu32p)a.cand_item0)[k] + ck, chunk = ((cu32p)a.cand_chunk0)[k] + ck;
    unsigned long long off0 = 0;
    if (FILL) {
        off0 = a.item_off[item];
        const unsigned long long off1 = a.item_off[item + 1];
        if (off1 == off0 || off1 <= a.first || off0 >= a.first + a.capacity) return;   // no rank of this item is in the window
    }
    const unsigned long long *pl = a.cand_planes + (size_t)k * 4;
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
    uint32_t af[T_WORDS], ar[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) af[t] = ar[t] = 0xFFFFFFFFu;
    const cu32p prog = (cu32p)(a.programs + (size_t)k * PROG6_DW);
    eval_strand<K>(prog, tile, af);
    eval_strand<K>(prog + K::PDW, tile, ar);
    const uint32_t set = a.state_set;
    if (!FILL) {
        uint32_t c[6] = {0, 0, 0, 0, 0, 0}, n = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            const uint32_t mp = raw.s[0][0][t], up = raw.s[0][1][t] & ~mp, mm = raw.s[0][2][t], um = raw.s[0][3][t] & ~mm;
            const uint32_t fm = af[t] & mp, fu = af[t] & up, fn = af[t] & ~(mp | up);
            const uint32_t rm = ar[t] & mm, ru = ar[t] & um, rn = ar[t] & ~(mm | um);
            c[0] += __popc(fm); c[1] += __popc(fu); c[2] += __popc(fn);
            c[3] += __popc(rm); c[4] += __popc(ru); c[5] += __popc(rn);
            n += __popc(pick(set, fm, fu, fn)) + __popc(pick(set, rm, ru, rn));
        }
        for (int o = 32; o; o >>= 1) {
            n += __shfl_xor(n, o);
#pragma unroll
            for (int j = 0; j < 6; ++j) c[j] += __shfl_xor(c[j], o);
        }
        if (lane == 0) {
            a.item_cnt[item] = n;
            if (a.table) {
                unsigned long long *row = a.table + ((size_t)((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[chunk]) * 6;
#pragma unroll
                for (int j = 0; j < 6; ++j)
                    if (c[j]) atomicAdd(row + j, (unsigned long long)c[j]);
            }
        }
        return;
    }
    // ---- fill: rank of the lane's first record = prefix of the item + records of the lanes before it
    uint32_t mine = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        const uint32_t mp = raw.s[0][0][t], up = raw.s[0][1][t] & ~mp, mm = raw.s[0][2][t], um = raw.s[0][3][t] & ~mm;
        mine += __popc(pick(set, af[t] & mp, af[t] & up, af[t] & ~(mp | up))) + __popc(pick(set, ar[t] & mm, ar[t] & um, ar[t] & ~(mm | um)));
    }
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
        const uint32_t mp = raw.s[0][0][t], up = raw.s[0][1][t] & ~mp, mm = raw.s[0][2][t], um = raw.s[0][3][t] & ~mm;
        const uint32_t f = pick(set, af[t] & mp, af[t] & up, af[t] & ~(mp | up));
        const uint32_t r = pick(set, ar[t] & mm, ar[t] & um, ar[t] & ~(mm | um));
        uint32_t both = f | r;
        while (both) {                                                  // ascending position, '+' before '-'
            const uint32_t b = __builtin_ctz(both), bit = 1u << b;
            both &= both - 1;
            const uint32_t pos = pos0 + t * 32 + b;
            if (f & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos;
                    a.out_code[at] = (uint8_t)((mp & bit) ? 0u : (up & bit) ? 1u : 2u);
                }
                ++at;
            }
            if (r & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos;
                    a.out_code[at] = (uint8_t)(NM_SITES_MINUS | ((mm & bit) ? 0u : (um & bit) ? 1u : 2u));
                }
                ++at;
            }
        }
    }
}

// cand_offset[k] = rank of candidate k's first record (k = n_cand: the batch's total)
__global__ void sites_gather_kernel(const unsigned long long *__restrict__ item_off, const uint32_t *__restrict__ cand_item0, uint32_t n,
                                    unsigned long long *__restrict__ cand_offset) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) cand_offset[k] = item_off[cand_item0[k]];
}

template <bool FILL>
void launch_width(int g, const SitesArgs &a, hipStream_t st) {
    const dim3 grid((a.n_items + 3) / 4), block(256);
    if (g == 2) hipLaunchKernelGGL((sites_kernel<3, FILL>), grid, block, 0, st, a);
    else if (g == 1) hipLaunchKernelGGL((sites_kernel<2, FILL>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((sites_kernel<1, FILL>), grid, block, 0, st, a);
}

// Everything a batch needs on the device, in one block: the staged tables, the programs, the item table(s), the count table.
struct SitesBatch {
    nm_ctx *c = nullptr;
    uint8_t *d = nullptr;
    SitesArgs base{};
    uint32_t cls_n[3] = {0, 0, 0}, cls_items[3] = {0, 0, 0};
    const uint32_t *cls_cand[3] = {}, *cls_item0[3] = {};
    unsigned long long *d_cand_offset = nullptr;
    void *d_scan = nullptr;
    size_t scan_bytes = 0;
    ~SitesBatch() {
        if (!c) return;
        (void)hipStreamSynchronize(c->stream);                           // nothing may still read the block
        if (d) (void)dev_free(d);
    }
};

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// validate the batch, compile its programs, stage the tables and enqueue the count pass (and, with_scan, the prefix + gather)
int sites_begin(SitesBatch &sb, nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, const uint64_t *row_offset,
                uint32_t state_set, bool with_scan) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks)) return fail(NM_EINVAL, "NULL argument");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (state_set == 0 || (state_set & ~7u)) return fail(NM_EINVAL, "state_set %u: a non-empty combination of NM_SITES_MOD / NOMOD / NOCALL", state_set);
    std::vector<uint32_t> item0(n_cand + 1, 0), chunk0(n_cand, 0), row0(n_cand, 0), programs((size_t)n_cand * PROG6_DW, 0);
    std::vector<unsigned long long> planes((size_t)n_cand * 4, 0);
    std::vector<uint32_t> cls_cand[3], cls_item0[3];
    uint64_t items = 0, rows = 0;
    for (uint32_t k = 0; k < n_cand; ++k) {
        const uint32_t slot = cand_mod_slot[k], bin = cand_bin[k];
        if (slot >= NM_MAX_MOD_SLOTS || !c->slots[slot].present || !c->slots[slot].planes[2])
            return fail(NM_ESTATE, "candidate %u uses mod slot %u with no pileup uploaded", k, slot);
        if (bin >= c->n_bins) return fail(NM_EINVAL, "candidate %u: bin %u >= n_bins %u", k, bin, c->n_bins);
        uint32_t full[PROG6_DW];
        int reach = 0;
        const int rc = compile_program(cand_masks + cand_mask_offset[k], cand_len[k], cand_modpos[k], full, &reach);
        if (rc) return rc;
        slice_program(full, reach + 1, programs.data() + (size_t)k * PROG6_DW);
        for (int j = 0; j < 4; ++j) planes[(size_t)k * 4 + j] = (unsigned long long)(uintptr_t)c->slots[slot].planes[2 + j];
        item0[k] = (uint32_t)items;
        chunk0[k] = c->bin_chunk0[bin];
        if (row_offset) {
            if (row_offset[k + 1] < row_offset[k] || row_offset[k + 1] - row_offset[k] < c->bin_ncontigs[bin])
                return fail(NM_EINVAL, "candidate %u: %llu rows for the %u resident contigs of bin %u", k,
                            (unsigned long long)(row_offset[k + 1] - row_offset[k]), c->bin_ncontigs[bin], bin);
            if (row_offset[k + 1] >= 0xFFFFFFFFull) return fail(NM_ERANGE, "more than 2^32 (candidate, contig) rows in one batch");
            row0[k] = (uint32_t)row_offset[k];
            rows = row_offset[k + 1];
        }
        const uint32_t nch = c->bin_nchunks[bin];
        if (nch) {
            cls_cand[reach].push_back(k);
            cls_item0[reach].push_back(0);                                // (filled in below)
        }
        items += nch;
        if (items >= 0xFFFFFFF0ull) return fail(NM_ERANGE, "more than 2^32 (candidate, chunk) work items in one batch: send fewer candidates");
    }
    item0[n_cand] = (uint32_t)items;
    for (int g = 0; g < 3; ++g) {                                         // class-local prefixes of the chunk counts
        uint32_t run = 0;
        for (size_t j = 0; j < cls_cand[g].size(); ++j) {
            cls_item0[g][j] = run;
            run += c->bin_nchunks[cand_bin[cls_cand[g][j]]];
        }
        cls_item0[g].push_back(run);
        sb.cls_n[g] = (uint32_t)cls_cand[g].size();
        sb.cls_items[g] = run;
    }
    if (row_offset && row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
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
    const size_t o_item0 = take((size_t)(n_cand + 1) * 4), o_chunk0 = take((size_t)n_cand * 4), o_row0 = take((size_t)n_cand * 4);
    const size_t o_planes = take((size_t)n_cand * 32), o_prog = take((size_t)n_cand * PROG6_DW * 4);
    const size_t o_cc = take((size_t)c->n_chunks * 4), o_cr = take((size_t)c->n_chunks * 4);
    size_t o_cls_cand[3], o_cls_item0[3];
    for (int g = 0; g < 3; ++g) { o_cls_cand[g] = take(cls_cand[g].size() * 4 + 4); o_cls_item0[g] = take(cls_item0[g].size() * 4); }
    const size_t in_bytes = at;
    const size_t o_cnt = take((size_t)(items + 1) * 8), o_table = take((size_t)rows * 48 + 8);
    const size_t zero_bytes = at - o_cnt;
    const size_t o_off = take(with_scan ? (size_t)(items + 1) * 8 : 0), o_coff = take(with_scan ? (size_t)(n_cand + 1) * 8 : 0);
    if (with_scan)
        HIP_TRY(rocprim::exclusive_scan(nullptr, sb.scan_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)items + 1,
                                        rocprim::plus<unsigned long long>(), c->stream));
    const size_t o_scan = take(sb.scan_bytes);
    sb.c = c;
    HIP_TRY(dev_malloc(&sb.d, at));
    std::vector<uint8_t> h(in_bytes, 0);
    auto put = [&](size_t o, const void *src, size_t bytes) { if (bytes) memcpy(h.data() + o, src, bytes); };
    put(o_item0, item0.data(), item0.size() * 4);
    put(o_chunk0, chunk0.data(), chunk0.size() * 4);
    put(o_row0, row0.data(), row0.size() * 4);
    put(o_planes, planes.data(), planes.size() * 8);
    put(o_prog, programs.data(), programs.size() * 4);
    put(o_cc, chunk_contig.data(), chunk_contig.size() * 4);
    put(o_cr, chunk_rank.data(), chunk_rank.size() * 4);
    for (int g = 0; g < 3; ++g) { put(o_cls_cand[g], cls_cand[g].data(), cls_cand[g].size() * 4); put(o_cls_item0[g], cls_item0[g].data(), cls_item0[g].size() * 4); }
    HIP_TRY(hipMemcpyAsync(sb.d, h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                              // (h is pageable memory of this frame)
    HIP_TRY(hipMemsetAsync(sb.d + o_cnt, 0, zero_bytes, c->stream));
    SitesArgs &a = sb.base;
    a.seq = seq_planes(c);
    a.cand_item0 = reinterpret_cast<const uint32_t *>(sb.d + o_item0);
    a.cand_chunk0 = reinterpret_cast<const uint32_t *>(sb.d + o_chunk0);
    a.cand_row0 = reinterpret_cast<const uint32_t *>(sb.d + o_row0);
    a.cand_planes = reinterpret_cast<const unsigned long long *>(sb.d + o_planes);
    a.programs = reinterpret_cast<const uint32_t *>(sb.d + o_prog);
    a.chunk_contig = reinterpret_cast<const uint32_t *>(sb.d + o_cc);
    a.chunk_rank = reinterpret_cast<const uint32_t *>(sb.d + o_cr);
    a.contig_chunk = c->d_contig_chunk;
    a.state_set = state_set;
    a.item_cnt = reinterpret_cast<unsigned long long *>(sb.d + o_cnt);
    a.table = row_offset ? reinterpret_cast<unsigned long long *>(sb.d + o_table) : nullptr;
    a.item_off = reinterpret_cast<const unsigned long long *>(sb.d + o_off);
    for (int g = 0; g < 3; ++g) {
        sb.cls_cand[g] = reinterpret_cast<const uint32_t *>(sb.d + o_cls_cand[g]);
        sb.cls_item0[g] = reinterpret_cast<const uint32_t *>(sb.d + o_cls_item0[g]);
    }
    sb.d_cand_offset = reinterpret_cast<unsigned long long *>(sb.d + o_coff);
    sb.d_scan = sb.d + o_scan;
    for (int g = 0; g < 3; ++g) {
        if (!sb.cls_items[g]) continue;
        SitesArgs ag = a;
        ag.cls_cand = sb.cls_cand[g];
        ag.cls_item0 = sb.cls_item0[g];
        ag.n_cls = sb.cls_n[g];
        ag.n_items = sb.cls_items[g];
        launch_width<false>(g, ag, c->stream);
        HIP_TRY(hipGetLastError());
        c->launches += 1;
    }
    if (with_scan) {
        HIP_TRY(rocprim::exclusive_scan(sb.d_scan, sb.scan_bytes, a.item_cnt, const_cast<unsigned long long *>(a.item_off), 0ull, (size_t)items + 1,
                                        rocprim::plus<unsigned long long>(), c->stream));
        hipLaunchKernelGGL(sites_gather_kernel, dim3((n_cand + 256) / 256), dim3(256), 0, c->stream, a.item_off, a.cand_item0, n_cand + 1, sb.d_cand_offset);
        HIP_TRY(hipGetLastError());
        c->launches += 2;
    }
    return NM_OK;
}

}  // namespace

int nm_motif_sites_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                         const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t state_set,
                         const uint64_t *row_offset, uint64_t *cand_total, int64_t *contig_counts) {
    if (!row_offset || (n_cand && (!cand_total || !contig_counts))) return fail(NM_EINVAL, "NULL argument");
    if (n_cand == 0) return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    SitesBatch sb;
    const int rc = sites_begin(sb, c, n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks, row_offset, state_set, false);
    if (rc) return rc;
    const uint64_t rows = row_offset[n_cand];
    if (rows) HIP_TRY(hipMemcpyAsync(contig_counts, sb.base.table, (size_t)rows * 48, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_cand; ++k) {                               // the totals are sums of the table's selected classes
        uint64_t n = 0;
        for (uint64_t r = row_offset[k]; r < row_offset[k + 1]; ++r)
            for (int j = 0; j < 6; ++j)
                if (state_set >> (j % 3) & 1u) n += (uint64_t)contig_counts[r * 6 + j];
        cand_total[k] = n;
    }
    return NM_OK;
}

int nm_motif_sites(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                   const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t state_set,
                   uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                   uint64_t *cand_offset, uint64_t *n_written) {
    if (!cand_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code))) return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (n_cand == 0) {
        cand_offset[0] = 0;
        return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    }
    SitesBatch sb;
    int rc = sites_begin(sb, c, n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr, state_set, true);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(cand_offset, sb.d_cand_offset, (size_t)(n_cand + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = cand_offset[n_cand];
    const uint64_t n = first_record >= total ? 0 : std::min<uint64_t>(capacity, total - first_record);
    if (n == 0) return NM_OK;
    uint8_t *d_out = nullptr;                                             // contig | pos | code of the window's records
    const size_t o_pos = align16((size_t)n * 4), o_code = o_pos + align16((size_t)n * 4);
    HIP_TRY(dev_malloc(&d_out, o_code + (size_t)n));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)dev_free(p); } } guard{d_out, c};
    SitesArgs a = sb.base;
    a.first = first_record;
    a.capacity = n;
    a.out_contig = reinterpret_cast<uint32_t *>(d_out);
    a.out_pos = reinterpret_cast<uint32_t *>(d_out + o_pos);
    a.out_code = d_out + o_code;
    for (int g = 0; g < 3; ++g) {
        if (!sb.cls_items[g]) continue;
        SitesArgs ag = a;
        ag.cls_cand = sb.cls_cand[g];
        ag.cls_item0 = sb.cls_item0[g];
        ag.n_cls = sb.cls_n[g];
        ag.n_items = sb.cls_items[g];
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
