// Two-sample comparison: every occurrence of every candidate of a batch, classified by its state in TWO resident mod slots (the
// same assembly sequenced twice: slot A, slot B).  The reference has no counterpart; the nearest is two runs of
// motif_model_contig(..., save_motif_positions=True) (find_motifs_bin.py:1285-1331) joined on the host.  An occurrence and its
// state in a slot are nm_motif_sites' (nmsites.hip); transition t = 3 * state_a + state_b.  Same shape as that unit:
//   count  one wave per (candidate, chunk of its bin): the chunk's sequence planes are loaded ONCE and the constraint program is
//          walked ONCE per strand for both samples — only the eight state planes differ; nine disjoint classes per strand go into
//          the (candidate, contig) table, the number of records under transition_set into the work item's slot
//   scan   one device-wide exclusive prefix (rocPRIM) over the work items, numbered in output order
//   fill   the masks are computed again and every selected occurrence writes its record at its rank; work items whose ranks miss the
//          caller's window are skipped before anything is loaded
// One launch per reach width G = 1, 2, 3 and pass: at most 3 + 1 + 1 + 3 launches whatever the batch holds.
#include <rocprim/device/device_scan.hpp>

#include "nmscan_device.h"

using namespace nmdetail;

namespace {

struct CompareArgs {
    Planes seq;
    const uint32_t *cls_cand;            // candidates of this width, in batch order
    const uint32_t *cls_item0;           // [n_cls + 1] prefix of their chunk counts
    uint32_t n_cls, n_items;
    const uint32_t *cand_item0;          // [n_cand + 1] first work item of a candidate in the batch-wide numbering
    const uint32_t *cand_chunk0;         // first chunk of the candidate's bin
    const uint32_t *cand_row0;           // first row of the candidate in the (candidate, contig) table
    const unsigned long long *cand_planes;   // [n_cand][8] MP UP MM UM of slot A, then of slot B
    const uint32_t *programs;            // [n_cand][PROG6_DW] sliced to the candidate's width
    const uint32_t *chunk_contig, *chunk_rank, *contig_chunk;
    uint32_t transition_set;             // bit t = transition t is exported
    unsigned long long *item_cnt;        // count pass: records per work item
    unsigned long long *table;           // count pass: [row][18], may be NULL
    const unsigned long long *item_off;  // fill pass: exclusive prefix of item_cnt (+ total)
    unsigned long long first, capacity;  // fill pass: the window of ranks that is written
    uint32_t *out_contig, *out_pos;
    uint8_t *out_code;
};

// the three disjoint states of one strand's word in one slot (a position called both ways is methylated)
struct States {
    uint32_t s[3];
    __device__ __forceinline__ States(uint32_t m, uint32_t u) : s{m, u & ~m, ~(m | u)} {}
};

// the occurrences of `acc` whose transition is in `set`
__device__ __forceinline__ uint32_t pick9(uint32_t set, uint32_t acc, const States &a, const States &b) {
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        uint32_t bsel = 0;                                                // states of B selected together with state i of A
#pragma unroll
        for (int j = 0; j < 3; ++j) bsel |= (set >> (3 * i + j) & 1u) ? b.s[j] : 0u;
        out |= a.s[i] & bsel;
    }
    return out & acc;
}

__device__ __forceinline__ uint32_t transition_of(uint32_t bit, const States &a, const States &b) {
    const uint32_t sa = (a.s[0] & bit) ? 0u : (a.s[1] & bit) ? 1u : 2u, sb = (b.s[0] & bit) ? 0u : (b.s[1] & bit) ? 1u : 2u;
    return 3u * sa + sb;
}

template <int G, bool FILL>
__global__ __launch_bounds__(256) void compare_kernel(CompareArgs a) {
    using K = Variant<G, G, false, 2, false, false>;
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
    const unsigned long long *pl = a.cand_planes + (size_t)k * 8;
    StatePlanes stp[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        stp[s].M = nullptr;
        stp[s].U = nullptr;
        stp[s].MP = reinterpret_cast<const uint32_t *>(pl[4 * s + 0]);
        stp[s].UP = reinterpret_cast<const uint32_t *>(pl[4 * s + 1]);
        stp[s].MM = reinterpret_cast<const uint32_t *>(pl[4 * s + 2]);
        stp[s].UM = reinterpret_cast<const uint32_t *>(pl[4 * s + 3]);
    }
    RawChunk<K> raw;
    raw.load(a.seq, stp, chunk, lane);                                   // sequence planes once, the state planes of both slots
    Tile<K> tile;
    tile.expand(raw);
    uint32_t af[T_WORDS], ar[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) af[t] = ar[t] = 0xFFFFFFFFu;
    const cu32p prog = (cu32p)(a.programs + (size_t)k * PROG6_DW);
    eval_strand<K>(prog, tile, af);                                      // one walk per strand serves both samples
    eval_strand<K>(prog + K::PDW, tile, ar);
    const uint32_t set = a.transition_set;
    if (!FILL) {
        uint32_t c[18], n = 0;
#pragma unroll
        for (int j = 0; j < 18; ++j) c[j] = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            const States fa(raw.s[0][0][t], raw.s[0][1][t]), fb(raw.s[1][0][t], raw.s[1][1][t]);
            const States ra(raw.s[0][2][t], raw.s[0][3][t]), rb(raw.s[1][2][t], raw.s[1][3][t]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint32_t fi = af[t] & fa.s[i], ri = ar[t] & ra.s[i];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    c[3 * i + j] += __popc(fi & fb.s[j]);
                    c[9 + 3 * i + j] += __popc(ri & rb.s[j]);
                }
            }
            n += __popc(pick9(set, af[t], fa, fb)) + __popc(pick9(set, ar[t], ra, rb));
        }
        for (int o = 32; o; o >>= 1) {
            n += __shfl_xor(n, o);
#pragma unroll
            for (int j = 0; j < 18; ++j) c[j] += __shfl_xor(c[j], o);
        }
        if (lane == 0) {
            a.item_cnt[item] = n;
            if (a.table) {
                unsigned long long *row = a.table + ((size_t)((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[chunk]) * 18;
#pragma unroll
                for (int j = 0; j < 18; ++j)
                    if (c[j]) atomicAdd(row + j, (unsigned long long)c[j]);
            }
        }
        return;
    }
    // ---- fill: rank of the lane's first record = prefix of the item + records of the lanes before it
    uint32_t mine = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        const States fa(raw.s[0][0][t], raw.s[0][1][t]), fb(raw.s[1][0][t], raw.s[1][1][t]);
        const States ra(raw.s[0][2][t], raw.s[0][3][t]), rb(raw.s[1][2][t], raw.s[1][3][t]);
        mine += __popc(pick9(set, af[t], fa, fb)) + __popc(pick9(set, ar[t], ra, rb));
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
        const States fa(raw.s[0][0][t], raw.s[0][1][t]), fb(raw.s[1][0][t], raw.s[1][1][t]);
        const States ra(raw.s[0][2][t], raw.s[0][3][t]), rb(raw.s[1][2][t], raw.s[1][3][t]);
        const uint32_t f = pick9(set, af[t], fa, fb), r = pick9(set, ar[t], ra, rb);
        uint32_t both = f | r;
        while (both) {                                                  // ascending position, '+' before '-'
            const uint32_t b = __builtin_ctz(both), bit = 1u << b;
            both &= both - 1;
            const uint32_t pos = pos0 + t * 32 + b;
            if (f & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos;
                    a.out_code[at] = (uint8_t)transition_of(bit, fa, fb);
                }
                ++at;
            }
            if (r & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos;
                    a.out_code[at] = (uint8_t)(NM_COMPARE_MINUS | transition_of(bit, ra, rb));
                }
                ++at;
            }
        }
    }
}

// cand_offset[k] = rank of candidate k's first record (k = n_cand: the batch's total)
__global__ void compare_gather_kernel(const unsigned long long *__restrict__ item_off, const uint32_t *__restrict__ cand_item0, uint32_t n,
                                      unsigned long long *__restrict__ cand_offset) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) cand_offset[k] = item_off[cand_item0[k]];
}

template <bool FILL>
void launch_width(int g, const CompareArgs &a, hipStream_t st) {
    const dim3 grid((a.n_items + 3) / 4), block(256);
    if (g == 2) hipLaunchKernelGGL((compare_kernel<3, FILL>), grid, block, 0, st, a);
    else if (g == 1) hipLaunchKernelGGL((compare_kernel<2, FILL>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((compare_kernel<1, FILL>), grid, block, 0, st, a);
}

// Everything a batch needs on the device, in one block: the staged tables, the programs, the item table(s), the count table.
struct CompareBatch {
    nm_ctx *c = nullptr;
    uint8_t *d = nullptr;
    CompareArgs base{};
    uint32_t cls_n[3] = {0, 0, 0}, cls_items[3] = {0, 0, 0};
    const uint32_t *cls_cand[3] = {}, *cls_item0[3] = {};
    unsigned long long *d_cand_offset = nullptr;
    void *d_scan = nullptr;
    size_t scan_bytes = 0;
    ~CompareBatch() {
        if (!c) return;
        (void)hipStreamSynchronize(c->stream);                           // nothing may still read the block
        if (d) (void)dev_free(d);
    }
};

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// validate the batch, compile its programs, stage the tables and enqueue the count pass (and, with_scan, the prefix + gather)
int compare_begin(CompareBatch &cb, nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_slot_a, const uint8_t *cand_slot_b,
                  const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                  const uint64_t *row_offset, uint32_t transition_set, bool with_scan) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand && (!cand_bin || !cand_slot_a || !cand_slot_b || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks))
        return fail(NM_EINVAL, "NULL argument");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (transition_set == 0 || (transition_set & ~NM_COMPARE_ALL))
        return fail(NM_EINVAL, "transition_set %u: a non-empty combination of the bits 0..8 (bit 3 * state_a + state_b)", transition_set);
    std::vector<uint32_t> item0(n_cand + 1, 0), chunk0(n_cand, 0), row0(n_cand, 0), programs((size_t)n_cand * PROG6_DW, 0);
    std::vector<unsigned long long> planes((size_t)n_cand * 8, 0);
    std::vector<uint32_t> cls_cand[3], cls_item0[3];
    uint64_t items = 0, rows = 0;
    if (row_offset && row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
    for (uint32_t k = 0; k < n_cand; ++k) {
        const uint32_t bin = cand_bin[k];
        const uint32_t slots[2] = {cand_slot_a[k], cand_slot_b[k]};
        for (int s = 0; s < 2; ++s) {
            if (slots[s] >= NM_MAX_MOD_SLOTS || !c->slots[slots[s]].present || !c->slots[slots[s]].planes[2])
                return fail(NM_ESTATE, "candidate %u uses mod slot %u (sample %c) with no pileup uploaded", k, slots[s], s ? 'B' : 'A');
            for (int j = 0; j < 4; ++j) planes[(size_t)k * 8 + 4 * s + j] = (unsigned long long)(uintptr_t)c->slots[slots[s]].planes[2 + j];
        }
        if (bin >= c->n_bins) return fail(NM_EINVAL, "candidate %u: bin %u >= n_bins %u", k, bin, c->n_bins);
        uint32_t full[PROG6_DW];
        int reach = 0;
        const int rc = compile_program(cand_masks + cand_mask_offset[k], cand_len[k], cand_modpos[k], full, &reach);
        if (rc) return rc;
        slice_program(full, reach + 1, programs.data() + (size_t)k * PROG6_DW);
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
        cb.cls_n[g] = (uint32_t)cls_cand[g].size();
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
    const size_t o_item0 = take((size_t)(n_cand + 1) * 4), o_chunk0 = take((size_t)n_cand * 4), o_row0 = take((size_t)n_cand * 4);
    const size_t o_planes = take((size_t)n_cand * 64), o_prog = take((size_t)n_cand * PROG6_DW * 4);
    const size_t o_cc = take((size_t)c->n_chunks * 4), o_cr = take((size_t)c->n_chunks * 4);
    size_t o_cls_cand[3], o_cls_item0[3];
    for (int g = 0; g < 3; ++g) { o_cls_cand[g] = take(cls_cand[g].size() * 4 + 4); o_cls_item0[g] = take(cls_item0[g].size() * 4); }
    const size_t in_bytes = at;
    const size_t o_cnt = take((size_t)(items + 1) * 8), o_table = take((size_t)rows * 144 + 8);
    const size_t zero_bytes = at - o_cnt;
    const size_t o_off = take(with_scan ? (size_t)(items + 1) * 8 : 0), o_coff = take(with_scan ? (size_t)(n_cand + 1) * 8 : 0);
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
    put(o_row0, row0.data(), row0.size() * 4);
    put(o_planes, planes.data(), planes.size() * 8);
    put(o_prog, programs.data(), programs.size() * 4);
    put(o_cc, chunk_contig.data(), chunk_contig.size() * 4);
    put(o_cr, chunk_rank.data(), chunk_rank.size() * 4);
    for (int g = 0; g < 3; ++g) { put(o_cls_cand[g], cls_cand[g].data(), cls_cand[g].size() * 4); put(o_cls_item0[g], cls_item0[g].data(), cls_item0[g].size() * 4); }
    HIP_TRY(hipMemcpyAsync(cb.d, h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                              // (h is pageable memory of this frame)
    HIP_TRY(hipMemsetAsync(cb.d + o_cnt, 0, zero_bytes, c->stream));
    CompareArgs &a = cb.base;
    a.seq = seq_planes(c);
    a.cand_item0 = reinterpret_cast<const uint32_t *>(cb.d + o_item0);
    a.cand_chunk0 = reinterpret_cast<const uint32_t *>(cb.d + o_chunk0);
    a.cand_row0 = reinterpret_cast<const uint32_t *>(cb.d + o_row0);
    a.cand_planes = reinterpret_cast<const unsigned long long *>(cb.d + o_planes);
    a.programs = reinterpret_cast<const uint32_t *>(cb.d + o_prog);
    a.chunk_contig = reinterpret_cast<const uint32_t *>(cb.d + o_cc);
    a.chunk_rank = reinterpret_cast<const uint32_t *>(cb.d + o_cr);
    a.contig_chunk = c->d_contig_chunk;
    a.transition_set = transition_set;
    a.item_cnt = reinterpret_cast<unsigned long long *>(cb.d + o_cnt);
    a.table = row_offset ? reinterpret_cast<unsigned long long *>(cb.d + o_table) : nullptr;
    a.item_off = reinterpret_cast<const unsigned long long *>(cb.d + o_off);
    for (int g = 0; g < 3; ++g) {
        cb.cls_cand[g] = reinterpret_cast<const uint32_t *>(cb.d + o_cls_cand[g]);
        cb.cls_item0[g] = reinterpret_cast<const uint32_t *>(cb.d + o_cls_item0[g]);
    }
    cb.d_cand_offset = reinterpret_cast<unsigned long long *>(cb.d + o_coff);
    cb.d_scan = cb.d + o_scan;
    for (int g = 0; g < 3; ++g) {
        if (!cb.cls_items[g]) continue;
        CompareArgs ag = a;
        ag.cls_cand = cb.cls_cand[g];
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
        hipLaunchKernelGGL(compare_gather_kernel, dim3((n_cand + 256) / 256), dim3(256), 0, c->stream, a.item_off, a.cand_item0, n_cand + 1, cb.d_cand_offset);
        HIP_TRY(hipGetLastError());
        c->launches += 2;
    }
    return NM_OK;
}

}  // namespace

int nm_motif_compare_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_slot_a, const uint8_t *cand_slot_b,
                           const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                           uint32_t transition_set, const uint64_t *row_offset, uint64_t *cand_total, int64_t *contig_counts) {
    if (!row_offset || (n_cand && (!cand_total || !contig_counts))) return fail(NM_EINVAL, "NULL argument");
    if (n_cand == 0) return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    CompareBatch cb;
    const int rc = compare_begin(cb, c, n_cand, cand_bin, cand_slot_a, cand_slot_b, cand_len, cand_modpos, cand_mask_offset, cand_masks, row_offset,
                                 transition_set, false);
    if (rc) return rc;
    const uint64_t rows = row_offset[n_cand];
    if (rows) HIP_TRY(hipMemcpyAsync(contig_counts, cb.base.table, (size_t)rows * 144, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_cand; ++k) {                               // the totals are sums of the table's selected transitions
        uint64_t n = 0;
        for (uint64_t r = row_offset[k]; r < row_offset[k + 1]; ++r)
            for (int j = 0; j < 18; ++j)
                if (transition_set >> (j % 9) & 1u) n += (uint64_t)contig_counts[r * 18 + j];
        cand_total[k] = n;
    }
    return NM_OK;
}

int nm_motif_compare_sites(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_slot_a, const uint8_t *cand_slot_b,
                           const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                           uint32_t transition_set, uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos,
                           uint8_t *site_code, uint64_t *cand_offset, uint64_t *n_written) {
    if (!cand_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code))) return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (n_cand == 0) {
        cand_offset[0] = 0;
        return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    }
    CompareBatch cb;
    int rc = compare_begin(cb, c, n_cand, cand_bin, cand_slot_a, cand_slot_b, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr,
                           transition_set, true);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(cand_offset, cb.d_cand_offset, (size_t)(n_cand + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = cand_offset[n_cand];
    const uint64_t n = first_record >= total ? 0 : std::min<uint64_t>(capacity, total - first_record);
    if (n == 0) return NM_OK;
    uint8_t *d_out = nullptr;                                             // contig | pos | code of the window's records
    const size_t o_pos = align16((size_t)n * 4), o_code = o_pos + align16((size_t)n * 4);
    HIP_TRY(dev_malloc(&d_out, o_code + (size_t)n));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)dev_free(p); } } guard{d_out, c};
    CompareArgs a = cb.base;
    a.first = first_record;
    a.capacity = n;
    a.out_contig = reinterpret_cast<uint32_t *>(d_out);
    a.out_pos = reinterpret_cast<uint32_t *>(d_out + o_pos);
    a.out_code = d_out + o_code;
    for (int g = 0; g < 3; ++g) {
        if (!cb.cls_items[g]) continue;
        CompareArgs ag = a;
        ag.cls_cand = cb.cls_cand[g];
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
