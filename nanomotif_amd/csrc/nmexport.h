// The scaffold the fourteen export units share; included by them and by nothing else.  Each hands out one wave per work item = (owner,
// chunk of the owner's bin) — an owner is a candidate, in nmcoverage.hip a set of candidates — and runs up to three steps:
//   count  the unit's kernel writes the number of records of every work item into the item table (and its own count tables)
//   scan   one device-wide exclusive prefix (rocPRIM) over the work items, which are numbered in (owner, contig rank, chunk)
//          order: that IS the order of the output, so nothing is sorted; a gather picks every owner's first rank
//   fill   the unit's kernel computes its masks again and every record is written at its rank; work items whose ranks miss the
//          caller's window of records are skipped before anything is loaded
// Owners of different width (word-groups G = 1, 2, 3 either side of the modified base) run in one launch per width and pass: at
// most 3 + 1 + 1 + 3 launches whatever a call holds.
//   all three steps (records): nmsites.hip, nmcoverage.hip, nmcompare.hip, nmstrands.hip — export_begin(with_scan) + export_window;
//                              nmpileup.hip, nmshift.hip and nmregions.hip, whose records carry two / four gathered columns / one class byte more,
//                              with a window half and a fill loop of their own
//   the count step only (tables): nmprofile.hip, nmtracks.hip, nmfractions.hip, nmcontext.hip, nmgc.hip, nmoverlap.hip — export_begin alone
//   the fourteenth, nmruns.hip: export_begin without the scan, then a stitch of its own over the work items of every (candidate, contig)
//                              BEFORE the prefix — a run crosses work items, so an item's record count is final only after it —, the
//                              prefix + gather enqueued by the unit, and a window half with two columns more
// Two more pieces belong to every unit and are owned by none:
//   stage_candidates  the host loop over a call's candidates: programs, widths, the work-item count and, on request, the state-plane
//                     addresses of a per-candidate mod slot and the row prefix of a (candidate, contig) table.  Its refusals come in ONE
//                     order — bin, the unit's own check, program, rows, work items — so a candidate wrong in two ways is refused the
//                     same way by every entry point.  (nmcoverage.hip stages sets and uses compile_motif / slot_state_planes.)
//   find_occurrences  the kernel prologue: the chunk and the state words loaded, the tile expanded, one walk per strand into fresh
//                     accumulators (walk_strands).  A free function with reference out-parameters: as a struct with members it costs
//                     4 - 5 VGPRs and a wave per SIMD at G = 2.  compare, tracks and context call it, fractions walk_strands;
//                     sites_kernel, strands_kernel, coverage_kernel and profile_kernel keep the lines written out, because through
//                     the helper they allocated other registers or measured about 1 % slower (profiles/r19/export_prologue.md).
// What a unit keeps is what differs: its own arguments and checks, how a work item's occurrences are classified and reduced, which
// of them become records, and the records' codes.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "nmscan_device.h"

namespace nmdetail {

// The kernel arguments every unit's *Args extends.
struct ExportArgs {
    Planes seq;
    const uint32_t *cls_owner;           // owners of this width, in call order
    const uint32_t *cls_item0;           // [n_cls + 1] prefix of their chunk counts
    uint32_t n_cls, n_items;
    const uint32_t *owner_item0;         // [n_owners + 1] first work item of an owner in the call-wide numbering
    const uint32_t *owner_chunk0;        // first chunk of the owner's bin
    const uint32_t *chunk_contig, *chunk_rank, *contig_chunk;
    unsigned long long *item_cnt;        // count pass: records per work item
    const unsigned long long *item_off;  // fill pass: exclusive prefix of item_cnt (+ total)
    unsigned long long first, capacity;  // fill pass: the window of ranks that is written
    uint32_t *out_contig, *out_pos;
    uint8_t *out_code;
    // (keep `programs` the last member: profile_kernel's arguments then lie as they did when it was ProfileArgs' first, and so does its code)
    const uint32_t *programs;            // [n_cand][PROG6_DW] sliced to the width the candidate runs at
};

struct WorkItem {                        // wave-uniform
    uint32_t owner, item, chunk;
    unsigned long long off0;             // fill pass: rank of the item's first record
};

// index into cls_owner of the owner of work item `it` of this launch: the last entry of the prefix that is <= it (scalar loads,
// scalar control flow)
__device__ __forceinline__ uint32_t class_slot(const ExportArgs &a, uint32_t it) {
    const cu32p item0 = (cu32p)a.cls_item0;
    uint32_t lo = 0, hi = a.n_cls;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (item0[mid] <= it) lo = mid; else hi = mid;
    }
    return lo;
}

// The work item of this wave; false when it has none (past the end, or FILL and no rank of the item is in the window).
template <bool FILL>
__device__ __forceinline__ bool locate_item(const ExportArgs &a, WorkItem &w) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t it = blockIdx.x * 4 + wave;                          // wave-uniform from here on
    if (it >= a.n_items) return false;
    const uint32_t lo = class_slot(a, it);
    const uint32_t ck = it - ((cu32p)a.cls_item0)[lo];
    w.owner = ((cu32p)a.cls_owner)[lo];
    w.item = ((cu32p)a.owner_item0)[w.owner] + ck;
    w.chunk = ((cu32p)a.owner_chunk0)[w.owner] + ck;
    w.off0 = 0;
    if (FILL) {
        w.off0 = a.item_off[w.item];
        const unsigned long long off1 = a.item_off[w.item + 1];
        if (off1 == w.off0 || off1 <= a.first || w.off0 >= a.first + a.capacity) return false;
    }
    return true;
}

// the four per-strand state planes MP UP MM UM of a mod slot, as the host staged their addresses
__device__ __forceinline__ StatePlanes slot_planes(const unsigned long long *pl) {
    StatePlanes s;
    s.M = nullptr;
    s.U = nullptr;
    s.MP = reinterpret_cast<const uint32_t *>(pl[0]);
    s.UP = reinterpret_cast<const uint32_t *>(pl[1]);
    s.MM = reinterpret_cast<const uint32_t *>(pl[2]);
    s.UM = reinterpret_cast<const uint32_t *>(pl[3]);
    return s;
}

// both strands' occurrences of one program in the tile, into fresh accumulators
template <class K>
__device__ __forceinline__ void walk_strands(const uint32_t *program, const Tile<K> &tile, uint32_t (&af)[T_WORDS], uint32_t (&ar)[T_WORDS]) {
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) af[t] = ar[t] = 0xFFFFFFFFu;
    const cu32p prog = (cu32p)program;
    eval_strand<K>(prog, tile, af);
    eval_strand<K>(prog + K::PDW, tile, ar);
}

// The prologue of a work item: its chunk and the state words of `stp` loaded, the tile expanded, the owner's occurrences on '+' (af)
// and '-' (ar).  (Out-parameters, not members of a result: see the head of this file.)
template <class K>
__device__ __forceinline__ void find_occurrences(const ExportArgs &a, const WorkItem &w, const StatePlanes (&stp)[K::NS], int lane, RawChunk<K> &raw,
                                                 Tile<K> &tile, uint32_t (&af)[T_WORDS], uint32_t (&ar)[T_WORDS]) {
    raw.load(a.seq, stp, w.chunk, lane);
    tile.expand(raw);
    walk_strands<K>(a.programs + (size_t)w.owner * PROG6_DW, tile, af, ar);
}

// word t of a plane's T_WORDS + 2 words (the lane's own and one either side) seen `sh` positions further along '+': UP = sh >= 0
// (bits = sh), else bits = 32 + sh
template <bool UP>
__device__ __forceinline__ uint32_t shifted(const uint32_t (&w)[T_WORDS + 2], int t, uint32_t bits) {
    return UP ? alignbit(w[t + 2], w[t + 1], bits) : alignbit(w[t + 1], w[t], bits);
}

// the three disjoint states of one strand's word in one slot (a position called both ways is methylated)
struct States {
    uint32_t s[3];
    __device__ __forceinline__ States(uint32_t m, uint32_t u) : s{m, u & ~m, ~(m | u)} {}
};

// the occurrences af ('+') and ar ('-') of word t by the state of their own base in the slot's words s = MP UP MM UM: f / r [0] mod,
// [1] nomod, [2] nocall
__device__ __forceinline__ void split_states(const uint32_t (&s)[4][T_WORDS], int t, uint32_t af, uint32_t ar, uint32_t (&f)[3], uint32_t (&r)[3]) {
    const States sf(s[0][t], s[1][t]), sr(s[2][t], s[3][t]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        f[i] = af & sf.s[i];
        r[i] = ar & sr.s[i];
    }
}

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

// The fill pass of a work item.  sel(t, f, r): the positions of the lane's word t that are records, forward and reverse strand;
// code(t, bit, minus): the code of the record at `bit` of word t on the forward (minus = false) or reverse strand.
template <class Sel, class Code>
__device__ __forceinline__ void emit_records(const ExportArgs &a, const WorkItem &w, int lane, Sel sel, Code code) {
    // rank of the lane's first record = prefix of the item + records of the lanes before it
    uint32_t mine = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t f, r;
        sel(t, f, r);
        mine += __popc(f) + __popc(r);
    }
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    // (ranks are taken relative to the window: one unsigned comparison covers both of its ends)
    unsigned long long at = w.off0 + (incl - mine) - a.first;
    const uint32_t contig = ((cu32p)a.chunk_contig)[w.chunk];
    const uint32_t pos0 = (w.chunk - ((cu32p)a.contig_chunk)[contig]) * (uint32_t)CHUNK_BP + (uint32_t)lane * (T_WORDS * 32);
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t f, r;
        sel(t, f, r);
        uint32_t both = f | r;
        while (both) {                                                  // ascending position, '+' before '-'
            const uint32_t b = __builtin_ctz(both), bit = 1u << b;
            both &= both - 1;
            const uint32_t pos = pos0 + t * 32 + b;
            if (f & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos;
                    a.out_code[at] = (uint8_t)code(t, bit, false);
                }
                ++at;
            }
            if (r & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos;
                    a.out_code[at] = (uint8_t)code(t, bit, true);
                }
                ++at;
            }
        }
    }
}

// owner_offset[k] = rank of owner k's first record (k = n_owners: the call's total)
static __global__ void export_gather_kernel(const unsigned long long *__restrict__ item_off, const uint32_t *__restrict__ owner_item0, uint32_t n,
                                            unsigned long long *__restrict__ owner_offset) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) owner_offset[k] = item_off[owner_item0[k]];
}

// a unit's kernel at G = 1, 2, 3, count or fill pass
template <class Args>
using ExportKernels = void (*const[3])(Args);

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// One table in the batch's block: uploaded from `src`, or (no src) reserved and zeroed for the count pass.  `field` is the pointer,
// usually of the unit's Args, that receives its device address.
struct ExportTable {
    void *field;
    const void *src;
    size_t bytes;
    template <class T>
    ExportTable(T **f, const void *s, size_t b) : field(f), src(s), bytes(b) {}
    template <class T>
    ExportTable(T **f, size_t b) : field(f), src(nullptr), bytes(b) {}
    void wire(uint8_t *p) const { memcpy(field, &p, sizeof p); }
};

// Everything a call needs on the device, in one block: the staged tables, the item table(s), the count table(s).
template <class Args>
struct ExportBatch {
    nm_ctx *c = nullptr;
    uint8_t *d = nullptr;
    Args base{};
    uint32_t cls_n[3] = {0, 0, 0}, cls_items[3] = {0, 0, 0};
    const uint32_t *cls_owner[3] = {}, *cls_item0[3] = {};
    unsigned long long *d_owner_offset = nullptr;
    ~ExportBatch() {
        if (!c) return;
        (void)hipStreamSynchronize(c->stream);                           // nothing may still read the block
        if (d) (void)dev_free(d);
    }
    // one launch per width that has work items
    int launch(ExportKernels<Args> &kernels, const Args &a) {
        for (int g = 0; g < 3; ++g) {
            if (!cls_items[g]) continue;
            Args ag = a;
            ag.cls_owner = cls_owner[g];
            ag.cls_item0 = cls_item0[g];
            ag.n_cls = cls_n[g];
            ag.n_items = cls_items[g];
            hipLaunchKernelGGL(kernels[g], dim3((ag.n_items + 3) / 4), dim3(256), 0, c->stream, ag);
            HIP_TRY(hipGetLastError());
            c->launches += 1;
        }
        return NM_OK;
    }
};

// The motif arguments of an entry point and, with their number and bins, its candidates (include/nmscan.h: as nm_score_batch takes them).
struct Motifs {
    const uint8_t *len, *modpos;
    const uint32_t *mask_offset;
    const uint8_t *masks;
};
struct Candidates {
    uint32_t n;
    const uint32_t *bin;
    Motifs motifs;
};

// The addresses of MP UP MM UM of a mod slot, for slot_planes; `arg`[i] is where the caller named the slot.
inline int slot_state_planes(const nm_ctx *c, const char *arg, uint32_t i, uint32_t slot, unsigned long long *out) {
    if (slot >= NM_MAX_MOD_SLOTS || !c->slots[slot].present || !c->slots[slot].planes[2])
        return fail(NM_ESTATE, "%s[%u]: no pileup uploaded in mod slot %u", arg, i, slot);
    for (int j = 0; j < 4; ++j) out[j] = (unsigned long long)(uintptr_t)c->slots[slot].planes[2 + j];
    return NM_OK;
}

// Motif k compiled into the six-group program full[PROG6_DW]; *reach: its width class (slice_program cuts it to a width).
inline int compile_motif(const Motifs &m, uint32_t k, uint32_t *full, int *reach) {
    return compile_program(m.masks + m.mask_offset[k], m.len[k], m.modpos[k], full, reach);
}

// What stage_candidates leaves for export_begin and the unit's uploads.
struct Staged {
    std::vector<uint32_t> programs, row0;    // [n][PROG6_DW]; first row of a candidate (zeros without rows)
    std::vector<unsigned long long> planes;  // [n][4] MP UP MM UM of cand_mod_slot (empty without it)
    std::vector<uint8_t> width;
    uint64_t rows = 0;
};

inline int no_check(uint32_t, uint32_t, uint64_t &) { return NM_OK; }

// The per-candidate staging of a call, every refusal in one order: bin, the mod slot (mod_slot != NULL: the call has a cand_mod_slot
// argument), check(k, bin, need) — the unit's own; `need` = rows the candidate takes, preset to the resident contigs of its bin —,
// program, rows, work items.  Rows: from the caller's row_offset, else (lay_rows) laid out here back to back, else none.
template <class Check>
int stage_candidates(const nm_ctx *c, const Candidates &cd, const uint8_t *mod_slot, const uint64_t *row_offset, bool lay_rows, Staged &st, Check check) {
    st.programs.assign((size_t)cd.n * PROG6_DW, 0);
    st.row0.assign(cd.n, 0);
    st.planes.assign(mod_slot ? (size_t)cd.n * 4 : 0, 0);
    st.width.assign(cd.n, 0);
    uint64_t items = 0;
    for (uint32_t k = 0; k < cd.n; ++k) {
        const uint32_t bin = cd.bin[k];
        if (bin >= c->n_bins) return fail(NM_EINVAL, "candidate %u: cand_bin %u >= n_bins %u", k, bin, c->n_bins);
        uint64_t need = c->bin_ncontigs[bin];
        uint32_t full[PROG6_DW];
        int reach = 0;
        int rc = mod_slot ? slot_state_planes(c, "cand_mod_slot", k, mod_slot[k], st.planes.data() + (size_t)k * 4) : NM_OK;
        if (!rc) rc = check(k, bin, need);
        if (!rc) rc = compile_motif(cd.motifs, k, full, &reach);
        if (rc) return rc;
        slice_program(full, reach + 1, st.programs.data() + (size_t)k * PROG6_DW);
        st.width[k] = (uint8_t)reach;
        if (row_offset || lay_rows) {
            const uint64_t r0 = row_offset ? row_offset[k] : st.rows, r1 = row_offset ? row_offset[k + 1] : st.rows + need;
            if (r1 < r0 || r1 - r0 < need)
                return fail(NM_EINVAL, "candidate %u: row_offset gives %llu rows, bin %u takes %llu", k, (unsigned long long)(r1 - r0), bin, (unsigned long long)need);
            if (r1 >= 0xFFFFFFFFull) return fail(NM_ERANGE, "more than 2^32 rows in one batch: send fewer candidates");
            st.row0[k] = (uint32_t)r0;
            st.rows = r1;
        }
        items += c->bin_nchunks[bin];
        if (items >= 0xFFFFFFF0ull) return fail(NM_ERANGE, "more than 2^32 (candidate, chunk) work items in one batch: send fewer candidates");
    }
    return NM_OK;
}

// Stage a validated call and enqueue its count pass (and, with_scan, the prefix + gather).  owner_bin / owner_width: per owner its
// bin and width class 0..2; the work items (one per chunk of the bin) must number less than 2^32 in all.  programs: of every
// candidate; uploads / reserved: the unit's own tables, wired into eb.base before the count pass runs; eb.base holds whatever else
// the unit has set.
template <class Args>
int export_begin(ExportBatch<Args> &eb, nm_ctx *c, uint32_t n_owners, const uint32_t *owner_bin, const uint8_t *owner_width,
                 const std::vector<uint32_t> &programs, const std::vector<ExportTable> &uploads, const std::vector<ExportTable> &reserved,
                 ExportKernels<Args> &count_kernels, bool with_scan) {
    std::vector<uint32_t> item0(n_owners + 1, 0), chunk0(n_owners, 0), cls_owner[3], cls_item0[3];
    uint32_t items = 0;
    for (uint32_t k = 0; k < n_owners; ++k) {                             // reach-class lists with class-local prefixes of the chunk counts
        const uint32_t nch = c->bin_nchunks[owner_bin[k]], g = owner_width[k];
        item0[k] = items;
        chunk0[k] = c->bin_chunk0[owner_bin[k]];
        if (nch) {
            cls_owner[g].push_back(k);
            cls_item0[g].push_back(eb.cls_items[g]);
        }
        eb.cls_items[g] += nch;
        items += nch;
    }
    item0[n_owners] = items;
    for (int g = 0; g < 3; ++g) {
        cls_item0[g].push_back(eb.cls_items[g]);
        eb.cls_n[g] = (uint32_t)cls_owner[g].size();
    }
    // per chunk: its contig and the contig's rank in its bin (pad chunks: never touched, no work item covers them)
    std::vector<uint32_t> chunk_contig(c->n_chunks, 0), chunk_rank(c->n_chunks, 0);
    for (uint32_t i = 0; i < c->n_contigs; ++i)
        for (uint32_t q = 0; q < c->contig_nchunks[i]; ++q) {
            chunk_contig[c->contig_chunk[i] + q] = i;
            chunk_rank[c->contig_chunk[i] + q] = c->contig_rank[i];
        }
    HIP_TRY(hipSetDevice(c->device));
    // ---- one device block: uploaded tables | zeroed tables | prefix, owner offsets, scan scratch
    Args &a = eb.base;
    std::vector<ExportTable> up = {{&a.owner_item0, item0.data(), item0.size() * 4},
                                   {&a.owner_chunk0, chunk0.data(), chunk0.size() * 4},
                                   {&a.chunk_contig, chunk_contig.data(), chunk_contig.size() * 4},
                                   {&a.chunk_rank, chunk_rank.data(), chunk_rank.size() * 4}};
    for (int g = 0; g < 3; ++g) {
        up.push_back({&eb.cls_owner[g], cls_owner[g].data(), cls_owner[g].size() * 4});
        up.push_back({&eb.cls_item0[g], cls_item0[g].data(), cls_item0[g].size() * 4});
    }
    up.push_back({&a.programs, programs.data(), programs.size() * 4});
    std::vector<ExportTable> zeroed = {{&a.item_cnt, ((size_t)items + 1) * 8}};
    up.insert(up.end(), uploads.begin(), uploads.end());
    zeroed.insert(zeroed.end(), reserved.begin(), reserved.end());
    size_t at = 0, scan_bytes = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align16(at + bytes); return o; };
    std::vector<size_t> o_up, o_zeroed;
    for (const ExportTable &t : up) o_up.push_back(take(t.bytes + 4));
    const size_t in_bytes = at;
    for (const ExportTable &t : zeroed) o_zeroed.push_back(take(t.bytes + 8));
    const size_t zero_bytes = at - in_bytes;
    const size_t o_off = take(with_scan ? ((size_t)items + 1) * 8 : 0), o_ooff = take(with_scan ? ((size_t)n_owners + 1) * 8 : 0);
    if (with_scan)
        HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)items + 1,
                                        rocprim::plus<unsigned long long>(), c->stream));
    const size_t o_scan = take(scan_bytes);
    eb.c = c;
    HIP_TRY(dev_malloc(&eb.d, at));
    std::vector<uint8_t> h(in_bytes, 0);
    for (size_t j = 0; j < up.size(); ++j) {
        if (up[j].bytes) memcpy(h.data() + o_up[j], up[j].src, up[j].bytes);
        up[j].wire(eb.d + o_up[j]);
    }
    for (size_t j = 0; j < zeroed.size(); ++j) zeroed[j].wire(eb.d + o_zeroed[j]);
    HIP_TRY(hipMemcpyAsync(eb.d, h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                              // (h is pageable memory of this frame)
    HIP_TRY(hipMemsetAsync(eb.d + in_bytes, 0, zero_bytes, c->stream));
    a.seq = seq_planes(c);
    a.contig_chunk = c->d_contig_chunk;
    a.item_off = reinterpret_cast<const unsigned long long *>(eb.d + o_off);
    eb.d_owner_offset = reinterpret_cast<unsigned long long *>(eb.d + o_ooff);
    const int rc = eb.launch(count_kernels, a);
    if (rc) return rc;
    if (with_scan) {
        HIP_TRY(rocprim::exclusive_scan(eb.d + o_scan, scan_bytes, a.item_cnt, const_cast<unsigned long long *>(a.item_off), 0ull, (size_t)items + 1,
                                        rocprim::plus<unsigned long long>(), c->stream));
        hipLaunchKernelGGL(export_gather_kernel, dim3((n_owners + 256) / 256), dim3(256), 0, c->stream, a.item_off, a.owner_item0, n_owners + 1,
                           eb.d_owner_offset);
        HIP_TRY(hipGetLastError());
        c->launches += 2;
    }
    return NM_OK;
}

// The second half of a *_sites entry point, after export_begin(..., with_scan = true): the owners' offsets to the host, the
// window [first_record, first_record + capacity) clamped to the call's total, the fill pass, and the window's records to the host.
template <class Args>
int export_window(ExportBatch<Args> &eb, ExportKernels<Args> &fill_kernels, uint32_t n_owners, uint64_t first_record, uint64_t capacity,
                  uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code, uint64_t *owner_offset, uint64_t *n_written) {
    nm_ctx *c = eb.c;
    HIP_TRY(hipMemcpyAsync(owner_offset, eb.d_owner_offset, (size_t)(n_owners + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = owner_offset[n_owners];
    const uint64_t n = first_record >= total ? 0 : std::min<uint64_t>(capacity, total - first_record);
    if (n == 0) return NM_OK;
    uint8_t *d_out = nullptr;                                             // contig | pos | code of the window's records
    const size_t o_pos = align16((size_t)n * 4), o_code = o_pos + align16((size_t)n * 4);
    HIP_TRY(dev_malloc(&d_out, o_code + (size_t)n));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)dev_free(p); } } guard{d_out, c};
    Args a = eb.base;
    a.first = first_record;
    a.capacity = n;
    a.out_contig = reinterpret_cast<uint32_t *>(d_out);
    a.out_pos = reinterpret_cast<uint32_t *>(d_out + o_pos);
    a.out_code = d_out + o_code;
    const int rc = eb.launch(fill_kernels, a);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(site_contig, a.out_contig, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_pos, a.out_pos, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_code, a.out_code, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_written = n;
    return NM_OK;
}

}  // namespace nmdetail
