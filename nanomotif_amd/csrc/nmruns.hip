// RUNS OF SAME-STATE MOTIF SITES along contigs: for every candidate of a batch and every contig of its bin, the maximal stretches of
// consecutive sites in one state (mod / nomod, with nocall_breaks also nocall; without it a nocall site is transparent) — counted into a
// run-length histogram per (candidate, contig) and exported as records (start, state, last, n_sites).  The first export whose result at
// a site depends on other sites at unbounded distance: a run crosses words, lanes, chunks and whole chunks without a site.
// An occurrence is nm_motif_sites' (nmsites.hip).  The fourteenth consumer of nmexport.h:
//   runs_kernel<G, FILL>  one wave per work item = (candidate, chunk of its bin).  The two strands' occurrences are ORed into an element
//          plane and two state planes per word.  "State of the last element before this lane" is a wave scan whose operator keeps the
//          right operand if it has an element; a lane then walks its element bits (ctz loop: motif sites are sparse) — an element whose
//          predecessor has another state, and the chunk's first element, START a run.  A lane closes the runs that start and end inside
//          it; the run left open at its end gets its length and last position from a segmented SUFFIX scan over the lanes (value = the
//          elements before a lane's first start, flag = the lane has a start).  A run belongs to the lane, and the work item, it starts
//          in.  The chunk's first run (head) and last run (tail) may go on in the neighbouring chunks: they go into the item's SUMMARY
//          (n_runs 0 / 1 / >= 2; with one run head == tail).  Every other run is final:
//            count  into a wave-private LDS histogram flushed to the (candidate, contig) row with 64-bit atomics (as gc_kernel does),
//                   atomicMax for the longest; the qualifying ones are the item's record count so far
//            fill   into records, behind the item's head slot if the stitch flagged it and before its flagged tail slot: that is by start
//   runs_stitch_kernel  one thread per (candidate, contig) row walks the contig's item summaries in chunk order with one open run as
//          carry: an empty chunk is transparent, a head of the carry's state extends it, anything else and the contig's end close it.  A
//          closed border run is added to the row; if it qualifies as a record it is attributed to the item it started in: that item's
//          count is raised and the run's final (n_sites, last) written into the item's head or tail slot, with a flag.
//   the prefix over the items (rocPRIM) and export_gather_kernel come AFTER the stitch, enqueued here: export_begin runs without its scan.
#include "nmexport.h"

using namespace nmdetail;

namespace {

constexpr int RUNS_MAX_R = NM_RUNS_MAX_MAX_RUN;
constexpr int RUNS_MAX_CELLS = 3 * (3 + RUNS_MAX_R);
constexpr int RUNS_SUMM_DW = 12;                 // an item's summary: n_runs, flags, head {state, len, start, last}, tail {...}, 2 unused
constexpr uint32_t RUNS_HEAD = 1u, RUNS_TAIL = 2u;   // flags: the slot's run is a record of this item
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int LANE_BP = T_WORDS * 32;

struct RunsArgs : ExportArgs {
    const uint32_t *cand_row0;               // first row of the candidate in the (candidate, contig) table
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    const uint32_t *row_item0, *row_nchunks; // [n_rows] the work items of the row's contig (rows no contig takes: 0 chunks)
    uint32_t state_set, min_run;             // which runs are records (state_set 0: none, the count call)
    uint32_t max_run, nocall_breaks, n_rows;
    unsigned long long *table;               // [n_rows][3][3 + max_run]
    uint32_t *summ;                          // [items][RUNS_SUMM_DW]
    unsigned long long *scan_off, *owner_off;   // the prefix of item_cnt and the owners' first ranks: written after the stitch
    uint8_t *scan_tmp;
    uint32_t *out_last, *out_n;              // fill pass: the two columns beside out_contig / out_pos / out_code
};

struct Run {
    uint32_t state, len, start, last;        // positions relative to the chunk until they are stored
};

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool qualifies(const RunsArgs &a, uint32_t state, uint32_t len) { return (a.state_set >> state & 1u) && len >= a.min_run; }

// What a lane knows after walking its element bits.
struct LaneRuns {
    uint32_t pre, pre_last;                  // elements before the lane's first start, the last of them (NONE: none)
    uint32_t nstarts;
    bool first_closed;                       // the lane's first run ends inside the lane (nstarts >= 2): `first`
    Run first, open;                         // open: the run of the lane's last start, as far as the lane sees it
};

// One walk over the lane's elements.  prev: the state of the last element before the lane (3: none).  later(run): the runs that start
// second or later in the lane and end inside it — never the chunk's head (another start precedes them), never its tail (one follows).
template <class F>
__device__ __forceinline__ void walk_lane(const uint32_t (&e)[T_WORDS], const uint32_t (&sm)[T_WORDS], const uint32_t (&su)[T_WORDS], uint32_t lane_pos,
                                          uint32_t prev, LaneRuns &lr, F later) {
    lr.pre = 0;
    lr.pre_last = NONE;
    lr.nstarts = 0;
    lr.first_closed = false;
    Run r{3u, 0u, 0u, 0u};
    lr.first = r;
    uint32_t cur = prev;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t x = e[t];
        while (x) {
            const uint32_t b = __builtin_ctz(x), bit = 1u << b;
            x &= x - 1;
            const uint32_t p = lane_pos + t * 32 + b, s = (sm[t] & bit) ? 0u : (su[t] & bit) ? 1u : 2u;
            if (s != cur) {                                               // a start (prev = 3: the chunk's first element is one)
                if (lr.nstarts == 1) {
                    lr.first = r;
                    lr.first_closed = true;
                } else if (lr.nstarts > 1) {
                    later(r);
                }
                r = Run{s, 0u, p, p};
                lr.nstarts += 1;
                cur = s;
            }
            if (lr.nstarts) {
                r.len += 1;
                r.last = p;
            } else {
                lr.pre += 1;
                lr.pre_last = p;
            }
        }
    }
    lr.open = r;
}

template <int G, bool FILL>
__global__ __launch_bounds__(256) void runs_kernel(RunsArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<FILL>(a, w)) return;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.cand_planes + (size_t)k * 4)};
    RawChunk<K> raw;
    Tile<K> tile;
    uint32_t af[T_WORDS], ar[T_WORDS];
    find_occurrences<K>(a, w, stp, lane, raw, tile, af, ar);
    // the element plane and the state planes mod / nomod of the lane's words, '+' and '-' ORed (nocall = e & ~(sm | su))
    uint32_t e[T_WORDS], sm[T_WORDS], su[T_WORDS], sites[3] = {0, 0, 0}, any = 0;
    const bool nb = a.nocall_breaks != 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t f[3], r[3];
        split_states(raw.s[0], t, af[t], ar[t], f, r);
#pragma unroll
        for (int i = 0; i < 3; ++i) sites[i] += __popc(f[i]) + __popc(r[i]);
        sm[t] = f[0] | r[0];
        su[t] = (f[1] | r[1]) & ~sm[t];
        e[t] = nb ? (af[t] | ar[t]) : (sm[t] | su[t]);
        any |= af[t] | ar[t];
    }
    if (!__any((int)(any != 0))) return;                                 // wave-uniform: no occurrence, the item's summary stays n_runs = 0
    // the state of the last element before this lane: an inclusive scan that keeps the right operand if it has an element, moved one lane up
    uint32_t prev;
    {
        uint32_t x = 3u;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t)
            if (e[t]) {
                const uint32_t bit = 0x80000000u >> __builtin_clz(e[t]);
                x = (sm[t] & bit) ? 0u : (su[t] & bit) ? 1u : 2u;
            }
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(x, o);
            if (lane >= o && x == 3u) x = up;
        }
        prev = __shfl_up(x, 1);
        if (lane == 0) prev = 3u;                                         // the chunk's first element starts a run; the stitch joins chunks
    }
    const uint32_t lane_pos = (uint32_t)lane * LANE_BP;
    const uint32_t R = a.max_run, stride = 3 + R, cells = 3 * stride;
    uint32_t *hist = nullptr;
    if constexpr (!FILL) {
        __shared__ uint32_t lds[4][RUNS_MAX_CELLS];
        hist = lds[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];     // this wave's [3][3 + R] counters
        for (uint32_t j = (uint32_t)lane; j < cells; j += 64) hist[j] = 0;
        wave_fence();
    }
    uint32_t mine = 0;                                                    // qualifying final runs of the lane
    auto final_run = [&](const Run &r) {                                  // count pass: a run that is neither the chunk's head nor its tail
        if constexpr (!FILL) {
            uint32_t *h = hist + r.state * stride;
            atomicAdd(h + 0, 1u);
            atomicMax(h + 2, r.len);
            atomicAdd(h + 3 + (r.len < R ? r.len : R) - 1, 1u);
        }
        mine += qualifies(a, r.state, r.len) ? 1u : 0u;
    };
    LaneRuns lr;
    walk_lane(e, sm, su, lane_pos, prev, lr, final_run);
    // the lanes with a start; the segmented suffix scan over (pre, pre_last, has a start) that closes the lanes' open runs
    const unsigned long long has = __ballot((int)(lr.nstarts != 0));
    // (has == 0: occurrences, but no element — nocall sites that do not take part; their count still goes to the row)
    if (FILL && has == 0) return;
    const int first_lane = has ? __builtin_ctzll(has) : 64, last_lane = has ? 63 - __builtin_clzll(has) : 64;
    uint32_t sv = lr.pre, sp = lr.pre_last, sf = lr.nstarts ? 1u : 0u;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t ov = __shfl_down(sv, o), op = __shfl_down(sp, o), of = __shfl_down(sf, o);
        if (lane + o < 64 && !sf) {
            sv += ov;
            if (op != NONE) sp = op;
            sf = of;
        }
    }
    uint32_t xv = __shfl_down(sv, 1), xp = __shfl_down(sp, 1), xf = __shfl_down(sf, 1);
    if (lane == 63) {
        xv = 0;
        xp = NONE;
        xf = 0;
    }
    Run open = lr.open;                                                   // (meaningful with nstarts != 0)
    open.len += xv;
    if (xp != NONE) open.last = xp;
    const bool open_is_tail = lr.nstarts != 0 && !xf;                     // no start follows: lane == last_lane
    const bool open_is_head = lane == first_lane && lr.nstarts == 1;
    const bool first_is_head = lane == first_lane && lr.first_closed;
    const bool first_final = lr.first_closed && !first_is_head, open_final = lr.nstarts != 0 && !open_is_tail && !open_is_head;
    uint32_t n_runs = lr.nstarts;
    for (int o = 32; o; o >>= 1) n_runs += __shfl_xor(n_runs, o);
    if (!FILL) {
        if (first_final) final_run(lr.first);
        if (open_final) final_run(open);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (sites[i]) atomicAdd(hist + i * stride + 1, sites[i]);
        uint32_t total = mine;
        for (int o = 32; o; o >>= 1) total += __shfl_xor(total, o);
        uint32_t *s = a.summ + (size_t)w.item * RUNS_SUMM_DW;
        if (lane == 0) {
            a.item_cnt[w.item] = total;                                   // the stitch adds the border runs it attributes to this item
            s[0] = n_runs < 2 ? n_runs : 2u;
            s[1] = 0;
        }
        if (lane == first_lane) {
            const Run h = lr.first_closed ? lr.first : open;
            s[2] = h.state; s[3] = h.len; s[4] = h.start; s[5] = h.last;
        }
        if (lane == last_lane) {
            s[6] = open.state; s[7] = open.len; s[8] = open.start; s[9] = open.last;
        }
        wave_fence();
        const uint32_t row = ((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk];
        if (row >= a.n_rows) return;
        unsigned long long *out = a.table + (size_t)row * cells;
        for (uint32_t j = (uint32_t)lane; j < cells; j += 64) {
            const uint32_t n = hist[j];
            if (!n) continue;
            if (j % stride == 2) atomicMax(out + j, (unsigned long long)n);
            else atomicAdd(out + j, (unsigned long long)n);
        }
        return;
    }
    // ---- fill: the item's flagged head slot, its final runs by start, its flagged tail slot
    const bool q_first = first_final && qualifies(a, lr.first.state, lr.first.len), q_open = open_final && qualifies(a, open.state, open.len);
    mine += (q_first ? 1u : 0u) + (q_open ? 1u : 0u);
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    const uint32_t total = __shfl(incl, 63);
    const uint32_t *s = a.summ + (size_t)w.item * RUNS_SUMM_DW;
    const uint32_t flags = s[1];
    const uint32_t contig = ((cu32p)a.chunk_contig)[w.chunk];
    const uint32_t chunk_pos = (w.chunk - ((cu32p)a.contig_chunk)[contig]) * (uint32_t)CHUNK_BP;
    // (ranks are taken relative to the window: one unsigned comparison covers both of its ends)
    const unsigned long long at0 = w.off0 - a.first;
    auto put = [&](unsigned long long at, uint32_t state, uint32_t start, uint32_t last, uint32_t n) {
        if (at < a.capacity) {
            a.out_contig[at] = contig;
            a.out_pos[at] = start;
            a.out_code[at] = (uint8_t)state;
            a.out_last[at] = last;
            a.out_n[at] = n;
        }
    };
    if (lane == 0 && (flags & RUNS_HEAD)) put(at0, s[2], s[4], s[5], s[3]);                         // (positions in the summary are the contig's)
    if (lane == 0 && (flags & RUNS_TAIL)) put(at0 + (flags & RUNS_HEAD) + total, s[6], s[8], s[9], s[7]);
    unsigned long long at = at0 + (flags & RUNS_HEAD) + (incl - mine);
    if (q_first) put(at++, lr.first.state, chunk_pos + lr.first.start, chunk_pos + lr.first.last, lr.first.len);
    if (mine > (q_first ? 1u : 0u) + (q_open ? 1u : 0u)) {                // the runs between them: the same walk again, now writing
        LaneRuns again;
        walk_lane(e, sm, su, lane_pos, prev, again, [&](const Run &r) {
            if (qualifies(a, r.state, r.len)) put(at++, r.state, chunk_pos + r.start, chunk_pos + r.last, r.len);
        });
    }
    if (q_open) put(at, open.state, chunk_pos + open.start, chunk_pos + open.last, open.len);
}

// One thread per (candidate, contig) row: the border runs of the contig's work items joined in chunk order.
__global__ __launch_bounds__(64) void runs_stitch_kernel(RunsArgs a) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.n_rows) return;
    const uint32_t n = a.row_nchunks[row], item0 = a.row_item0[row];
    const uint32_t R = a.max_run, stride = 3 + R;
    unsigned long long *out = a.table + (size_t)row * 3 * stride;
    Run carry{3u, 0u, 0u, 0u};                                            // state 3: none open
    uint32_t c_item = 0, c_slot = 0;                                      // where the carry started: its item, 0 head / 1 tail
    auto close = [&](const Run &r, uint32_t item, uint32_t slot) {
        unsigned long long *h = out + r.state * stride;
        h[0] += 1;
        if (h[2] < r.len) h[2] = r.len;
        h[3 + (r.len < R ? r.len : R) - 1] += 1;
        if (qualifies(a, r.state, r.len)) {
            uint32_t *s = a.summ + (size_t)item * RUNS_SUMM_DW;
            a.item_cnt[item] += 1;
            s[1] |= slot ? RUNS_TAIL : RUNS_HEAD;
            s[2 + 4 * slot + 1] = r.len;
            s[2 + 4 * slot + 2] = r.start;
            s[2 + 4 * slot + 3] = r.last;
        }
    };
    for (uint32_t q = 0; q < n; ++q) {
        const uint32_t item = item0 + q;
        const uint32_t *s = a.summ + (size_t)item * RUNS_SUMM_DW;
        const uint32_t n_runs = s[0];
        if (n_runs == 0) continue;                                        // a chunk without an element is transparent
        const uint32_t pos = q * (uint32_t)CHUNK_BP;
        const Run head{s[2], s[3], pos + s[4], pos + s[5]}, tail{s[6], s[7], pos + s[8], pos + s[9]};
        if (carry.state == head.state) {                                  // the head goes on with the open run
            carry.len += head.len;
            carry.last = head.last;
            if (n_runs == 1) continue;
            close(carry, c_item, c_slot);
        } else {
            if (carry.state != 3u) close(carry, c_item, c_slot);
            if (n_runs == 1) {
                carry = head;
                c_item = item;
                c_slot = 0;
                continue;
            }
            close(head, item, 0);
        }
        carry = tail;
        c_item = item;
        c_slot = 1;
    }
    if (carry.state != 3u) close(carry, c_item, c_slot);
}

template <bool FILL>
constexpr ExportKernels<RunsArgs> runs_kernels = {runs_kernel<1, FILL>, runs_kernel<2, FILL>, runs_kernel<3, FILL>};
using RunsBatch = ExportBatch<RunsArgs>;

int check_runs_args(uint32_t state_set, uint32_t min_run, uint32_t max_run, int nocall_breaks, bool records) {
    if (!records) {
        if (max_run < NM_RUNS_MIN_MAX_RUN || max_run > NM_RUNS_MAX_MAX_RUN)
            return fail(NM_EINVAL, "max_run %u outside %d..%d", max_run, NM_RUNS_MIN_MAX_RUN, NM_RUNS_MAX_MAX_RUN);
        return NM_OK;
    }
    if (min_run < 1) return fail(NM_EINVAL, "min_run %u: at least 1", min_run);
    if (state_set == 0 || (state_set & ~7u)) return fail(NM_EINVAL, "state_set %u: a non-empty combination of NM_SITES_MOD / NOMOD / NOCALL", state_set);
    if ((state_set & NM_SITES_NOCALL) && !nocall_breaks) return fail(NM_EINVAL, "state_set %u: NM_SITES_NOCALL runs exist with nocall_breaks only", state_set);
    return NM_OK;
}

// validate the batch, stage the tables, and enqueue the count pass, the stitch and (records) the prefix + gather
int runs_begin(RunsBatch &rb, nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
               const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, const uint64_t *row_offset, uint32_t state_set,
               uint32_t min_run, uint32_t max_run, int nocall_breaks, bool records) {
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (row_offset && row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
    Staged st;
    const int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, cand_mod_slot, row_offset, !row_offset, st, no_check);
    if (rc) return rc;
    // the work items of every row's contig, in the numbering export_begin gives them: owner k's items follow its bin's chunks
    const uint32_t rows = (uint32_t)st.rows;
    std::vector<uint32_t> row_item0(rows, 0), row_nchunks(rows, 0);
    uint64_t items = 0;
    {
        std::vector<std::vector<uint32_t>> bin_contigs(c->n_bins);
        for (uint32_t i = 0; i < c->n_contigs; ++i)
            if (c->contig_bin[i] < c->n_bins) bin_contigs[c->contig_bin[i]].push_back(i);
        for (uint32_t k = 0; k < n_cand; ++k) {
            const uint32_t bin = cand_bin[k];
            for (const uint32_t i : bin_contigs[bin]) {
                const uint32_t row = st.row0[k] + c->contig_rank[i];
                if (row >= rows || c->contig_chunk[i] < c->bin_chunk0[bin] || c->contig_chunk[i] - c->bin_chunk0[bin] + c->contig_nchunks[i] > c->bin_nchunks[bin])
                    continue;                                             // (a bin's contigs lie back to back in its chunk range)
                row_item0[row] = (uint32_t)items + (c->contig_chunk[i] - c->bin_chunk0[bin]);
                row_nchunks[row] = c->contig_nchunks[i];
            }
            items += c->bin_nchunks[bin];
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    size_t scan_bytes = 0;
    if (records)
        HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)items + 1,
                                        rocprim::plus<unsigned long long>(), c->stream));
    RunsArgs &a = rb.base;
    a.state_set = records ? state_set : 0u;
    a.min_run = min_run;
    a.max_run = max_run;
    a.nocall_breaks = nocall_breaks ? 1u : 0u;
    a.n_rows = rows;
    const int rc2 = export_begin(rb, c, n_cand, cand_bin, st.width.data(), st.programs,
                                 {{&a.cand_row0, st.row0.data(), st.row0.size() * 4},
                                  {&a.cand_planes, st.planes.data(), st.planes.size() * 8},
                                  {&a.row_item0, row_item0.data(), row_item0.size() * 4},
                                  {&a.row_nchunks, row_nchunks.data(), row_nchunks.size() * 4}},
                                 {{&a.table, (size_t)rows * 3 * (3 + max_run) * 8},
                                  {&a.summ, (size_t)items * RUNS_SUMM_DW * 4},
                                  {&a.scan_off, records ? ((size_t)items + 1) * 8 : 0},
                                  {&a.owner_off, records ? ((size_t)n_cand + 1) * 8 : 0},
                                  {&a.scan_tmp, scan_bytes}},
                                 runs_kernels<false>, false);
    if (rc2) return rc2;
    if (rows) {
        hipLaunchKernelGGL(runs_stitch_kernel, dim3((rows + 63) / 64), dim3(64), 0, c->stream, a);
        HIP_TRY(hipGetLastError());
        c->launches += 1;
    }
    if (records) {
        HIP_TRY(rocprim::exclusive_scan(a.scan_tmp, scan_bytes, a.item_cnt, a.scan_off, 0ull, (size_t)items + 1, rocprim::plus<unsigned long long>(), c->stream));
        hipLaunchKernelGGL(export_gather_kernel, dim3((n_cand + 256) / 256), dim3(256), 0, c->stream, a.scan_off, a.owner_item0, n_cand + 1, a.owner_off);
        HIP_TRY(hipGetLastError());
        c->launches += 2;
        a.item_off = a.scan_off;
    }
    return NM_OK;
}

// export_window of nmexport.h with five columns
int runs_window(RunsBatch &rb, uint32_t n_cand, uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                uint32_t *site_last, uint32_t *site_n, uint64_t *cand_offset, uint64_t *n_written) {
    nm_ctx *c = rb.c;
    HIP_TRY(hipMemcpyAsync(cand_offset, rb.base.owner_off, (size_t)(n_cand + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = cand_offset[n_cand];
    const uint64_t n = first_record >= total ? 0 : std::min<uint64_t>(capacity, total - first_record);
    if (n == 0) return NM_OK;
    uint8_t *d_out = nullptr;                                             // contig | pos | last | n | code of the window's records
    const size_t col = align16((size_t)n * 4);
    HIP_TRY(dev_malloc(&d_out, 4 * col + (size_t)n));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)dev_free(p); } } guard{d_out, c};
    RunsArgs a = rb.base;
    a.first = first_record;
    a.capacity = n;
    a.out_contig = reinterpret_cast<uint32_t *>(d_out);
    a.out_pos = reinterpret_cast<uint32_t *>(d_out + col);
    a.out_last = reinterpret_cast<uint32_t *>(d_out + 2 * col);
    a.out_n = reinterpret_cast<uint32_t *>(d_out + 3 * col);
    a.out_code = d_out + 4 * col;
    const int rc = rb.launch(runs_kernels<true>, a);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(site_contig, a.out_contig, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_pos, a.out_pos, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_last, a.out_last, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_n, a.out_n, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_code, a.out_code, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_written = n;
    return NM_OK;
}

}  // namespace

int nm_motif_runs_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                        const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t max_run, int nocall_breaks,
                        const uint64_t *row_offset, int64_t *contig_rows) {
    if (!row_offset || (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !contig_rows)))
        return fail(NM_EINVAL, "NULL argument");
    if (const int rc = check_runs_args(0, 1, max_run, nocall_breaks, false)) return rc;
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) return NM_OK;
    RunsBatch rb;
    const int rc = runs_begin(rb, c, n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks, row_offset, 0, 1, max_run, nocall_breaks,
                              false);
    if (rc) return rc;
    const uint64_t rows = row_offset[n_cand];
    if (rows) HIP_TRY(hipMemcpyAsync(contig_rows, rb.base.table, (size_t)rows * 3 * (3 + max_run) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}

int nm_motif_runs_sites(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                        const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t state_set, uint32_t min_run,
                        int nocall_breaks, uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                        uint32_t *site_last, uint32_t *site_n, uint64_t *cand_offset, uint64_t *n_written) {
    if (!cand_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code || !site_last || !site_n)) ||
        (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks)))
        return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (const int rc = check_runs_args(state_set, min_run, NM_RUNS_MIN_MAX_RUN, nocall_breaks, true)) return rc;
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) {
        cand_offset[0] = 0;
        return NM_OK;
    }
    RunsBatch rb;
    const int rc = runs_begin(rb, c, n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr, state_set, min_run,
                              NM_RUNS_MIN_MAX_RUN, nocall_breaks, true);
    if (rc) return rc;
    return runs_window(rb, n_cand, first_record, capacity, site_contig, site_pos, site_code, site_last, site_n, cand_offset, n_written);
}
