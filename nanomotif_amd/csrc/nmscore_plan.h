// The plan of one scoring batch: everything score_impl (nmscan.hip) decides before it enqueues anything — validation, the
// batch's class, the byte layout of the staging pair, the sorted tables written into it, the launch grid.  Pure integer work
// over plain inputs: no HIP type, no allocation, nothing of nm_ctx but the few facts of PlanFacts, so that a host compiler
// builds it and tools/plan_check/driver.cpp checks every step against a restatement (tests/test_score_plan_host.py).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/nmscan.h"

namespace nmdetail {

struct SpecSource;                                      // nmscan_internal.h: motifs written on the device

// One candidate record as the host stages it (sorted by mod-type slot, then bin).
struct CandRec {
    uint32_t mask_off;   // into the staged mask bytes
    uint32_t orig;       // caller's index of this candidate
    uint8_t len, modpos, slot, pad;
};

struct PlanU4 { uint32_t x, y, z, w; };                 // a range or segment entry as the kernels read it (uint4)

constexpr size_t PLAN_STAGE_DIRECT_MAX = (size_t)4 << 20;      // count tables and staged tables up to here take the short ways
// candidates of a (slot, bin) group one pass of score_kernel counts in LDS (BMAX, nmscan_internal.h), and what the parked class
// kernel has room for beside its park area (nmscan_device.h: Variant::PARK)
constexpr uint32_t PLAN_PASS_ROWS = 32, PLAN_PARK_ROWS = 28;
// workgroups a CU holds at once: the parked class kernel runs 7 waves per SIMD, every other heavy kernel 6 or fewer
constexpr uint32_t PLAN_RESIDENT_PER_CU = 6, PLAN_RESIDENT_PER_CU_PARKED = 7;

// What a scoring call is asked for; an entry point fills the fields it uses.
struct ScoreRequest {
    uint32_t n_cand = 0;
    const uint32_t *bin = nullptr;
    const uint8_t *slot = nullptr, *len = nullptr, *modpos = nullptr;
    const uint32_t *mask_off = nullptr;
    const uint8_t *masks = nullptr;
    unsigned long long *d_out = nullptr;                // device count table of the caller, or
    int64_t *h_out = nullptr;                           // host counts (neither: the ctx's own table)
    const uint64_t *row_offset = nullptr;               // per-contig counters: first output row of every candidate, [n_cand + 1]
    bool defer = false;                                 // host counts collected later (nm_score_batch_end); the call returns with everything enqueued
    const SpecSource *spec = nullptr;                   // the motifs are written on the device; always deferred, noted in spec_wait, on `stream`
    uint32_t spec_mask_stride = 0;                      // ... and what the plan reads of it: mask bytes per candidate,
    size_t spec_extra_in = 0, spec_extra_out = 0;       // the writer's bytes behind the staged tables and behind the counts
    void *stream = nullptr;                             // spec: the batch's stream
    int flight = 0;
};

// What planning reads of an nm_ctx.
struct PlanFacts {
    uint32_t n_bins = 0;
    const uint32_t *bin_nchunks = nullptr, *bin_chunk0 = nullptr, *bin_ncontigs = nullptr;
    uint32_t slot_present = 0, slot_is_c = 0;           // bit s: slot s holds a pileup / its canonical base is C
    uint32_t n_segments = 0, seg_chunks = 16, n_cus = 256;
    bool opt_no_lit = false, opt_no_cf = false, opt_no_inline = false;
    int opt_fine = -1, opt_split = -1;
    // the work lists of the heavy kernels (nmscore_worklist.h), [0] plain, [1] contig tails packed: per bin its first entry and its
    // entries, and the segments of the static table over list positions.  NULL: no lists, the chunk table serves every batch
    const uint32_t *list_start[2] = {nullptr, nullptr}, *list_len[2] = {nullptr, nullptr};
    uint32_t list_segments[2] = {0, 0};
};

enum PlanCompile { PLAN_COMPILE_NONE, PLAN_COMPILE_FUSED, PLAN_COMPILE_ONLY, PLAN_COMPILE_THEN_COMMON, PLAN_COMPILE_SPEC };

struct ScorePlan {
    int status = NM_OK;
    char err[192] = {0};
    // ---- classify
    int any_wide = 0;                                   // widest offset class of the batch: 0: offsets in [-32, 31], 1: [-64, 63], 2: [-96, 95]
    bool all_compact = true, all_literal = true, per_contig = false;
    uint32_t n_prog = 0;                                // resident candidates
    uint64_t mask_lo = 0, mask_hi = 0;                  // byte range of the mask pool they reference
    uint32_t n_active = 0, active[NM_MAX_MOD_SLOTS] = {};
    int slot_to_active[NM_MAX_MOD_SLOTS] = {};
    uint32_t n_active_bins = 0, n_groups = 0;
    size_t n_active_segs = 0;
    bool use_list = false, pack = false;                // the batch walks a work list (heavy, not per-contig), the one with packed tails
    bool park_fits = true;                              // no (slot, bin) group takes more passes at PLAN_PARK_ROWS candidates than at PLAN_PASS_ROWS
    uint64_t out_rows = 0;
    // ---- shape
    bool lit = false, light = false, cf = false, classes = false, cls_head = true, fuse = false;
    bool park = false;                                  // the class kernel that parks a chunk's state words in LDS (7 waves per SIMD)
    int cls_tail = 3;                                   // tail descriptors the class compiler writes: 1 literals, 2 the lone class
    bool own_segments = false, via_stage = false, inline_prep = false, by_kernels = false;
    PlanCompile compile = PLAN_COMPILE_NONE;
    uint32_t np = 8, pdw = 0, n_entries = 0;
    size_t prog_dw = 0;                                 // room the batch needs in the program buffer
    // ---- layout of the staging pair
    size_t off_orig = 0, off_masks = 0, off_range = 0, off_rows = 0, off_segs = 0, off_posof = 0, off_xin = 0, total = 0;
    size_t off_counts = 0, off_xout = 0, stage_end = 0;
    size_t range_bytes = 0, out_bytes = 0, clear_bytes = 0;
    // ---- geometry
    uint32_t n_segments = 0;                            // of the table the launch walks
    uint32_t split_log2 = 0, pieces_per_run = 0, fine_log2 = 0, j_big = 0, gx = 0, gy = 1;
    uint64_t last_wgs = 0;
};

inline size_t plan_align16(size_t x) { return (x + 15) & ~(size_t)15; }

#if defined(__HIPCC__)
#define NM_PLAN_HD __host__ __device__ __forceinline__
#else
#define NM_PLAN_HD inline
#endif

// The grid of a launch as score_kernel reads it (plan_geometry decides it).
struct PlanGrid { uint32_t n_segments, split_log2, pieces_per_run, j_big, fine_log2; };

// Workgroup `block` of the x dimension -> its piece of work, in the two steps score_kernel takes around its read of the segment
// table.  The grid is `runs` runs of pieces (8: the heavy variants — blocks b and b + 8 share an XCD under round-robin dispatch, so
// every XCD gets a contiguous run of segments and the programs and counters of one bin stay in one L2; 1: the streaming CF variants,
// where the remap costs 3 % of the read rate, tools/stream_pattern.hip).  A piece is a segment, or a half / quarter of one for
// assemblies that fill the device for less than two rounds of workgroups (split_log2); the workgroups dispatched LAST (j >= j_big
// in every run) take pieces cut finer still (fine_log2): the last, partly filled round of workgroups then lasts a quarter as long.
// plan_block_piece: the piece, and which part of it (sub of n_sub); false: the workgroup has none and leaves.
NM_PLAN_HD bool plan_block_piece(const PlanGrid &g, bool cf, uint32_t block, uint32_t *piece, uint32_t *sub, uint32_t *n_sub) {
    const uint32_t x = cf ? 0u : block % 8, j = cf ? block : block / 8;
    *sub = 0;
    *n_sub = 1;
    if (j < g.j_big) *piece = x * g.pieces_per_run + j;
    else {
        const uint32_t k = j - g.j_big;
        *piece = x * g.pieces_per_run + g.j_big + (k >> g.fine_log2);
        *sub = k & ((1u << g.fine_log2) - 1);
        *n_sub = 1u << g.fine_log2;
        if (g.j_big + (k >> g.fine_log2) >= g.pieces_per_run) return false;
    }
    return (*piece >> g.split_log2) < g.n_segments;    // its segment: piece >> split_log2
}
// plan_cut_piece: the piece's share [*first, *first + *count) of its segment's entries (in: the whole segment); false: an empty share.
NM_PLAN_HD bool plan_cut_piece(const PlanGrid &g, uint32_t piece, uint32_t sub, uint32_t n_sub, uint32_t *first, uint32_t *count) {
    if (g.split_log2) {
        const uint32_t len = (*count + (1u << g.split_log2) - 1) >> g.split_log2;
        const uint32_t at = (piece & ((1u << g.split_log2) - 1)) * len;
        if (at >= *count) return false;
        *first += at;
        *count = len < *count - at ? len : *count - at;
    }
    if (n_sub > 1) {
        const uint32_t len = (*count + n_sub - 1) / n_sub;
        const uint32_t at = sub * len;
        if (at >= *count) return false;
        *first += at;
        *count = len < *count - at ? len : *count - at;
    }
    return true;
}
// Both steps around a table in host memory: what tools/plan_check/driver.cpp walks to show that a planned grid reaches every entry
// of its table (chunks of the chunk table, positions of a work list) exactly once.
inline bool plan_decode_block(const PlanGrid &g, bool cf, uint32_t block, const PlanU4 *segments, uint32_t *seg, uint32_t *first, uint32_t *count) {
    uint32_t piece, sub, n_sub;
    if (!plan_block_piece(g, cf, block, &piece, &sub, &n_sub)) return false;
    *seg = piece >> g.split_log2;
    *first = segments[*seg].x;
    *count = segments[*seg].y;
    return plan_cut_piece(g, piece, sub, n_sub, first, count);
}

inline int plan_fail(ScorePlan &p, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
inline int plan_fail(ScorePlan &p, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.err, sizeof p.err, fmt, ap);
    va_end(ap);
    return p.status = code;
}

// The motif of candidate k: its length against `max_len`, the modified position, no empty set, one specified position.
// NM_OK or the status with its text in p.err; *literal: no 2- or 3-base set.
inline int check_motif(ScorePlan &p, uint32_t k, uint32_t len, uint32_t mp, const uint8_t *m, uint32_t max_len, bool *literal) {
    if (len == 0 || len > max_len) return plan_fail(p, NM_ERANGE, "candidate %u: motif length %u outside 1..%d", k, len, (int)max_len);
    if (mp >= len) return plan_fail(p, NM_EINVAL, "candidate %u: mod_position %u outside motif of length %u", k, mp, len);
    uint32_t all_and = 15u, any_zero = 0, any_set = 0;
    for (uint32_t j = 0; j < len; ++j) {
        const uint32_t v = m[j] & 15u;
        all_and &= v;
        any_zero |= (v == 0);
        any_set |= (v != 15u) & ((v & (v - 1)) != 0);      // a 2- or 3-base set
    }
    if (any_zero) return plan_fail(p, NM_EINVAL, "candidate %u: empty base set in the motif", k);
    if (all_and == 15u) return plan_fail(p, NM_EINVAL, "candidate %u: motif has no specified position", k);
    *literal = !any_set;
    return NM_OK;
}

// Active slots are numbered in ascending order: slot_to_active[s] = the index of slot s among the used ones, or -1.
inline uint32_t number_active_slots(const bool used[NM_MAX_MOD_SLOTS], int slot_to_active[NM_MAX_MOD_SLOTS], uint32_t *active = nullptr) {
    uint32_t n = 0;
    for (int s = 0; s < NM_MAX_MOD_SLOTS; ++s) {
        slot_to_active[s] = -1;
        if (!used[s]) continue;
        if (active) active[n] = (uint32_t)s;
        slot_to_active[s] = (int)n++;
    }
    return n;
}

// light: <= 6 candidates per (slot, bin) group on average (plan_shape)
inline bool plan_is_light(const ScorePlan &p) { return (uint64_t)p.n_prog <= 6ull * p.n_groups && !p.per_contig; }

// ---- 1. one pass over the candidates: validate, classify the batch, count per (slot, bin) bucket.
// bucket: NM_MAX_MOD_SLOTS * n_bins + 1 zeroed words, entry slot * n_bins + bin + 1 counts the group; bin_active: n_bins zeroed bytes.
// Candidates whose bin has no contig on this device (multi-GPU shard) contribute zero and get no program.
inline int plan_classify(ScorePlan &p, const ScoreRequest &rq, const PlanFacts &f, uint32_t *bucket, uint8_t *bin_active) {
    const uint32_t n_bins = f.n_bins;
    uint64_t mask_bytes = 0, mask_lo = ~0ull;
    bool slot_used[NM_MAX_MOD_SLOTS] = {};
    for (uint32_t k = 0; k < rq.n_cand; ++k) {
        const uint32_t slot = rq.slot[k], bin = rq.bin[k];
        if (slot >= NM_MAX_MOD_SLOTS || !(f.slot_present >> slot & 1u))
            return plan_fail(p, NM_ESTATE, "candidate %u uses mod slot %u with no pileup uploaded", k, slot);
        if (bin >= n_bins) return plan_fail(p, NM_EINVAL, "candidate %u: bin %u >= n_bins %u", k, bin, n_bins);
        if (f.bin_nchunks[bin] == 0) continue;          // not resident here: the rank that holds the bin validates it
        if (rq.spec) {                                  // motif unknown here: literal, compact, narrow by contract; mask_stride bytes each
            mask_lo = 0;
            mask_bytes = std::max<uint64_t>(mask_bytes, (uint64_t)(k + 1) * rq.spec_mask_stride);
        } else {
            const uint32_t len = rq.len[k], mp = rq.modpos[k];
            const uint8_t *m = rq.masks + rq.mask_off[k];
            bool literal = true;
            if (check_motif(p, k, len, mp, m, NM_MAX_MOTIF_LEN, &literal)) return p.status;
            if (!literal) p.all_literal = false;
            mask_lo = std::min<uint64_t>(mask_lo, rq.mask_off[k]);
            mask_bytes = std::max<uint64_t>(mask_bytes, (uint64_t)rq.mask_off[k] + len);
            // offsets relative to the modified base span [-mp, len-1-mp] forward and the mirror image in reverse
            const uint32_t reach = std::max(mp, len - 1 - mp);
            if (reach > 95) return plan_fail(p, NM_ERANGE, "candidate %u: a position %u away from the modified base (the engine reaches 95)", k, reach);
            p.any_wide = std::max(p.any_wide, reach > 63 ? 2 : reach > 31 ? 1 : 0);
            if ((m[mp] & 15u) != ((f.slot_is_c >> slot & 1u) ? NM_BASE_C : NM_BASE_A)) p.all_compact = false;
        }
        bucket[(size_t)slot * n_bins + bin + 1] += 1;
        slot_used[slot] = true;
        p.n_prog += 1;
    }
    if (p.n_prog == 0) { mask_lo = 0; mask_bytes = 0; }
    p.mask_lo = mask_lo;
    p.mask_hi = mask_bytes;
    p.n_active = number_active_slots(slot_used, p.slot_to_active, p.active);
    p.per_contig = rq.row_offset != nullptr;
    p.out_rows = p.per_contig ? rq.row_offset[rq.n_cand] : rq.n_cand;
    if (p.per_contig)
        for (uint32_t k = 0; k < rq.n_cand; ++k)
            if (rq.row_offset[k + 1] - rq.row_offset[k] != f.bin_ncontigs[rq.bin[k]])
                return plan_fail(p, NM_EINVAL, "candidate %u: %llu output rows for a bin of %u resident contigs", k,
                                 (unsigned long long)(rq.row_offset[k + 1] - rq.row_offset[k]), f.bin_ncontigs[rq.bin[k]]);
    // the bins the batch has candidates for, their segments, and the (slot, bin) groups.  A heavy batch that is not per-contig walks
    // a work list (nmscore_worklist.h), the one with packed tails unless NM_SCORE_PACK_TAILS=0 (read at every call, like
    // NM_SCORE_CLASSES: same-process A/B, tests/test_gpu_score_tail_pack.py); its segments are cut over list positions
    const char *pack_env = getenv("NM_SCORE_PACK_TAILS");
    const int which = pack_env && atoi(pack_env) == 0 ? 0 : 1;
    size_t list_segs = 0;
    for (uint32_t b = 0; b < n_bins; ++b) {
        uint32_t groups = 0;
        for (uint32_t i = 0; i < p.n_active; ++i) {
            const uint32_t n = bucket[(size_t)p.active[i] * n_bins + b + 1];
            groups += n > 0;
            if ((n + PLAN_PARK_ROWS - 1) / PLAN_PARK_ROWS != (n + PLAN_PASS_ROWS - 1) / PLAN_PASS_ROWS) p.park_fits = false;
        }
        if (!groups) continue;
        p.n_groups += groups;
        bin_active[b] = 1;
        p.n_active_bins += 1;
        p.n_active_segs += (f.bin_nchunks[b] + f.seg_chunks - 1) / f.seg_chunks;
        if (f.list_len[which]) list_segs += (f.list_len[which][b] + f.seg_chunks - 1) / f.seg_chunks;
    }
    p.use_list = f.list_len[which] && !p.per_contig && !(plan_is_light(p) && !f.opt_no_cf);
    p.pack = p.use_list && which == 1;
    if (p.use_list) p.n_active_segs = list_segs;
    return NM_OK;
}

// ---- 2. the batch's shape, decided once.  heavy: one workgroup column per classification (blockIdx.y), candidates VALU-bound;
// light (<= 6 candidates per (slot, bin) group on average — a round of the greedy search, measured crossover, profiles/): HBM-bound,
// groups share their common constraints (CF), two classifications (the usual 6mA + 5mC batch) share one pass over the sequence planes.
inline void plan_shape(ScorePlan &p, const ScoreRequest &rq, const PlanFacts &f) {
    p.lit = p.all_literal && p.all_compact && !p.any_wide && !f.opt_no_lit && !p.per_contig;   // literal-only tiles exist for the narrow compact kernels
    p.np = p.lit ? 4u : 8u;
    p.pdw = 2u * (2u + 2u * (uint32_t)p.any_wide) * p.np;          // dwords per program: [strand][word-group][plane]
    p.light = plan_is_light(p);
    p.cf = p.light && !f.opt_no_cf;
    p.fuse = p.n_active == 2 && p.cf && p.lit;          // (fusing two slots on the 8-plane tile needs 128 VGPRs)
    // IUPAC classes: exactly the batches that launch Variant<1, 1, true, 1, false, false, PC> take the class-plane twin of
    // that variant and the class program layout (the same 32 dwords per program).  NM_SCORE_CLASSES=0, read at every call,
    // keeps them on the 8-plane path (same-process A/B, tests/test_gpu_iupac_classes.py).  NM_SCORE_HEAD=0, read at every
    // call as well, compiles class programs without a head: every walk starts with plain moves and all literals stay in
    // their words (tests/test_gpu_head_pair.py).  NM_SCORE_TAIL, read at every call too, says which tail descriptors the
    // compiler writes: unset both, 0 none (what is left behind the head is walked from the words), 1 the literal descriptors
    // only, 2 the lone-class descriptor only (tests/test_gpu_tail_descriptors.py).  One device build: only programs differ.
    const char *cls_env = getenv("NM_SCORE_CLASSES"), *head_env = getenv("NM_SCORE_HEAD"), *tail_env = getenv("NM_SCORE_TAIL");
    p.cls_head = !(head_env && atoi(head_env) == 0);
    p.cls_tail = tail_env ? atoi(tail_env) & 3 : 3;
    p.classes = !rq.spec && !p.lit && !p.any_wide && p.all_compact && !p.cf && !(cls_env && atoi(cls_env) == 0);
    // A class batch that is not per-contig runs the parked instantiation (nmscan_device.h: Variant::PARK; 28 candidates a pass,
    // 7 waves per SIMD) unless a group would pay for the smaller pass with one more walk over its segments (29 - 32 and 57 - 64
    // candidates).  NM_SCORE_PARK=0, read at every call as well, keeps the batch on the unparked instantiation (same-process
    // A/B, tests/test_gpu_score_park.py).
    const char *park_env = getenv("NM_SCORE_PARK");
    p.park = p.classes && !p.per_contig && p.park_fits && !(park_env && atoi(park_env) == 0);
    // The static segment table covers every bin; a batch whose candidates sit in a few bins only — the long tail of the
    // search: a handful of tasks still open among hundreds of bins — would launch thousands of workgroups that find no
    // candidate range and leave.  Such a batch brings its own table: the segments of the bins it has candidates for.
    const uint32_t static_segments = p.use_list ? f.list_segments[p.pack] : f.n_segments;
    p.own_segments = p.n_prog && p.n_active_segs * 4 <= (size_t)static_segments * 3 && getenv("NM_ALL_SEGMENTS") == nullptr;
    p.n_segments = p.own_segments ? (uint32_t)p.n_active_segs : static_segments;
    p.n_entries = std::max(p.n_active, 1u) * f.n_bins;
    // a light batch appends one common program per (slot, bin) entry
    p.prog_dw = ((size_t)std::max(p.n_prog, 1u) + (p.cf ? p.n_entries : 0)) * p.pdw;
    // host counts come back through the pinned half of the staging pair (a copy into pageable memory is staged by the
    // runtime and costs tens of microseconds more per round of the search); tables too large for that go directly
    p.out_bytes = (size_t)p.out_rows * 2 * sizeof(int64_t);
    p.via_stage = rq.defer || (rq.h_out && p.out_bytes <= PLAN_STAGE_DIRECT_MAX);
    // a call that returns host counts has nothing to overlap the compile with (the caller waits for this very batch):
    // it prepares on the scoring stream itself — no event, no cross-stream wait in its chain of launch latencies
    p.inline_prep = (rq.h_out || rq.defer) && !f.opt_no_inline;
    if (rq.spec) p.compile = PLAN_COMPILE_SPEC;         // the writer compiles what it wrote
    else if (!p.n_prog) p.compile = PLAN_COMPILE_NONE;
    else if (p.cf && p.n_prog <= 2048 && p.n_entries <= 8192 && !f.opt_no_inline) p.compile = PLAN_COMPILE_FUSED;   // compile_common_kernel
    else p.compile = p.cf ? PLAN_COMPILE_THEN_COMMON : PLAN_COMPILE_ONLY;      // compile_kernel (+ common_kernel)
}

// ---- 3. the staging pair: candidate records (sorted) | orig_index | mask bytes | cand_range | row bases (per-contig) | own
// segment table | spec: sorted position of candidate k, the writer's extra input || counts | spec: the writer's extra output
inline void plan_layout(ScorePlan &p, const ScoreRequest &rq) {
    const size_t rec_bytes = (size_t)p.n_prog * sizeof(CandRec);
    p.off_orig = plan_align16(rec_bytes);
    p.off_masks = plan_align16(p.off_orig + (size_t)p.n_prog * 4);
    p.off_range = plan_align16(p.off_masks + (p.mask_hi - p.mask_lo));
    p.range_bytes = (size_t)p.n_entries * sizeof(PlanU4);
    p.off_rows = plan_align16(p.off_range + p.range_bytes);
    const size_t rows_end = p.off_rows + (p.per_contig ? (size_t)p.n_prog * 8 : 0);
    p.off_segs = plan_align16(rows_end);
    const size_t segs_end = p.own_segments ? p.off_segs + p.n_active_segs * sizeof(PlanU4) : p.off_segs;
    p.off_posof = plan_align16(segs_end);
    p.off_xin = plan_align16(p.off_posof + (size_t)rq.n_cand * 4);
    p.total = rq.spec ? p.off_xin + rq.spec_extra_in : p.own_segments ? segs_end : rows_end;
    p.off_counts = plan_align16(p.total);
    p.off_xout = plan_align16(p.off_counts + p.out_bytes);
    p.stage_end = rq.spec ? p.off_xout + rq.spec_extra_out : p.off_counts + p.out_bytes;
    p.clear_bytes = rq.spec ? p.stage_end - p.off_counts : (size_t)p.out_rows * 2 * sizeof(unsigned long long);
    // a batch somebody waits for (a round of the search): tables in, outputs cleared, results out by KERNELS on its own stream — no
    // copy engine in the chain (nmscan_internal.h: stage_in); everything else keeps the copy engines
    p.by_kernels = p.inline_prep && p.total <= PLAN_STAGE_DIRECT_MAX && (p.via_stage || !rq.h_out) && getenv("NM_STAGE_COPIES") == nullptr;
}

// ---- 4. the tables, written at those offsets into the host half `hs` (at least p.total bytes).  The bucket counts become the
// exclusive prefix -> first sorted index of each (slot, bin); the sort is stable within a bucket.
inline void plan_fill(const ScorePlan &p, const ScoreRequest &rq, const PlanFacts &f, uint32_t *bucket, const uint8_t *bin_active, uint8_t *hs) {
    const uint32_t n_bins = f.n_bins;
    CandRec *h_rec = reinterpret_cast<CandRec *>(hs);
    uint32_t *h_orig = reinterpret_cast<uint32_t *>(hs + p.off_orig);
    PlanU4 *h_range = reinterpret_cast<PlanU4 *>(hs + p.off_range);
    if (!rq.spec && p.mask_hi > p.mask_lo) memcpy(hs + p.off_masks, rq.masks + p.mask_lo, p.mask_hi - p.mask_lo);
    memset(h_range, 0, p.range_bytes);
    if (p.own_segments) {
        PlanU4 *h_segs = reinterpret_cast<PlanU4 *>(hs + p.off_segs);
        const uint32_t *first = p.use_list ? f.list_start[p.pack] : f.bin_chunk0, *count = p.use_list ? f.list_len[p.pack] : f.bin_nchunks;
        size_t at = 0;
        for (uint32_t b = 0; b < n_bins; ++b)
            if (bin_active[b])
                for (uint32_t k = 0; k < count[b]; k += f.seg_chunks)
                    h_segs[at++] = PlanU4{first[b] + k, std::min<uint32_t>(f.seg_chunks, count[b] - k), b, 0};
    }
    const size_t n_bucket = (size_t)NM_MAX_MOD_SLOTS * n_bins + 1;
    for (size_t i = 1; i < n_bucket; ++i) bucket[i] += bucket[i - 1];
    for (uint32_t i = 0; i < p.n_active; ++i)
        for (uint32_t b = 0; b < n_bins; ++b) {
            const uint32_t lo = bucket[(size_t)p.active[i] * n_bins + b], hi = bucket[(size_t)p.active[i] * n_bins + b + 1];
            if (hi > lo) h_range[(size_t)i * n_bins + b] = PlanU4{lo, hi - lo, 0xFFFFFFFFu, 0};
        }
    for (uint32_t k = 0; k < rq.n_cand; ++k) {
        const uint32_t slot = rq.slot[k], bin = rq.bin[k];
        if (f.bin_nchunks[bin] == 0) continue;
        const uint32_t at = bucket[(size_t)slot * n_bins + bin]++;
        h_orig[at] = k;
        if (rq.spec) {
            h_rec[at] = CandRec{k * rq.spec_mask_stride, k, 0, 0, (uint8_t)slot, 0};
            reinterpret_cast<uint32_t *>(hs + p.off_posof)[k] = at;
            continue;
        }
        h_rec[at] = CandRec{(uint32_t)(rq.mask_off[k] - p.mask_lo), k, rq.len[k], rq.modpos[k], (uint8_t)slot, 0};
        if (p.per_contig) reinterpret_cast<uint64_t *>(hs + p.off_rows)[at] = rq.row_offset[k];
    }
}

// ---- 5. the grid.  Workgroups that will find candidates, against what the device runs at once (6 per CU, 7 of the parked class kernel): below ~2 rounds of
// workgroups the last, partly filled round is a large share of the launch -> smaller pieces.  The grid is runs of pieces (8 for
// the XCD-remapped heavy variants, 1 for the streaming ones); in every run the pieces a full round of resident workgroups would
// take LAST are cut finer (down to 4 chunks = one per wave).  score_kernel (nmscan_device.h) decodes blockIdx.x accordingly.
inline void plan_geometry(ScorePlan &p, const PlanFacts &f) {
    uint64_t est_wgs = (uint64_t)p.n_segments * p.n_groups / std::max<uint32_t>(p.own_segments ? p.n_active_bins : f.n_bins, 1);
    if (p.light && p.n_active == 2 && p.lit) est_wgs = (est_wgs + 1) / 2;   // fused slots: one workgroup serves both
    const uint64_t resident = (uint64_t)f.n_cus * (p.park ? PLAN_RESIDENT_PER_CU_PARKED : PLAN_RESIDENT_PER_CU);
    uint32_t split_log2 = 0;
    while (split_log2 < 2 && (est_wgs << split_log2) < 2 * resident) ++split_log2;      // measured: halves win below ~2 rounds, quarters never
    if (f.opt_split >= 0) split_log2 = (uint32_t)f.opt_split;
    p.split_log2 = split_log2;
    const uint32_t runs = p.cf ? 1u : 8u;
    const uint32_t n_pieces = p.n_segments << split_log2;
    p.pieces_per_run = (n_pieces + runs - 1) / runs;
    p.fine_log2 = f.opt_fine >= 0 ? (uint32_t)f.opt_fine : 2u - split_log2;
    p.gy = p.fuse ? 1u : std::max(p.n_active, 1u);
    uint32_t tail_pieces = (uint32_t)std::min<uint64_t>(p.pieces_per_run, (resident / p.gy + runs - 1) / runs);
    if (p.fine_log2 == 0) tail_pieces = 0;
    p.j_big = p.pieces_per_run - tail_pieces;
    p.gx = (p.j_big + (tail_pieces << p.fine_log2)) * runs;
    p.last_wgs = (uint64_t)p.gx * p.gy;
}

}  // namespace nmdetail
