// Stand-alone check of the scoring plan (nanomotif_amd/csrc/nmscore_plan.h) on the CPU: random and directed batches, every
// plan compared with a plain restatement written here, the work lists of the heavy kernels (nmscore_worklist.h) included: the grid
// of every planned batch reaches every strip of sequence of every active bin exactly once.  Build: g++ -O2 -std=c++17 driver.cpp -o plan_check; run: ./plan_check [seed]
// (./plan_check park: the cases of the parked class kernel alone, one line per planned batch — tests/test_score_park_host.py)
// (tests/test_score_plan_host.py does both, a second time with -fsanitize=address,undefined where that links).
#include <cinttypes>
#include <cstdarg>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../nanomotif_amd/csrc/nmscore_plan.h"
#include "../../nanomotif_amd/csrc/nmscore_worklist.h"

using namespace nmdetail;

namespace {

std::mt19937_64 rng;
uint32_t rnd(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % ((uint64_t)hi - lo + 1)); }      // inclusive
bool chance(double p) { return (rng() >> 11) * (1.0 / 9007199254740992.0) < p; }

long g_checks = 0, g_cases = 0, g_rejected = 0;
std::string g_case;
[[noreturn]] void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "plan_check FAILED in case '%s': ", g_case.c_str());
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) die(__VA_ARGS__); } while (0)

struct World {                                          // an uploaded assembly as the plan sees it
    std::vector<uint32_t> nchunks, chunk0, ncontigs;
    std::vector<PlanU4> static_segs;
    uint32_t n_chunks = 0;
    PlanFacts f;
    // the contigs behind the chunks and the work lists built from them (nmscore_worklist.h); lists = false: an engine without lists
    std::vector<uint32_t> contig_bin, contig_chunk;
    std::vector<uint64_t> contig_len;
    WorkList wl[2];
    bool lists = true;
};

// a contig of exactly `chunks` chunks (its 96 bp of gap included)
uint64_t contig_of_chunks(uint32_t chunks) {
    const uint64_t hi = (uint64_t)chunks * 8192 - 96, lo = chunks > 1 ? hi - 8191 : 1;
    return chance(0.15) ? hi : chance(0.15) ? (hi / 8192) * 8192 + (chunks > 1 || hi >= 8192 ? 0 : 1) : lo + rng() % (hi - lo + 1);
}

void add_contig(World &w, uint32_t bin, uint64_t len, uint32_t chunk) {
    w.contig_bin.push_back(bin);
    w.contig_len.push_back(len);
    w.contig_chunk.push_back(chunk);
}

// needs_v as the geometry alone decides it (no N in the sequence): a contig's first chunk, and every chunk whose own positions or
// the 96 behind it are not all inside the contig
void build_lists(World &w) {
    std::vector<uint8_t> needs_v(w.n_chunks, 1);
    for (size_t i = 0; i < w.contig_len.size(); ++i)
        for (uint64_t q = 1; (q + 1) * 8192 + 96 <= w.contig_len[i]; ++q) needs_v[w.contig_chunk[i] + q] = 0;
    std::vector<uint32_t> order(w.contig_bin.size());
    std::iota(order.begin(), order.end(), 0u);          // (the worlds are made bin by bin)
    for (int pack = 0; pack < 2; ++pack)
        build_work_list(w.wl[pack], pack == 1, w.f.n_bins, (uint32_t)order.size(), order.data(), w.contig_bin.data(), w.contig_len.data(), w.contig_chunk.data(),
                        needs_v.data(), w.n_chunks, w.f.seg_chunks);
}

World make_world(uint32_t n_bins, uint32_t max_chunks, uint32_t n_slots, double resident = 0.85, int fixed_chunks = -1) {
    World w;
    w.nchunks.resize(n_bins);
    w.chunk0.assign(n_bins, 0);
    w.ncontigs.assign(n_bins, 0);
    w.f.seg_chunks = chance(0.8) ? 16 : rnd(4, 24);
    uint32_t next = 1;                                  // chunk 0 and the last chunk are pads (nm_upload_contigs)
    for (uint32_t b = 0; b < n_bins; ++b) {
        w.nchunks[b] = fixed_chunks >= 0 ? (uint32_t)fixed_chunks : chance(resident) ? rnd(1, max_chunks) : 0;
        if (!w.nchunks[b]) continue;
        w.chunk0[b] = next;
        w.ncontigs[b] = rnd(1, std::min(4u, w.nchunks[b]));
        for (uint32_t k = 0, left = w.nchunks[b], at = next; k < w.ncontigs[b]; ++k) {        // the bin's chunks dealt to its contigs
            const uint32_t mine = k + 1 == w.ncontigs[b] ? left : rnd(1, left - (w.ncontigs[b] - 1 - k));
            add_contig(w, b, contig_of_chunks(mine), at);
            at += mine;
            left -= mine;
        }
        for (uint32_t k = 0; k < w.nchunks[b]; k += w.f.seg_chunks)
            w.static_segs.push_back(PlanU4{next + k, std::min(w.f.seg_chunks, w.nchunks[b] - k), b, 0});
        next += w.nchunks[b];
    }
    w.n_chunks = next + 1;
    w.f.n_bins = n_bins;
    w.f.n_segments = (uint32_t)w.static_segs.size();
    for (uint32_t s = 0; s < n_slots; ++s) {
        w.f.slot_present |= 1u << s;
        if (chance(0.5)) w.f.slot_is_c |= 1u << s;
    }
    w.f.n_cus = chance(0.7) ? 256 : rnd(1, 304);
    build_lists(w);
    return w;
}

// bins given contig by contig: lengths[b] = the contigs of bin b
World make_world_of(const std::vector<std::vector<uint64_t>> &lengths, uint32_t seg_chunks, uint32_t n_slots) {
    World w;
    const uint32_t n_bins = (uint32_t)lengths.size();
    w.nchunks.assign(n_bins, 0);
    w.chunk0.assign(n_bins, 0);
    w.ncontigs.assign(n_bins, 0);
    w.f.seg_chunks = seg_chunks;
    uint32_t next = 1;
    for (uint32_t b = 0; b < n_bins; ++b) {
        if (!lengths[b].empty()) w.chunk0[b] = next;
        for (uint64_t len : lengths[b]) {
            const uint32_t nch = (uint32_t)((len + 96 + 8191) / 8192);
            add_contig(w, b, len, next);
            next += nch;
            w.nchunks[b] += nch;
            w.ncontigs[b] += 1;
        }
        for (uint32_t k = 0; k < w.nchunks[b]; k += seg_chunks) w.static_segs.push_back(PlanU4{w.chunk0[b] + k, std::min(seg_chunks, w.nchunks[b] - k), b, 0});
    }
    w.n_chunks = next + 1;
    w.f.n_bins = n_bins;
    w.f.n_segments = (uint32_t)w.static_segs.size();
    for (uint32_t s = 0; s < n_slots; ++s) w.f.slot_present |= 1u << s;
    build_lists(w);
    return w;
}

void bind(World &w) {                                   // (the vectors may have moved)
    w.f.bin_nchunks = w.nchunks.data();
    w.f.bin_chunk0 = w.chunk0.data();
    w.f.bin_ncontigs = w.ncontigs.data();
    for (int pack = 0; pack < 2; ++pack) {
        w.f.list_start[pack] = w.lists ? w.wl[pack].bin_start.data() : nullptr;
        w.f.list_len[pack] = w.lists ? w.wl[pack].bin_len.data() : nullptr;
        w.f.list_segments[pack] = w.lists ? (uint32_t)w.wl[pack].segs.size() : 0;
    }
}

struct Batch {
    std::vector<uint32_t> bin, off;
    std::vector<uint8_t> slot, len, mp, masks;
    std::vector<uint64_t> rows;                         // per-contig batches only
    bool per_contig = false, defer = false, host_out = true, spec = false;
    uint32_t stride = 64;
    size_t extra_in = 0, extra_out = 0;
    size_t size() const { return bin.size(); }
};

// kind: 0 literal, 1 with 2-sets, 2 with 3-sets, 3 an empty set, 4 all-N; reach_len: 0 = short, else the reach to sit at
void add_motif(Batch &b, const World &w, uint32_t bin, uint32_t slot, int kind, uint32_t reach = 0, bool compact = true) {
    uint32_t len, mp;
    if (reach) {                                        // a position exactly `reach` from the modified base
        mp = chance(0.5) ? reach : rnd(0, std::min(reach, 254u - reach));
        len = mp == reach ? reach + 1 + rnd(0, std::min(reach, 254u - reach)) : mp + reach + 1;
    } else {
        len = rnd(1, 14);
        mp = rnd(0, len - 1);
    }
    std::vector<uint8_t> m(len, 15);
    const uint8_t can = (w.f.slot_is_c >> (slot & 7) & 1u) ? NM_BASE_C : NM_BASE_A;
    static const uint8_t lits[4] = {1, 2, 4, 8}, two[6] = {3, 5, 6, 9, 10, 12}, three[4] = {7, 11, 13, 14};
    if (kind != 4) {
        for (uint32_t j = 0; j < len; ++j)
            if (chance(len > 20 ? 0.08 : 0.5)) m[j] = lits[rnd(0, 3)];
        m[0] = lits[rnd(0, 3)];                         // both ends specified: the reach is what was asked for
        m[len - 1] = lits[rnd(0, 3)];
        m[mp] = compact ? can : (uint8_t)(can == NM_BASE_A ? NM_BASE_G : NM_BASE_T);
        const uint32_t at = rnd(0, len - 1);            // (a set on the modified base would undo `compact`: such a motif stays literal)
        if (kind == 1 && at != mp) m[at] = two[rnd(0, 5)];
        if (kind == 2 && at != mp) m[at] = three[rnd(0, 3)];
        if (kind == 3) m[at] = 0;
    }
    if (chance(0.2)) for (auto &v : m) v |= (uint8_t)(rnd(0, 15) << 4);      // the high nibble is not part of a set
    if (chance(0.1)) b.masks.insert(b.masks.end(), rnd(1, 9), 0);            // unreferenced bytes between motifs
    b.bin.push_back(bin);
    b.slot.push_back((uint8_t)slot);
    b.len.push_back((uint8_t)len);
    b.mp.push_back((uint8_t)mp);
    b.off.push_back((uint32_t)b.masks.size());
    b.masks.insert(b.masks.end(), m.begin(), m.end());
}

void add_rows(Batch &b, const World &w) {
    b.per_contig = true;
    b.rows.assign(b.size() + 1, 0);
    for (size_t k = 0; k < b.size(); ++k) b.rows[k + 1] = b.rows[k] + (b.bin[k] < w.f.n_bins ? w.ncontigs[b.bin[k]] : 0);
}

ScoreRequest request_of(const Batch &b) {
    static int64_t host_sink;
    static const int spec_tag = 0;
    ScoreRequest rq;
    rq.n_cand = (uint32_t)b.size();
    rq.bin = b.bin.data();
    rq.slot = b.slot.data();
    if (!b.spec) { rq.len = b.len.data(); rq.modpos = b.mp.data(); rq.mask_off = b.off.data(); rq.masks = b.masks.data(); }
    if (b.per_contig) rq.row_offset = b.rows.data();
    rq.defer = b.defer;
    rq.h_out = b.host_out && !b.defer && !b.spec ? &host_sink : nullptr;
    if (b.spec) {
        rq.spec = reinterpret_cast<const SpecSource *>(&spec_tag);           // (opaque to the plan)
        rq.spec_mask_stride = b.stride;
        rq.spec_extra_in = b.extra_in;
        rq.spec_extra_out = b.extra_out;
        rq.defer = true;
    }
    return rq;
}

// the answer of the validation, candidate by candidate: {status, candidate}
std::pair<int, uint32_t> brute_validate(const Batch &b, const World &w) {
    for (uint32_t k = 0; k < b.size(); ++k) {
        if (b.slot[k] >= NM_MAX_MOD_SLOTS || !(w.f.slot_present >> b.slot[k] & 1u)) return {NM_ESTATE, k};
        if (b.bin[k] >= w.f.n_bins) return {NM_EINVAL, k};
        if (w.nchunks[b.bin[k]] == 0 || b.spec) continue;
        const int len = b.len[k], mp = b.mp[k];
        if (len < 1 || len > NM_MAX_MOTIF_LEN) return {NM_ERANGE, k};
        if (mp >= len) return {NM_EINVAL, k};
        bool specified = false;
        for (int j = 0; j < len; ++j) {
            if ((b.masks[b.off[k] + j] & 15) == 0) return {NM_EINVAL, k};
            specified |= (b.masks[b.off[k] + j] & 15) != 15;
        }
        if (!specified) return {NM_EINVAL, k};
        if (mp > 95 || len - 1 - mp > 95) return {NM_ERANGE, k};
    }
    if (b.per_contig)
        for (uint32_t k = 0; k < b.size(); ++k)
            if (b.rows[k + 1] - b.rows[k] != w.ncontigs[b.bin[k]]) return {NM_EINVAL, k};
    return {NM_OK, 0};
}

// One workgroup's piece of the table: plan_decode_block (nmscore_plan.h), composed of the two functions score_kernel calls.
bool decode_block(const ScorePlan &p, bool cf, uint32_t block, const PlanU4 *segments, uint32_t *first, uint32_t *count) {
    const PlanGrid g{p.n_segments, p.split_log2, p.pieces_per_run, p.j_big, p.fine_log2};
    uint32_t seg = 0;
    return plan_decode_block(g, cf, block, segments, &seg, first, count);
}

std::vector<uint32_t> g_bucket;
std::vector<uint8_t> g_bin_active, g_stage, g_visits;

bool env_zero(const char *name) { const char *e = getenv(name); return e && atoi(e) == 0; }

// plan the batch as score_impl does and compare every step with its restatement; returns the plan
ScorePlan run_case(const char *name, World &w, const Batch &b) {
    g_case = name;
    ++g_cases;
    bind(w);
    const PlanFacts &f = w.f;
    const ScoreRequest rq = request_of(b);
    const uint32_t n_bins = f.n_bins, n = rq.n_cand;
    g_bucket.assign((size_t)NM_MAX_MOD_SLOTS * n_bins + 1, 0);
    g_bin_active.assign(n_bins, 0);
    ScorePlan p;
    const int rc = plan_classify(p, rq, f, g_bucket.data(), g_bin_active.data());
    // ---- validation
    const auto want = brute_validate(b, w);
    CHECK(rc == want.first && p.status == rc, "status %d (%s), the brute force says %d at candidate %u", rc, p.err, want.first, want.second);
    if (rc != NM_OK) {
        unsigned k = ~0u;
        CHECK(sscanf(p.err, "candidate %u", &k) == 1 && k == want.second, "message '%s' names another candidate than %u", p.err, want.second);
        ++g_rejected;
        return p;
    }
    // ---- the batch's class
    std::vector<uint32_t> order;                        // resident candidates, stable by (slot, bin)
    for (uint32_t k = 0; k < n; ++k) if (w.nchunks[b.bin[k]]) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return b.slot[x] != b.slot[y] ? b.slot[x] < b.slot[y] : b.bin[x] < b.bin[y]; });
    int wide = 0;
    bool compact = true, literal = true, slot_used[NM_MAX_MOD_SLOTS] = {};
    std::vector<uint8_t> bin_used(n_bins, 0);
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t k : order) {
        slot_used[b.slot[k]] = true;
        bin_used[b.bin[k]] = 1;
        if (b.spec) { lo = 0; hi = std::max<uint64_t>(hi, (uint64_t)(k + 1) * b.stride); continue; }
        const int reach = std::max<int>(b.mp[k], b.len[k] - 1 - b.mp[k]);
        wide = std::max(wide, reach >= 64 ? 2 : reach >= 32 ? 1 : 0);
        for (int j = 0; j < b.len[k]; ++j) {
            const int v = b.masks[b.off[k] + j] & 15, bits = __builtin_popcount(v);
            if (bits == 2 || bits == 3) literal = false;
        }
        if ((b.masks[b.off[k] + b.mp[k]] & 15) != ((f.slot_is_c >> b.slot[k] & 1u) ? NM_BASE_C : NM_BASE_A)) compact = false;
        lo = std::min<uint64_t>(lo, b.off[k]);
        hi = std::max<uint64_t>(hi, (uint64_t)b.off[k] + b.len[k]);
    }
    if (order.empty()) lo = hi = 0;
    CHECK(p.n_prog == order.size(), "n_prog %u, %zu candidates are resident", p.n_prog, order.size());
    CHECK(p.any_wide == wide && p.all_compact == compact && p.all_literal == literal, "class (wide %d compact %d literal %d), expected (%d %d %d)",
          p.any_wide, p.all_compact, p.all_literal, wide, compact, literal);
    CHECK(p.mask_lo == lo && p.mask_hi == hi, "mask bytes [%" PRIu64 ", %" PRIu64 "), expected [%" PRIu64 ", %" PRIu64 ")", p.mask_lo, p.mask_hi, lo, hi);
    uint32_t n_active = 0, n_act_bins = 0, n_groups = 0;
    size_t n_act_segs = 0, n_act_list_segs = 0;
    const int pack = env_zero("NM_SCORE_PACK_TAILS") ? 0 : 1;
    const WorkList &wl = w.wl[pack];
    for (int s = 0; s < NM_MAX_MOD_SLOTS; ++s) {
        CHECK(p.slot_to_active[s] == (slot_used[s] ? (int)n_active : -1), "slot %d numbered %d", s, p.slot_to_active[s]);
        if (slot_used[s]) { CHECK(p.active[n_active] == (uint32_t)s, "active[%u] = %u, expected %d", n_active, p.active[n_active], s); ++n_active; }
    }
    for (uint32_t bb = 0; bb < n_bins; ++bb) {
        CHECK(g_bin_active[bb] == bin_used[bb], "bin %u active %d, expected %d", bb, g_bin_active[bb], bin_used[bb]);
        if (bin_used[bb]) { ++n_act_bins; n_act_segs += (w.nchunks[bb] + f.seg_chunks - 1) / f.seg_chunks; }
        if (bin_used[bb] && w.lists) n_act_list_segs += (wl.bin_len[bb] + f.seg_chunks - 1) / f.seg_chunks;
    }
    // the park rule: no (slot, bin) group takes more passes of 28 candidates than of 32 (sizes 29 - 32 and 57 - 64 do)
    bool park_fits = true;
    for (size_t i = 0, from = 0; i < order.size(); ++i) {
        if (i == 0 || b.slot[order[i]] != b.slot[order[i - 1]] || b.bin[order[i]] != b.bin[order[i - 1]]) { ++n_groups; from = i; }
        if (i + 1 == order.size() || b.slot[order[i + 1]] != b.slot[order[i]] || b.bin[order[i + 1]] != b.bin[order[i]]) {
            const size_t size = i + 1 - from;
            if ((size + 27) / 28 != (size + 31) / 32) park_fits = false;
        }
    }
    CHECK(p.park_fits == park_fits, "park_fits %d, the group sizes say %d", p.park_fits, park_fits);
    // a heavy batch that is not per-contig walks the work list: its segments are counted over list positions
    const bool use_list = w.lists && !b.per_contig && !(order.size() <= 6 * (size_t)n_groups && !f.opt_no_cf);
    CHECK(p.use_list == use_list && p.pack == (use_list && pack == 1), "use_list %d pack %d, expected %d %d", p.use_list, p.pack, use_list, use_list && pack == 1);
    if (use_list) n_act_segs = n_act_list_segs;
    const size_t n_static = use_list ? wl.segs.size() : f.n_segments;
    CHECK(p.n_active == n_active && p.n_active_bins == n_act_bins && p.n_active_segs == n_act_segs && p.n_groups == n_groups,
          "active slots %u bins %u segments %zu groups %u, expected %u %u %zu %u", p.n_active, p.n_active_bins, p.n_active_segs, p.n_groups, n_active,
          n_act_bins, n_act_segs, n_groups);
    CHECK(p.out_rows == (b.per_contig ? b.rows[n] : n), "out_rows %" PRIu64, p.out_rows);
    // ---- shape
    plan_shape(p, rq, f);
    const bool lit = literal && compact && !wide && !f.opt_no_lit && !b.per_contig;
    const bool light = !b.per_contig && order.size() <= 6 * (size_t)n_groups, cf = light && !f.opt_no_cf;
    const bool classes = !b.spec && !lit && !wide && compact && !cf && !env_zero("NM_SCORE_CLASSES");
    const bool own = !order.empty() && 4 * n_act_segs <= 3 * n_static && !getenv("NM_ALL_SEGMENTS");
    const uint32_t n_entries = std::max(n_active, 1u) * n_bins, np = lit ? 4 : 8, pdw = np * (wide == 0 ? 4 : wide == 1 ? 8 : 12);
    CHECK(p.lit == lit && p.light == light && p.cf == cf && p.classes == classes && p.fuse == (n_active == 2 && cf && lit) && p.own_segments == own,
          "shape lit %d light %d cf %d classes %d fuse %d own %d, expected %d %d %d %d %d %d", p.lit, p.light, p.cf, p.classes, p.fuse, p.own_segments, lit,
          light, cf, classes, n_active == 2 && cf && lit, own);
    const bool park = classes && !b.per_contig && park_fits && !env_zero("NM_SCORE_PARK");
    CHECK(p.park == park, "park %d, expected %d (classes %d per-contig %d fits %d)", p.park, park, classes, b.per_contig, park_fits);
    CHECK(p.cls_head == !env_zero("NM_SCORE_HEAD"), "cls_head %d", p.cls_head);
    const char *tail = getenv("NM_SCORE_TAIL");                                      // unset: both kinds of tail descriptor; 0, 1, 2
    CHECK(p.cls_tail == (tail ? tail[0] - '0' : 3), "cls_tail %d", p.cls_tail);
    CHECK(p.np == np && p.pdw == pdw && p.n_entries == n_entries, "np %u pdw %u entries %u, expected %u %u %u", p.np, p.pdw, p.n_entries, np, pdw, n_entries);
    CHECK(p.prog_dw == (std::max<size_t>(order.size(), 1) + (cf ? n_entries : 0)) * pdw, "program room %zu dwords", p.prog_dw);
    const PlanCompile compile = b.spec ? PLAN_COMPILE_SPEC : order.empty() ? PLAN_COMPILE_NONE
                                : !cf ? PLAN_COMPILE_ONLY
                                : order.size() <= 2048 && n_entries <= 8192 && !f.opt_no_inline ? PLAN_COMPILE_FUSED : PLAN_COMPILE_THEN_COMMON;
    CHECK(p.compile == compile, "compile path %d, expected %d", p.compile, compile);
    const size_t out_bytes = (size_t)p.out_rows * 16;
    CHECK(p.via_stage == (rq.defer || (rq.h_out && out_bytes <= ((size_t)4 << 20))), "via_stage %d for %zu count bytes", p.via_stage, out_bytes);
    CHECK(p.inline_prep == ((rq.h_out || rq.defer) && !f.opt_no_inline), "inline_prep %d", p.inline_prep);
    // ---- layout: regions 16-byte aligned, in order, disjoint, ending at the total
    plan_layout(p, rq);
    struct Region { const char *what; size_t at, bytes; };
    std::vector<Region> regions = {{"records", 0, order.size() * sizeof(CandRec)}, {"orig_index", p.off_orig, order.size() * 4},
                                   {"masks", p.off_masks, (size_t)(hi - lo)}, {"ranges", p.off_range, (size_t)n_entries * 16}};
    if (b.per_contig) regions.push_back({"row bases", p.off_rows, order.size() * 8});
    if (own) regions.push_back({"segments", p.off_segs, n_act_segs * 16});
    if (b.spec) { regions.push_back({"pos_of", p.off_posof, (size_t)n * 4}); regions.push_back({"extra in", p.off_xin, b.extra_in}); }
    size_t end = 0;
    for (const Region &r : regions) {
        CHECK(r.at % 16 == 0 && r.at >= end && r.at < end + 16, "%s at %zu: the region before it ends at %zu", r.what, r.at, end);
        end = r.at + r.bytes;
    }
    CHECK(p.total == end, "total %zu, the last region ends at %zu", p.total, end);
    CHECK(p.range_bytes == (size_t)n_entries * 16 && p.out_bytes == out_bytes, "range bytes %zu, count bytes %zu", p.range_bytes, p.out_bytes);
    CHECK(p.off_counts % 16 == 0 && p.off_counts >= p.total && p.off_counts < p.total + 16, "counts at %zu behind a total of %zu", p.off_counts, p.total);
    if (b.spec) {
        CHECK(p.off_xout % 16 == 0 && p.off_xout >= p.off_counts + out_bytes && p.off_xout < p.off_counts + out_bytes + 16, "extra out at %zu", p.off_xout);
        CHECK(p.stage_end == p.off_xout + b.extra_out && p.clear_bytes == p.stage_end - p.off_counts, "stage end %zu, clear %zu", p.stage_end, p.clear_bytes);
    } else CHECK(p.stage_end == p.off_counts + out_bytes && p.clear_bytes == out_bytes, "stage end %zu, clear %zu", p.stage_end, p.clear_bytes);
    CHECK(p.by_kernels == (p.inline_prep && p.total <= ((size_t)4 << 20) && (p.via_stage || !rq.h_out) && !getenv("NM_STAGE_COPIES")),
          "by_kernels %d for %zu staged bytes", p.by_kernels, p.total);
    // ---- fill
    g_stage.assign(p.total + 16, 0xA5);
    uint8_t *hs = g_stage.data();
    plan_fill(p, rq, f, g_bucket.data(), g_bin_active.data(), hs);
    for (size_t i = 0; i < 16; ++i) CHECK(hs[p.total + i] == 0xA5, "fill wrote behind the total (%zu + %zu)", p.total, i);
    const CandRec *rec = reinterpret_cast<const CandRec *>(hs);
    const uint32_t *orig = reinterpret_cast<const uint32_t *>(hs + p.off_orig);
    for (size_t i = 0; i < order.size(); ++i) {
        const uint32_t k = order[i];
        CHECK(rec[i].orig == k && orig[i] == k && rec[i].slot == b.slot[k], "sorted position %zu holds candidate %u, the stable sort puts %u there", i, rec[i].orig, k);
        if (b.spec) {
            CHECK(rec[i].mask_off == k * b.stride && reinterpret_cast<const uint32_t *>(hs + p.off_posof)[k] == i, "spec record %zu", i);
            continue;
        }
        CHECK(rec[i].len == b.len[k] && rec[i].modpos == b.mp[k], "record %zu: len %u modpos %u", i, rec[i].len, rec[i].modpos);
        CHECK((uint64_t)rec[i].mask_off + b.len[k] <= hi - lo && memcmp(hs + p.off_masks + rec[i].mask_off, b.masks.data() + b.off[k], b.len[k]) == 0,
              "record %zu: its staged mask bytes are not the candidate's", i);
        if (b.per_contig) CHECK(reinterpret_cast<const uint64_t *>(hs + p.off_rows)[i] == b.rows[k], "row base of sorted candidate %zu", i);
    }
    const PlanU4 *range = reinterpret_cast<const PlanU4 *>(hs + p.off_range);
    {
        size_t at = 0;
        for (uint32_t a = 0; a < std::max(n_active, 1u); ++a)
            for (uint32_t bb = 0; bb < n_bins; ++bb) {
                size_t cnt = 0;
                while (n_active && at + cnt < order.size() && b.slot[order[at + cnt]] == p.active[a] && b.bin[order[at + cnt]] == bb) ++cnt;
                const PlanU4 &r = range[(size_t)a * n_bins + bb];
                if (cnt) CHECK(r.x == at && r.y == cnt && r.z == 0xFFFFFFFFu && r.w == 0, "range (%u, %u) = {%u, %u, %u, %u}, the sort has %zu from %zu", a, bb, r.x, r.y, r.z, r.w, cnt, at);
                else CHECK(r.x == 0 && r.y == 0 && r.z == 0 && r.w == 0, "range (%u, %u) of an empty group is not zero", a, bb);
                at += cnt;
            }
        CHECK(at == order.size(), "the ranges hold %zu candidates of %zu", at, order.size());
    }
    // ---- the table the launch walks, over chunks or over the positions of the work list: the batch's own holds exactly the
    // entries of the active bins
    const PlanU4 *segments = own ? reinterpret_cast<const PlanU4 *>(hs + p.off_segs) : use_list ? wl.segs.data() : w.static_segs.data();
    CHECK(p.n_segments == (own ? n_act_segs : n_static), "n_segments %u", p.n_segments);
    const uint32_t *first_of = use_list ? wl.bin_start.data() : w.chunk0.data(), *count_of = use_list ? wl.bin_len.data() : w.nchunks.data();
    const size_t n_items = use_list ? wl.entries.size() : w.n_chunks;
    g_visits.assign(n_items, 0);
    std::vector<uint8_t> in_table(n_items, 0);
    for (uint32_t s = 0; s < p.n_segments; ++s) {
        const PlanU4 &sg = segments[s];
        CHECK(sg.y >= 1 && sg.y <= f.seg_chunks && sg.z < n_bins && sg.x >= first_of[sg.z] && sg.x + sg.y <= first_of[sg.z] + count_of[sg.z],
              "segment %u = {%u, %u, %u} leaves its bin", s, sg.x, sg.y, sg.z);
        for (uint32_t c = 0; c < sg.y; ++c) { CHECK(!in_table[sg.x + c], "item %u is in two segments", sg.x + c); in_table[sg.x + c] = 1; }
    }
    for (uint32_t bb = 0; bb < n_bins; ++bb)
        for (uint32_t c = 0; c < count_of[bb]; ++c)
            CHECK(in_table[first_of[bb] + c] == (own ? bin_used[bb] : 1), "item %u of bin %u: in the table %d, bin active %d", first_of[bb] + c, bb, in_table[first_of[bb] + c], bin_used[bb]);
    // ---- geometry: every chunk (every list entry) of every segment is visited exactly once, nothing else is
    plan_geometry(p, f);
    const uint32_t split = f.opt_split >= 0 ? (uint32_t)f.opt_split : p.split_log2;
    CHECK(p.split_log2 == split && p.split_log2 <= 2 && p.fine_log2 == (f.opt_fine >= 0 ? (uint32_t)f.opt_fine : 2 - split), "split %u fine %u", p.split_log2, p.fine_log2);
    CHECK(p.gy == ((n_active == 2 && cf && lit) ? 1u : std::max(n_active, 1u)) && p.last_wgs == (uint64_t)p.gx * p.gy, "gy %u, workgroups %" PRIu64, p.gy, p.last_wgs);
    CHECK(p.gx % (cf ? 1 : 8) == 0 && p.j_big <= p.pieces_per_run, "gx %u j_big %u pieces_per_run %u", p.gx, p.j_big, p.pieces_per_run);
    {   // the grid's numbers from what a CU holds at once: 7 workgroups of the parked class kernel, 6 of every other
        const uint64_t resident = (uint64_t)f.n_cus * (park ? 7 : 6);
        uint64_t est = (uint64_t)p.n_segments * n_groups / std::max<uint32_t>(own ? n_act_bins : n_bins, 1);
        if (light && n_active == 2 && lit) est = (est + 1) / 2;
        const uint32_t want_split = f.opt_split >= 0 ? (uint32_t)f.opt_split : est >= 2 * resident ? 0 : 2 * est >= 2 * resident ? 1 : 2;
        const uint32_t runs = cf ? 1 : 8, per_run = ((p.n_segments << want_split) + runs - 1) / runs;
        const uint32_t tail = p.fine_log2 == 0 ? 0 : (uint32_t)std::min<uint64_t>(per_run, (resident / p.gy + runs - 1) / runs);
        CHECK(p.split_log2 == want_split && p.pieces_per_run == per_run && p.j_big == per_run - tail && p.gx == (per_run - tail + (tail << p.fine_log2)) * runs,
              "grid split %u per run %u j_big %u gx %u; %" PRIu64 " resident workgroups give %u %u %u %u", p.split_log2, p.pieces_per_run, p.j_big, p.gx, resident,
              want_split, per_run, per_run - tail, (per_run - tail + (tail << p.fine_log2)) * runs);
    }
    for (uint32_t block = 0; block < p.gx; ++block) {
        uint32_t first = 0, count = 0;
        if (!decode_block(p, cf, block, segments, &first, &count)) continue;
        CHECK(count >= 1 && (size_t)first + count <= n_items, "workgroup %u walks items [%u, +%u)", block, first, count);
        for (uint32_t c = 0; c < count; ++c) g_visits[first + c] += 1;
    }
    for (size_t c = 0; c < n_items; ++c)
        CHECK(g_visits[c] == in_table[c], "item %zu is visited %d times (in the table: %d); gx %u split %u fine %u j_big %u pieces_per_run %u segments %u", c, g_visits[c],
              in_table[c], p.gx, p.split_log2, p.fine_log2, p.j_big, p.pieces_per_run, p.n_segments);
    // ---- and through the list: every strip of an active bin that holds sequence is reached by exactly one lane of one visited entry
    if (use_list) {
        std::vector<uint8_t> strip_hits((size_t)w.n_chunks * 64, 0);
        for (size_t e = 0; e < n_items; ++e) {
            if (!g_visits[e]) continue;
            const uint32_t entry = wl.entries[e];
            for (uint32_t lane = 0; lane < 64; ++lane) {
                uint32_t word = (entry & (WORK_NEED_V - 1)) * 256 + lane * 4;
                if (entry & WORK_PACKED) {
                    word = wl.strip_rows[(size_t)(entry & ~WORK_PACKED) * 64 + lane];
                    if (word == WORK_NO_STRIP) continue;
                }
                CHECK(word % 4 == 0 && word / 4 < strip_hits.size(), "entry %zu lane %u reads word %u", e, lane, word);
                strip_hits[word / 4] += 1;
            }
        }
        for (size_t i = 0; i < w.contig_len.size(); ++i) {
            const bool active = !own || bin_used[w.contig_bin[i]];
            for (uint64_t st = 0; st * 128 < w.contig_len[i]; ++st)
                CHECK(strip_hits[(size_t)w.contig_chunk[i] * 64 + st] == (active ? 1 : 0), "strip %" PRIu64 " of contig %zu is walked %d times", st, i,
                      strip_hits[(size_t)w.contig_chunk[i] * 64 + st]);
        }
    }
    return p;
}

void set_env(const char *name, const char *value) { if (value) setenv(name, value, 1); else unsetenv(name); }

void random_case(int i) {
    const uint32_t n_bins = chance(0.3) ? rnd(1, 8) : rnd(1, 400), n_slots = rnd(1, 8);
    World w = make_world(n_bins, chance(0.5) ? 40 : 6, n_slots);
    w.f.opt_no_lit = chance(0.1); w.f.opt_no_cf = chance(0.1); w.f.opt_no_inline = chance(0.1);
    w.f.opt_split = (int)rnd(0, 5) - 3; if (w.f.opt_split < -1) w.f.opt_split = -1;
    w.f.opt_fine = (int)rnd(0, 5) - 3;  if (w.f.opt_fine < -1) w.f.opt_fine = -1;
    set_env("NM_ALL_SEGMENTS", chance(0.1) ? "1" : nullptr);
    set_env("NM_STAGE_COPIES", chance(0.1) ? "1" : nullptr);
    set_env("NM_SCORE_CLASSES", chance(0.15) ? "0" : nullptr);
    set_env("NM_SCORE_HEAD", chance(0.15) ? "0" : nullptr);
    { static const char *const tails[3] = {"0", "1", "2"}; set_env("NM_SCORE_TAIL", chance(0.3) ? tails[rnd(0, 2)] : nullptr); }
    set_env("NM_SCORE_PACK_TAILS", chance(0.3) ? "0" : nullptr);
    set_env("NM_SCORE_PARK", chance(0.25) ? "0" : nullptr);
    w.lists = chance(0.85);
    Batch b;
    const uint32_t n = chance(0.05) ? 0 : chance(0.15) ? rnd(1, 5000) : rnd(1, 300);
    const uint32_t use_bins = chance(0.5) ? n_bins : rnd(1, n_bins), use_slots = rnd(1, n_slots);
    const int style = (int)rnd(0, 4);                    // 0 literal compact, 1 with sets, 2 general, 3 wide, 4 anything
    static const uint32_t borders[6] = {31, 32, 63, 64, 95, 95};
    for (uint32_t k = 0; k < n; ++k) {
        int kind = style == 0 ? 0 : (int)rnd(0, 2);
        const bool compact = style == 0 || style == 1 || (style != 2 ? chance(0.9) : chance(0.5));
        const uint32_t reach = (style == 3 && chance(0.3)) || (style == 4 && chance(0.05)) ? borders[rnd(0, 5)] : 0;
        add_motif(b, w, rnd(0, use_bins - 1), rnd(0, use_slots - 1), kind, reach, compact);
    }
    if (n && chance(0.25)) {                             // one candidate the validation must name
        const uint32_t k = rnd(0, n - 1);
        Batch one;
        switch (rnd(0, 7)) {
        case 0: b.slot[k] = (uint8_t)(chance(0.5) ? n_slots : rnd(8, 255)); if (b.slot[k] < 8 && (w.f.slot_present >> b.slot[k] & 1u)) b.slot[k] = 200; break;
        case 1: b.bin[k] = n_bins + rnd(0, 3); break;
        case 2: b.len[k] = chance(0.5) ? 0 : (uint8_t)rnd(192, 255); break;
        case 3: b.mp[k] = (uint8_t)(b.len[k] + rnd(0, 3)); break;
        case 4: add_motif(one, w, b.bin[k], b.slot[k], 3); break;
        case 5: add_motif(one, w, b.bin[k], b.slot[k], 4); break;
        case 6: add_motif(one, w, b.bin[k], b.slot[k], 0, 96); break;
        case 7: add_motif(one, w, b.bin[k], b.slot[k], 0, 120); break;
        }
        if (one.size()) {
            b.len[k] = one.len[0]; b.mp[k] = one.mp[0];
            b.off[k] = (uint32_t)b.masks.size();
            b.masks.insert(b.masks.end(), one.masks.begin() + one.off[0], one.masks.end());
        }
        if (b.len[k] > 14) b.masks.insert(b.masks.end(), 260, 15);          // (a forged length reads on: keep it inside the pool)
    }
    const int mode = (int)rnd(0, 9);                      // host counts, deferred, device counts, per-contig, spec
    if (mode == 5) b.defer = true;
    if (mode == 6) b.host_out = false;
    if (mode == 7) {
        add_rows(b, w);
        if (n && chance(0.15)) { const uint32_t k = rnd(1, n); for (uint32_t q = k; q <= n; ++q) b.rows[q] += 1; }
    }
    if (mode == 8) { b.spec = true; b.stride = 64 * rnd(1, 3); b.extra_in = rnd(0, 5000); b.extra_out = rnd(0, 5000); }
    run_case(("random " + std::to_string(i)).c_str(), w, b);
}

void clear_env() { for (const char *e : {"NM_ALL_SEGMENTS", "NM_STAGE_COPIES", "NM_SCORE_CLASSES", "NM_SCORE_HEAD", "NM_SCORE_TAIL", "NM_SCORE_PACK_TAILS", "NM_SCORE_PARK"}) unsetenv(e); }

// n candidates dealt round the groups (slot s, bin b), s < n_slots, b < use_bins
Batch dealt(const World &w, uint32_t n, uint32_t use_bins, uint32_t n_slots, int kind) {
    Batch b;
    for (uint32_t k = 0; k < n; ++k) add_motif(b, w, k % use_bins, (k / use_bins) % n_slots, kind);
    return b;
}

void directed_cases() {
    clear_env();
    {   // exactly 6 and 7 candidates per group: the light / heavy crossover
        World w = make_world(10, 20, 2, 1.0);
        for (uint32_t per : {6u, 7u}) {
            const ScorePlan p = run_case("6 | 7 per group", w, dealt(w, per * 20, 10, 2, 1));
            CHECK(p.light == (per == 6) && p.cf == p.light && p.classes == !p.light, "%u per group: light %d classes %d", per, p.light, p.classes);
        }
        const ScorePlan p = run_case("6 per group + 1", w, dealt(w, 121, 10, 2, 1));
        CHECK(!p.light, "121 candidates in 20 groups are light");
    }
    {   // n_prog 2048 | 2049: the single-launch compile
        World w = make_world(400, 3, 1, 1.0);
        for (uint32_t n : {2048u, 2049u}) {
            const ScorePlan p = run_case("n_prog 2048 | 2049", w, dealt(w, n, 400, 1, 0));
            CHECK(p.cf && p.compile == (n == 2048 ? PLAN_COMPILE_FUSED : PLAN_COMPILE_THEN_COMMON), "%u light candidates compile by path %d", n, p.compile);
        }
    }
    {   // n_entries 8192 | 8193
        World w2 = make_world(4096, 1, 2, 1.0), w3 = make_world(2731, 1, 3, 1.0);
        ScorePlan p = run_case("n_entries 8192", w2, dealt(w2, 2000, 1000, 2, 0));
        CHECK(p.n_entries == 8192 && p.compile == PLAN_COMPILE_FUSED, "entries %u path %d", p.n_entries, p.compile);
        p = run_case("n_entries 8193", w3, dealt(w3, 2001, 667, 3, 0));
        CHECK(p.n_entries == 8193 && p.compile == PLAN_COMPILE_THEN_COMMON, "entries %u path %d", p.n_entries, p.compile);
    }
    for (uint32_t n : {8u, 16u, 400u}) {   // active segments at 4a = 3n and one more
        World w = make_world(n, 1, 2, 1.0, 1);
        const uint32_t a = 3 * n / 4;
        ScorePlan p = run_case("4a = 3n", w, dealt(w, 3 * a, a, 1, 1));
        CHECK(p.own_segments && p.n_segments == a, "%u of %u segments: own %d", a, n, p.own_segments);
        p = run_case("4a = 3n + 4", w, dealt(w, 3 * (a + 1), a + 1, 1, 1));
        CHECK(!p.own_segments && p.n_segments == n, "%u of %u segments: own %d", a + 1, n, p.own_segments);
        setenv("NM_ALL_SEGMENTS", "1", 1);
        p = run_case("4a = 3n, NM_ALL_SEGMENTS", w, dealt(w, 3 * a, a, 1, 1));
        CHECK(!p.own_segments, "NM_ALL_SEGMENTS=1 and the batch's own table");
        clear_env();
    }
    {   // staged bytes at 4 MiB and 16 bytes beyond: pad the mask pool until the total lands there
        World w = make_world(1, 1, 1, 1.0);
        for (size_t target : {(size_t)4 << 20, ((size_t)4 << 20) + 16}) {
            Batch b = dealt(w, 1000, 1, 1, 0);
            bind(w);
            ScorePlan probe = run_case("staged bytes, probe", w, b);
            b.masks.insert(b.masks.end(), target - probe.total, 15);
            b.off.back() = (uint32_t)(b.masks.size() - b.len.back());        // the last candidate's motif moves to the end of the pool
            for (uint32_t j = 0; j < b.len.back(); ++j) b.masks[b.off.back() + j] = j == b.mp.back() ? ((w.f.slot_is_c & 1u) ? NM_BASE_C : NM_BASE_A) : 15;
            const ScorePlan p = run_case("staged bytes 4 MiB | + 16", w, b);
            CHECK(p.total == target && p.by_kernels == (target == (size_t)4 << 20), "total %zu (wanted %zu), by_kernels %d", p.total, target, p.by_kernels);
        }
    }
    {   // count bytes at 4 MiB and 16 bytes beyond
        World w = make_world(1, 1, 1, 1.0);
        Batch b = dealt(w, 10, 1, 1, 0);
        for (uint32_t n : {262144u, 262145u}) {
            Batch big;
            for (uint32_t k = 0; k < n; ++k) { big.bin.push_back(0); big.slot.push_back(0); big.len.push_back(b.len[k % 10]); big.mp.push_back(b.mp[k % 10]); big.off.push_back(b.off[k % 10]); }
            big.masks = b.masks;
            const ScorePlan p = run_case("count bytes 4 MiB | + 16", w, big);
            CHECK(p.out_bytes == (size_t)n * 16 && p.via_stage == (n == 262144) && !p.by_kernels, "%u candidates: via_stage %d by_kernels %d", n, p.via_stage, p.by_kernels);
            big.defer = true;
            const ScorePlan q = run_case("count bytes, deferred", w, big);
            CHECK(q.via_stage, "a deferred batch comes back through the pair");
        }
    }
    for (int split = -1; split <= 2; ++split)           // every NM_SPLIT x NM_FINE setting, small and large assemblies, light and heavy
        for (int fine = -1; fine <= 2; ++fine)
            for (uint32_t n_bins : {1u, 3u, 60u, 400u})
                for (uint32_t per : {1u, 9u}) {
                    World w = make_world(n_bins, 40, 2, 0.9);
                    w.f.opt_split = split;
                    w.f.opt_fine = fine;
                    run_case("NM_SPLIT x NM_FINE", w, dealt(w, per * 2 * n_bins, n_bins, 2, 1));
                    run_case("NM_SPLIT x NM_FINE, few bins", w, dealt(w, per * 2, 1, 2, 0));
                }
    {   // tails packed: a bin of 17 chunks in two contigs is two segments of chunks and of the plain list, one of the packed list (15
        // full chunks and one row); light and per-contig batches keep the chunk table whatever the switch says
        World w = make_world_of({{10 * 8192 + 3000, 5 * 8192 + 4000}, {20 * 8192 + 100}, {300, 500, 700}, {}}, 16, 2);
        Batch heavy;
        for (uint32_t k = 0; k < 28; ++k) add_motif(heavy, w, k % 4 == 3 ? 0 : k % 4, 0, 1);
        ScorePlan p = run_case("tails packed", w, heavy);
        CHECK(p.use_list && p.pack && !p.own_segments && p.n_segments == 1 + 2 + 1, "packed list: use_list %d pack %d segments %u", p.use_list, p.pack, p.n_segments);
        setenv("NM_SCORE_PACK_TAILS", "0", 1);
        p = run_case("tails packed, NM_SCORE_PACK_TAILS=0", w, heavy);
        CHECK(p.use_list && !p.pack && p.n_segments == 2 + 2 + 1, "plain list: use_list %d pack %d segments %u", p.use_list, p.pack, p.n_segments);
        clear_env();
        Batch rows = heavy;
        add_rows(rows, w);
        p = run_case("tails packed, per-contig", w, rows);
        CHECK(!p.use_list && p.n_segments == 2 + 2 + 1, "per-contig: use_list %d segments %u", p.use_list, p.n_segments);
        p = run_case("tails packed, light", w, dealt(w, 6, 3, 1, 1));
        CHECK(!p.use_list && p.cf, "light: use_list %d", p.use_list);
        w.lists = false;
        p = run_case("no lists", w, heavy);
        CHECK(!p.use_list && p.n_segments == 2 + 2 + 1, "no lists: use_list %d segments %u", p.use_list, p.n_segments);
    }
    for (uint32_t slots : {1u, 2u})                      // one and two active slots, with and without lit
        for (int kind : {0, 1}) {
            World w = make_world(12, 20, 2, 1.0);
            const ScorePlan p = run_case("slots x lit", w, dealt(w, 3 * 12 * slots, 12, slots, kind));
            CHECK(p.n_active == slots && p.lit == (kind == 0) && p.fuse == (slots == 2 && kind == 0) && p.gy == (p.fuse ? 1u : slots), "slots %u kind %d: lit %d fuse %d gy %u",
                  slots, kind, p.lit, p.fuse, p.gy);
            w.f.opt_no_lit = true;
            const ScorePlan q = run_case("slots x lit, NM_NO_LIT", w, dealt(w, 3 * 12 * slots, 12, slots, kind));
            CHECK(!q.lit && !q.fuse && q.np == 8, "NM_NO_LIT and a literal tile");
        }
}

// ---- the parked class kernel: which batches take it, and what its 7 resident workgroups a CU do to the grid.  `report`: one line
// per planned batch on stdout, for tests/test_score_park_host.py
void park_line(bool report, const char *what, uint32_t size, const World &w, const ScorePlan &p) {
    if (report)
        printf("park %s size %u parked %d classes %d fits %d n_cus %u n_segments %u n_groups %u split_log2 %u fine_log2 %u pieces_per_run %u j_big %u gx %u gy %u\n", what, size,
               p.park, p.classes, p.park_fits, w.f.n_cus, p.n_segments, p.n_groups, p.split_log2, p.fine_log2, p.pieces_per_run, p.j_big, p.gx, p.gy);
}

// `size` candidates with a set in each of `groups` (slot 0, bin) groups, bin < groups
Batch park_batch(const World &w, uint32_t size, uint32_t groups) {
    Batch b;
    for (uint32_t g = 0; g < groups; ++g)
        for (uint32_t k = 0; k < size; ++k) add_motif(b, w, g, 0, k == 0 ? 1 : (int)rnd(0, 2));
    // (a set that fell on the modified base stays a literal: one candidate that surely has a set)
    const uint8_t can = (w.f.slot_is_c & 1u) ? NM_BASE_C : NM_BASE_A;
    const uint8_t motif[3] = {5, can, 8};
    b.len[0] = 3; b.mp[0] = 1; b.off[0] = (uint32_t)b.masks.size();
    b.masks.insert(b.masks.end(), motif, motif + 3);
    return b;
}

void park_cases(bool report) {
    clear_env();
    // a small assembly: two bins of a few contigs
    World small = make_world_of({{3 * 8192 + 500, 9000, 700}, {5 * 8192 + 100, 300}}, 16, 2);
    for (uint32_t size : {1u, 10u, 27u, 28u, 29u, 30u, 32u, 33u, 56u, 57u, 60u, 64u, 65u, 84u, 85u, 96u, 97u}) {
        const bool fits = (size + 27) / 28 == (size + 31) / 32;
        // size 1 .. 6 in both groups is a light batch: the group under test sits beside one of 28
        Batch b = park_batch(small, size, 1);
        for (uint32_t k = 0; k < 28; ++k) add_motif(b, small, 1, 0, 1);
        ScorePlan p = run_case("park rule", small, b);
        CHECK(p.classes && p.park == fits && p.park_fits == fits, "a group of %u: classes %d parked %d", size, p.classes, p.park);
        park_line(report, "rule", size, small, p);
        setenv("NM_SCORE_PARK", "0", 1);
        p = run_case("park rule, NM_SCORE_PARK=0", small, b);
        CHECK(p.classes && !p.park && p.park_fits == fits, "NM_SCORE_PARK=0 and a group of %u: parked %d", size, p.park);
        park_line(report, "switch0", size, small, p);
        setenv("NM_SCORE_PARK", "1", 1);
        p = run_case("park rule, NM_SCORE_PARK=1", small, b);
        CHECK(p.park == fits, "NM_SCORE_PARK=1 and a group of %u: parked %d", size, p.park);
        clear_env();
        // one group that does not fit unparks the whole batch, wherever it is
        Batch two = park_batch(small, 28, 1);
        for (uint32_t k = 0; k < size; ++k) add_motif(two, small, 1, 1, 1);
        p = run_case("park rule, second slot", small, two);
        CHECK(p.classes && p.park == fits, "a group of %u in the second slot: parked %d", size, p.park);
        // per-contig rows: the twin kernel, never parked
        Batch rows = b;
        add_rows(rows, small);
        p = run_case("park rule, per-contig", small, rows);
        CHECK(p.classes && !p.park, "a per-contig batch is parked");
        park_line(report, "per_contig", size, small, p);
        setenv("NM_SCORE_CLASSES", "0", 1);
        p = run_case("park rule, NM_SCORE_CLASSES=0", small, b);
        CHECK(!p.classes && !p.park, "NM_SCORE_CLASSES=0 and a parked batch");
        park_line(report, "classes0", size, small, p);
        clear_env();
    }
    {   // light (six a group), literal-only and wide batches: other kernels
        ScorePlan p = run_case("park, light", small, dealt(small, 12, 2, 1, 1));
        CHECK(p.cf && !p.classes && !p.park, "a light batch: cf %d parked %d", p.cf, p.park);
        park_line(report, "light", 6, small, p);
        p = run_case("park, literal", small, dealt(small, 40, 2, 1, 0));
        CHECK(p.lit && !p.park, "a literal batch: lit %d parked %d", p.lit, p.park);
        park_line(report, "literal", 20, small, p);
        Batch wide = park_batch(small, 10, 2);
        add_motif(wide, small, 0, 0, 1, 40);
        p = run_case("park, wide", small, wide);
        CHECK(p.any_wide == 1 && !p.classes && !p.park, "a wide batch: parked %d", p.park);
        park_line(report, "wide", 11, small, p);
    }
    // the grid: `bins` bins of one contig of 255 full chunks and a tail (16 or 17 segments each), 256 CUs.  208 bins are more than two
    // rounds of 6 x 256 workgroups and fewer than two of 7 x 256: the parked batch halves its pieces, the unparked one does not; 120 bins
    // are fewer than two rounds and 400 more on both sides: the same split, other j_big and gx
    for (uint32_t bins : {120u, 208u, 400u}) {
        World big = make_world_of(std::vector<std::vector<uint64_t>>(bins, {(uint64_t)255 * 8192 + 4000}), 16, 1);
        const Batch b = park_batch(big, 7, bins);
        const ScorePlan parked = run_case("park grid", big, b);
        park_line(report, "grid", bins, big, parked);
        setenv("NM_SCORE_PARK", "0", 1);
        const ScorePlan plain = run_case("park grid, NM_SCORE_PARK=0", big, b);
        park_line(report, "grid0", bins, big, plain);
        clear_env();
        CHECK(parked.park && !plain.park && parked.n_segments == plain.n_segments, "grid of %u bins: parked %d | %d", bins, parked.park, plain.park);
        const uint64_t est = parked.n_segments;            // one group a bin, every bin active
        CHECK((est < 2 * 6 * 256) == (bins == 120) && (est >= 2 * 7 * 256) == (bins == 400), "%u bins are %" PRIu64 " workgroups", bins, est);
        CHECK(parked.split_log2 == (bins == 400 ? 0u : 1u) && plain.split_log2 == (bins == 120 ? 1u : 0u), "%u bins: split %u | %u", bins, parked.split_log2, plain.split_log2);
        const uint32_t per_run_parked = ((parked.n_segments << parked.split_log2) + 7) / 8, per_run_plain = ((plain.n_segments << plain.split_log2) + 7) / 8;
        CHECK(parked.j_big == per_run_parked - 7 * 256 / 8 && plain.j_big == per_run_plain - 6 * 256 / 8, "%u bins: j_big %u | %u", bins, parked.j_big, plain.j_big);
        CHECK(parked.gx == (parked.j_big + (7u * 256 / 8 << parked.fine_log2)) * 8 && plain.gx == (plain.j_big + (6u * 256 / 8 << plain.fine_log2)) * 8, "%u bins: gx %u | %u", bins,
              parked.gx, plain.gx);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "park") {   // the park cases alone, reported line by line
        rng.seed(20240521ull);
        park_cases(true);
        printf("plan_check ok: park cases, %ld batches, %ld checks\n", g_cases, g_checks);
        return 0;
    }
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 20240521ull;
    const int n_random = argc > 2 ? atoi(argv[2]) : 3000;
    rng.seed(seed);
    directed_cases();
    park_cases(false);
    const long directed = g_cases;
    for (int i = 0; i < n_random; ++i) random_case(i);
    clear_env();
    printf("plan_check ok: seed %" PRIu64 ", %ld directed + %d random batches (%ld rejected by the validation), %ld checks\n", seed, directed, n_random, g_rejected, g_checks);
    return 0;
}
