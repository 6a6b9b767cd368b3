// Device-side building blocks of the scan shared by the translation units that evaluate motifs against the resident
// planes (nmscan.hip: the scoring kernels and nm_hit_positions; nmmeth.hip: the per-contig read-methylation table), plus
// the host-side compiler of one motif into its constraint program.  Internal: not part of the C ABI.
#pragma once
#include "nmscan_internal.h"

namespace nmdetail {

__device__ __forceinline__ uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
    return __builtin_amdgcn_alignbit(hi, lo, sh);
}

// Read-only tables are addressed through the constant address space so that wave-uniform reads become scalar
// loads (s_load_dwordx16 straight into SGPRs) instead of vector loads + v_readfirstlane.
typedef const uint32_t __attribute__((address_space(4))) *cu32p;
typedef const uint8_t __attribute__((address_space(4))) *cu8p;

// Kernel variant: GN / GP halo words left / right (narrow 1 / 1: offsets in [-32, 31]; wide 2 / 2), COMPACT state planes
// {M, U} or the four per-strand planes, NS mod-type slots fused per workgroup, LIT = every constraint of the batch is a
// literal (only the four is-X planes are built — every batch of the greedy search is: children are single letters,
// find_motifs_bin.py:1005-1018), CF = the constraints common to all candidates of a (slot, bin) group are evaluated
// once per tile (sibling children of one expansion differ in ONE position, :1116-1135).
// Tried and dropped for the light variants (same-device A/B, tools/gpu_ab.sh, 1 Gbp greedy round): a register double
// buffer of the next chunk's raw words (120 VGPRs, 4 waves: -18 %); touching the next chunk's lines with one dword per
// lane and plane so that they are on their way into L2 (-25 %; with nontemporal touches -45 %); 8 waves per SIMD by
// launch bounds (3 spills; -4 % with two children per group, +6 % with four); segments of 8 / 32 / 64 chunks (all
// slower than 16); handing segments out through a device-wide atomic queue instead of one workgroup per segment
// (-60 %: device-scope atomics are served at the memory side on this multi-die part and serialise).  A 10 Gbp run
// takes 10.0 x the 1 Gbp time: there is no partial-last-round tail worth chasing at that size.  An EVEN static split —
// exactly the resident number of workgroups, each walking an equal, candidate-weighted share of the active bins' chunks
// across bin boundaries (parity green) — was 28 % slower at 1 Gbp and 20 % slower on a 125 Mbp shard: equal shares do
// not finish together, and nothing rebalances them; the hardware dispatcher's one-workgroup-per-segment order does.
#ifndef NM_LIT_WAVES
#define NM_LIT_WAVES 4      // minimum waves per SIMD the literal-only variants are compiled for
#endif

// CLS (narrow, compact, non-literal heavy batches only): every IUPAC set is ONE constraint on the class planes
// (ClassTile / ClassWalk below); the program is the 32-dword class layout, of which PDW and NP say nothing.
// PARK (the CLS variant that is not per-contig): the chunk's state words M and U, read by nothing but the finalize of a walk, wait
// in LDS through the walks — a slot per thread, written once per entry and read back behind every walk's last constraint.
// Their eight registers are free where the body peaks: 72 VGPRs, 7 waves per SIMD.  A pass counts PLAN_PARK_ROWS candidates, so
// that seven workgroups' counters and park areas fit a CU's LDS (profiles/r27/park_state.md).
template <int GN_, int GP_, bool COMPACT_, int NS_, bool LIT_, bool CF_, bool PC_ = false, bool CLS_ = false, bool PARK_ = false>
struct Variant {
    static constexpr int GN = GN_, GP = GP_, NS = NS_;
    static constexpr bool COMPACT = COMPACT_, LIT = LIT_, CF = CF_, PC = PC_;   // PC: counters keyed by (candidate, contig)
    static constexpr bool CLS = CLS_, PARK = PARK_;
    static_assert(!CLS || (GN == 1 && GP == 1 && COMPACT && NS == 1 && !LIT && !CF), "class planes: narrow compact heavy variants only");
    static_assert(!PARK || (CLS && !PC), "parked state words: the class variant with LDS counters only");
    static constexpr int ROWS = PARK ? (int)PLAN_PARK_ROWS : BMAX;   // LDS counter rows of a workgroup = candidates of a pass (NS = 1)
    static_assert(BMAX == (int)PLAN_PASS_ROWS, "the plan counts passes of BMAX candidates");
    static constexpr int NW = T_WORDS + GN + GP;
    static constexpr int NP = LIT ? 4 : 8;                 // planes per tile
    static constexpr int NST = COMPACT ? 2 : 4;            // state planes per slot
    static constexpr int PDW = (GN + GP) * NP;             // dwords of one strand's program
};

// The raw words one lane holds of one chunk: T main words of H / L (/ V) plus the halo, and the state words of the
// NS slots.  All loads of a chunk are issued back to back, nothing is waited for here.
template <class K>
struct RawChunk {
    uint32_t h[K::NW], l[K::NW], v[K::NW];
    uint32_t s[K::NS][K::NST][T_WORDS];
    bool need_v;                                           // wave-uniform

    __device__ __forceinline__ void load(const Planes &seq, const StatePlanes (&stp)[K::NS], uint32_t chunk, int lane) {
        need_v = ((cu8p)seq.needs_v)[chunk] != 0;          // scalar load, issued first
        load_at(seq, stp, (size_t)chunk * CHUNK_WORDS + (size_t)lane * T_WORDS);
    }
    // One entry of a work list (nmscore_worklist.h; the heavy variants that are not per-contig): a chunk with its needs_v bit, or
    // a packed row, whose lanes take the strips strip_rows gives them — the partly filled last chunks of the bin's contigs, always
    // with V.  Everything a lane uses hangs on its own base, so the walk, the counters and the flush do not see the difference.  A
    // lane without a strip reads words 3 .. 10 of chunk 0, the zero pad in front of the space in every plane: V = 0 keeps it out
    // of every count, as it keeps padding out (no branch, no lane switched off around the loads).
    __device__ __forceinline__ void load_entry(const Planes &seq, const StatePlanes (&stp)[K::NS], uint32_t entry, const uint32_t *strip_rows, int lane) {
        if (entry & WORK_PACKED) {                         // wave-uniform
            const uint32_t w = strip_rows[(size_t)(entry & ~WORK_PACKED) * WORK_STRIPS + lane];
            need_v = true;
            load_at(seq, stp, (size_t)(w == WORK_NO_STRIP ? (uint32_t)T_WORDS : w));
        } else {
            need_v = (entry & WORK_NEED_V) != 0;
            load_at(seq, stp, (size_t)(entry & (WORK_NEED_V - 1)) * CHUNK_WORDS + (size_t)lane * T_WORDS);
        }
    }
    // base: the lane's first word in every plane; need_v is set
    __device__ __forceinline__ void load_at(const Planes &seq, const StatePlanes (&stp)[K::NS], const size_t base) {
        constexpr int GN = K::GN, GP = K::GP;
#pragma unroll
        for (int j = 0; j < K::NS; ++j) {
            const uint32_t *src[4] = {K::COMPACT ? stp[j].M : stp[j].MP, K::COMPACT ? stp[j].U : stp[j].UP, stp[j].MM, stp[j].UM};
#pragma unroll
            for (int i = 0; i < K::NST; ++i) {
                const uint4 q = *reinterpret_cast<const uint4 *>(src[i] + base);
                s[j][i][0] = q.x; s[j][i][1] = q.y; s[j][i][2] = q.z; s[j][i][3] = q.w;
            }
        }
        const uint4 h4 = *reinterpret_cast<const uint4 *>(seq.H + base);
        const uint4 l4 = *reinterpret_cast<const uint4 *>(seq.L + base);
        h[GN + 0] = h4.x; h[GN + 1] = h4.y; h[GN + 2] = h4.z; h[GN + 3] = h4.w;
        l[GN + 0] = l4.x; l[GN + 1] = l4.y; l[GN + 2] = l4.z; l[GN + 3] = l4.w;
#pragma unroll
        for (int j = 0; j < GN; ++j) { h[j] = seq.H[base - GN + j]; l[j] = seq.L[base - GN + j]; }
#pragma unroll
        for (int j = 0; j < GP; ++j) { h[GN + T_WORDS + j] = seq.H[base + T_WORDS + j]; l[GN + T_WORDS + j] = seq.L[base + T_WORDS + j]; }
        if (need_v) {                                      // wave-uniform
            const uint4 v4 = *reinterpret_cast<const uint4 *>(seq.V + base);
            v[GN + 0] = v4.x; v[GN + 1] = v4.y; v[GN + 2] = v4.z; v[GN + 3] = v4.w;
#pragma unroll
            for (int j = 0; j < GN; ++j) v[j] = seq.V[base - GN + j];
#pragma unroll
            for (int j = 0; j < GP; ++j) v[GN + T_WORDS + j] = seq.V[base + T_WORDS + j];
        } else if constexpr (!K::CLS) {                    // (a CLS variant never looks at V in an all-valid chunk)
#pragma unroll
            for (int j = 0; j < K::NW; ++j) v[j] = 0xFFFFFFFFu;
        }
    }
};

// Derived planes of the tile: is-A/C/G/T and (unless LIT) valid-not-A/C/G/T, NW words each.
template <class K>
struct Tile {
    uint32_t w[K::NP][K::NW];

    __device__ __forceinline__ void expand(const RawChunk<K> &r) {
#pragma unroll
        for (int j = 0; j < K::NW; ++j) {
            const uint32_t hh = r.h[j], ll = r.l[j], vv = r.v[j];
            w[0][j] = vv & ~hh & ~ll;          // A = 00
            w[1][j] = vv & ~hh & ll;           // C = 01
            w[2][j] = vv & hh & ll;            // G = 11
            w[3][j] = vv & hh & ~ll;           // T = 10
            if (!K::LIT) {
                w[4][j] = vv & (hh | ll);          // valid, not A
                w[5][j] = vv & (hh | ~ll);         // valid, not C
                w[6][j] = vv & ~(hh & ll);         // valid, not G
                w[7][j] = vv & (~hh | ll);         // valid, not T
            }
        }
    }
};

// acc[t] &= plane p at offset d (d = 32 g + r) for every constraint bit of one strand's program
// (prog[g * NP + p], bit r; g counts from the leftmost word-group the variant reads).  Control flow is scalar and
// wave-uniform (s_ff1 over the SGPR masks), register indices are static.
template <class K>
__device__ __forceinline__ void eval_masks(const uint32_t (&m)[K::PDW], const Tile<K> &tile, uint32_t (&acc)[T_WORDS]) {
#pragma unroll
    for (int g = 0; g < K::GN + K::GP; ++g) {            // word pair (t + g, t + g + 1)
#pragma unroll
        for (int p = 0; p < K::NP; ++p) {
            uint32_t mm = m[g * K::NP + p];
            while (mm) {
                const uint32_t r = __builtin_ctz(mm);
                mm &= mm - 1;
#pragma unroll
                for (int t = 0; t < T_WORDS; ++t) acc[t] &= alignbit(tile.w[p][t + g + 1], tile.w[p][t + g], r);
            }
        }
    }
}

// ---- both strands of a heavy candidate from its FORWARD masks (score_candidates, non-CF variants) -------------------
// compile_one writes the reverse half as the mirror of the forward one: a forward constraint on plane p at offset
// d = 32 (g - GN) + r is a reverse constraint on the complemented plane at -d, i.e. word-group 2 GN - 1 - g, shift 32 - r
// for r > 0, and word-group 2 GN - g, shift 0 for r = 0 (no d = -32 GN: the host sends no offset that far to the variant).
// So one scalar walk over the forward words drives both strands, and the reverse half is not read.
constexpr int comp_plane(int p) { return (p & 4) | (3 - (p & 3)); }   // A<->T, C<->G, not-A<->not-T, not-C<->not-G

template <class K>
struct JointWalk {
    uint32_t accf[T_WORDS], accr[T_WORDS];                 // the match masks once walk() returns

    // r = 0 can reach word-group G unless it is d = -32 GN (beyond every variant's reach) or the modified position of a
    // compact batch (folded into the base)
    template <int G>
    static constexpr bool r0_possible() { return G > 0 && !(K::COMPACT && G == K::GN); }

    // acc &= the words of constraint bit r of forward mask word I shifted into place, both strands (R0: the bit-0
    // constraint of a word whose reverse twin sits one word-group further, unshifted)
    template <int I, bool R0 = false>
    __device__ __forceinline__ void and_in(const Tile<K> &tile, uint32_t r) {
        constexpr int G = I / K::NP, P = I % K::NP, CP = comp_plane(P), GR = R0 ? 2 * K::GN - G : 2 * K::GN - 1 - G;
        const uint32_t rr = R0 ? 0u : 32u - r;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) accf[t] &= alignbit(tile.w[P][t + G + 1], tile.w[P][t + G], r);
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) accr[t] &= alignbit(tile.w[CP][t + GR + 1], tile.w[CP][t + GR], rr);
    }
    // acc = base, then every constraint of the forward masks m: four v_alignbit + four v_and per strand, one s_ff1 walk.
    template <int I = 0>
    __device__ __forceinline__ void walk(const uint32_t (&m)[K::PDW], const Tile<K> &tile, const uint32_t (&bf)[T_WORDS],
                                         const uint32_t (&br)[T_WORDS]) {
        if constexpr (I == 0) {
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) { accf[t] = bf[t]; accr[t] = br[t]; }
        }
        if constexpr (I < K::PDW) {
            uint32_t mm = m[I];
            if (r0_possible<I / K::NP>() && (mm & 1u)) {   // wave-uniform
                mm &= ~1u;
                and_in<I, true>(tile, 0u);
            }
            while (mm) {                                   // wave-uniform
                const uint32_t r = __builtin_ctz(mm);
                mm &= mm - 1;
                and_in<I>(tile, r);
            }
            walk<I + 1>(m, tile, bf, br);
        }
    }
};

// ---- IUPAC classes: every set of 1, 2 or 3 bases as ONE constraint (score_candidates, the CLS variants) ---------------
// On the stored 2-bit code (A = 00, C = 01, G = 11, T = 10 as H, L) every 2-set is a bit function of H, L and
// X = H ^ L — [GT] = H, [AC] = ~H, [CG] = L, [AT] = ~L, [CT] = X, [AG] = ~X — and every 3-set is the complement of a
// literal plane.  A constraint is a plane and a sense: positive (acc &= plane) or negative (acc &= ~plane).
// Class word p of a word-group (bit r = shift r, as everywhere):
//     0..3   A+ C+ G+ T+                  the literals
//     4..7   A- C- G- T-                  the 3-sets [CGT] [AGT] [ACT] [ACG]
//     8, 9   H+ H-    10, 11   L+ L-    12, 13   X+ X-
// The reverse strand takes the complemented set: A <-> T, C <-> G, and complementing flips H (so H+ <-> H-, X+ <-> X-)
// and leaves L alone.  One program is CLS_PROG_DW dwords, forward half only:
//     [0..7] literal words of word-groups 0, 1   [8] summary   [9..28] words 4..13 of word-groups 0, 1   [29..31] head
// summary: bit 10 g + (p - 4) is set iff word p >= 4 of word-group g is not empty, and bit 20 + q iff one of the four
// class words 4 q .. 4 q + 3 (counted from dword 9) is: the walk tests the whole dword, then one bit per quad.  It fetches a program as two
// s_load_dwordx16: the first holds everything a candidate of literals needs (and the first seven class words).
// Canonical first: all candidates of a workgroup belong to one mod slot, so their canonical base is known before the
// first chunk arrives.  Flipping L swaps A <-> C and G <-> T and commutes with complementation (which flips H), so the
// tile of a C slot is built from (H, ~L) and the tile of an A slot from (H, L): plane 0 is then the canonical base and
// plane 3 its complement whatever the slot, the walk starts from those two planes with plain moves, and the compiler
// (compile_one_classes) applies the same swap to every base set of a C-slot candidate.  One body for both mod types.
// head: the first two literal constraints of a candidate in walk order (lowest dword, then lowest bit) are taken out of
// their words and become the FIRST operation of its walk, acc = canonical plane & shift(P1) & shift(P2) straight from the
// tile: one v_bitop3 per accumulator word where the walk had a move and two v_and.  It happens once, before the word
// loop, so nothing is pending afterwards (a pair anywhere else needs state: docs/NEXT.md).  The descriptor is three
// dwords, laid out so that the walk spends two scalar shifts on it (v_alignbit takes the low five bits of a shift operand
// and the switch the id dword as it is; a scalar instruction of this kernel costs about an issue cycle):
//     [29] id   [30] r1 | r2 << 8 | lit_left << 16   [31] (32 - r1) | (32 - r2) << 8, the reverse twins' shifts
// id 0..35: the unordered pair (w1 <= w2) of literal words, w = 4 g + p = the word's dword (w1 == w2: two bits of one word,
// r1 < r2); 36..43: a single literal w; 44: no literal, the walk starts with plain moves.  lit_left: a literal word is still
// not empty (clear: the eight literal words are skipped behind one test).  A shift is never 0 here (the modified position
// is folded and the offsets lie in [-31, 31]), so the head has no unshifted form.
// tail: 39 % of the candidates of a search have exactly ONE class constraint, and the walk reads it from the summary, not
// from behind the quad guards and the word tests: bit 25 says so, the constraint's word is then the one set bit among summary
// bits 0..19 (one s_ff1), its r sits in bits 26..30 and the reverse shift is one s_sub; the class word keeps its bit and is
// not read.  (Descriptors for one or two left-over literals beside the head's shifts were built and measured too: they did
// not separate from the words in time and are not here, profiles/r25/tail_descriptors.md.)
constexpr int CLS_PROG_DW = 32, CLS_SUMMARY_DW = 8, CLS_WORDS_DW = 9, CLS_HEAD_DW = 29, CLS_HEAD_FWD_DW = 30, CLS_HEAD_REV_DW = 31;
constexpr int CLS_QUAD_BIT = 20;                // summary: bit CLS_QUAD_BIT + q is set iff one of class words 4 q .. 4 q + 3 is not empty
constexpr int CLS_LIT_WORDS = 8, CLS_HEAD_SINGLE = 36, CLS_HEAD_NONE = 44, CLS_HEADS = 45;
constexpr int CLS_CLASS_WORDS = 20;
constexpr int CLS_ONE_CLASS_BIT = 25, CLS_ONE_CLASS_R_BIT = 26;                        // summary
constexpr int CLS_TAIL_CLASS = 2;                                  // NM_SCORE_TAIL: the bit that asks for the lone-class descriptor (bit 0 named the literal ones)
// (w1, w2) -> id; w2 < 0: a single head; w1 < 0 as well: none
constexpr int cls_head_id(int w1, int w2) {
    return w1 < 0 ? CLS_HEAD_NONE : w2 < 0 ? CLS_HEAD_SINGLE + w1 : w1 * CLS_LIT_WORDS - w1 * (w1 - 1) / 2 + (w2 - w1);
}
constexpr int cls_head_w1(int id) {
    if (id >= CLS_HEAD_NONE) return -1;
    if (id >= CLS_HEAD_SINGLE) return id - CLS_HEAD_SINGLE;
    int w1 = 0;
    while (w1 + 1 < CLS_LIT_WORDS && cls_head_id(w1 + 1, w1 + 1) <= id) ++w1;
    return w1;
}
constexpr int cls_head_w2(int id) { return id >= CLS_HEAD_SINGLE ? -1 : cls_head_w1(id) + id - cls_head_id(cls_head_w1(id), cls_head_w1(id)); }
constexpr int cls_plane(int p) { return p < 4 ? p : p < 8 ? p - 4 : 4 + (p - 8) / 2; }         // planes of ClassTile
constexpr bool cls_neg(int p) { return p >= 4 && (p < 8 || ((p - 8) & 1)); }
constexpr int cls_mirror(int p) { return p < 4 ? 3 - p : p < 8 ? 11 - p : (p == 10 || p == 11) ? p : (p ^ 1); }
constexpr int cls_dword(int g, int p) { return p < 4 ? 4 * g + p : CLS_WORDS_DW + 10 * g + (p - 4); }
// class word of a base set (bit 0..3 = A C G T) of one, two or three bases
constexpr int cls_word_of_set(uint32_t set) {
    return set == 1 ? 0 : set == 2 ? 1 : set == 4 ? 2 : set == 8 ? 3 :
           set == 14 ? 4 : set == 13 ? 5 : set == 11 ? 6 : set == 7 ? 7 :
           set == 12 ? 8 : set == 3 ? 9 : set == 6 ? 10 : set == 9 ? 11 : set == 10 ? 12 : 13 /* set == 5 */;
}
// the base set of a C slot as its flipped tile sees it: A <-> C, G <-> T
constexpr uint32_t cls_swap_set(uint32_t set) { return ((set & 5u) << 1) | ((set & 10u) >> 1); }
// what the swap does to a class word: literals and 3-sets trade places pairwise, L+ <-> L-, X+ <-> X-, H stays
constexpr int cls_swap_word(int p) { return p < 8 ? (p ^ 1) : p < 10 ? p : (p ^ 1); }
constexpr uint32_t cls_comp_set(uint32_t set) { return ((set & 1u) << 3) | ((set & 2u) << 1) | ((set & 4u) >> 1) | ((set & 8u) >> 3); }
constexpr bool cls_swap_ok() {
    for (uint32_t set = 1; set < 15; ++set) {
        const int p = cls_word_of_set(set), q = cls_word_of_set(cls_swap_set(set));
        if (cls_swap_set(cls_swap_set(set)) != set) return false;
        if (q != cls_swap_word(p)) return false;                                      // the expected word
        if (cls_mirror(p) != cls_word_of_set(cls_comp_set(set))) return false;        // (the mirror is complementation)
        if (cls_mirror(q) != cls_swap_word(cls_mirror(p))) return false;              // the swap commutes with it
    }
    return true;
}
static_assert(cls_swap_ok(), "A<->C, G<->T swap of a base set: class word and mirror, all 14 sets");
static_assert(cls_word_of_set(cls_swap_set(2)) == 0 && cls_word_of_set(cls_swap_set(4)) == 3,
              "a C slot's canonical base is plane 0 of its tile, the complement plane 3");
constexpr bool cls_heads_ok() {
    int seen = 0;
    for (int w1 = -1; w1 < CLS_LIT_WORDS; ++w1)
        for (int w2 = -1; w2 < CLS_LIT_WORDS; ++w2) {
            if (w2 >= 0 && (w1 < 0 || w2 < w1)) continue;
            const int id = cls_head_id(w1, w2);
            if (id < 0 || id >= CLS_HEADS || cls_head_w1(id) != w1 || cls_head_w2(id) != w2) return false;
            ++seen;
        }
    for (int id = 0; id < CLS_HEADS; ++id)
        if (cls_head_id(cls_head_w1(id), cls_head_w2(id)) != id) return false;
    return seen == CLS_HEADS;                                                         // dense: 36 pairs, 8 singles, none
}
static_assert(cls_heads_ok(), "the 45 head ids and their (w1, w2) round-trip");
// the reverse twin of literal word w = 4 g + p (narrow: GN = 1): plane 3 - p at word-group 2 GN - 1 - g
constexpr bool cls_head_mirror_ok() {
    for (int w = 0; w < CLS_LIT_WORDS; ++w) {
        const int g = w / 4, p = w % 4;
        if (cls_dword(g, p) != w || cls_plane(p) != p || cls_neg(p)) return false;    // a literal word is its dword, positive
        if (cls_mirror(p) != 3 - p || cls_dword(2 * 1 - 1 - g, cls_mirror(p)) != CLS_LIT_WORDS - 1 - w) return false;
    }
    return true;
}
static_assert(cls_head_mirror_ok(), "mirror of a head word: plane 3 - p at word-group 2 GN - 1 - g");
// the lone class as the walk reads it back, beside the word and quad bits; every (word, r), r = 0 excluded as for the head
constexpr bool cls_tail_ok() {
    for (int c = 0; c < CLS_CLASS_WORDS; ++c)
        for (uint32_t r = 1; r < 32; ++r) {
            const uint32_t s = 1u << c | 1u << (CLS_QUAD_BIT + c / 4) | 1u << CLS_ONE_CLASS_BIT | r << CLS_ONE_CLASS_R_BIT;
            int low = 0;
            while (!((s >> low) & 1u)) ++low;                                         // s_ff1
            if (low != c || ((s >> CLS_ONE_CLASS_R_BIT) & 31u) != r || !((s >> (CLS_QUAD_BIT + c / 4)) & 1u)) return false;
        }
    return CLS_QUAD_BIT + (CLS_CLASS_WORDS + 3) / 4 <= CLS_ONE_CLASS_BIT && CLS_ONE_CLASS_R_BIT + 5 <= 32;
}
static_assert(cls_tail_ok(), "the lone-class descriptor: every (word, shift) round-trips beside the summary's word and quad bits");

// Planes is-A / C / G / T, H, L, X (and V when BV) of the code (H, L ^ cm); cm is the wave-uniform flip of the slot, all
// ones for canonical base C, so for a C slot the planes read is-C / A / T / G, H, ~L, ~X.  pack_kernel writes H and L as
// zero at invalid positions; in a boundary chunk the flipped L is masked with V before any plane is derived, so planes
// 1..5 and X are zero there on their own as they are without the flip; plane 0 (~H & ~L) is masked with V.
// BV = false: an all-valid chunk (needs_v == 0: the chunk and the halo are valid) — no V anywhere, a negative
// constraint is acc & ~shift(P).  BV = true: a boundary chunk — a negative constraint is acc & ~shift(P) & shift(V):
// nothing but V keeps an invalid position out of a negative class.  There V takes X's place in the tile and an X
// constraint shifts H and L (shift(X) = shift(H) ^ shift(L)): with V as an eighth plane the body needs 48 plane words
// plus eight temporaries per negative constraint — 91 VGPRs, or 80 and scratch.  A boundary chunk is a contig's first
// or last one, and one constraint in six is on X.
template <class K, bool BV>
struct ClassTile {
    static constexpr bool HAS_V = BV;
    static constexpr int VP = 6;                           // (BV) where V sits
    uint32_t w[7][K::NW];

    __device__ __forceinline__ void expand(const RawChunk<K> &r, const uint32_t cm) {
#pragma unroll
        for (int j = 0; j < K::NW; ++j) {
            const uint32_t hh = r.h[j];
            uint32_t ll = r.l[j] ^ cm;
            // the flipped word is all the tile knows of L: left to fold the flip into the plane expressions, the compiler
            // keeps the raw word beside the flipped one through the boundary body (six registers, and scratch at 80)
            asm("" : "+v"(ll));
            if (BV) ll &= r.v[j];
            w[0][j] = BV ? r.v[j] & ~(hh | ll) : ~(hh | ll);
            w[1][j] = ll & ~hh;
            w[2][j] = hh & ll;
            w[3][j] = hh & ~ll;
            w[4][j] = hh;
            w[5][j] = ll;
            w[6][j] = BV ? r.v[j] : hh ^ ll;
        }
    }
};

// JointWalk over a class program: one scalar walk drives both strands, the reverse twin of class word p is word
// cls_mirror(p) at word-group 2 GN - 1 - g, shift 32 - r (r = 0: word-group 2 GN - g, unshifted).  The class words are
// looked at only behind the summary: not at all for a candidate of literals, in groups of four otherwise.
template <class K, class TileT>
struct ClassWalk {
    uint32_t accf[T_WORDS], accr[T_WORDS];

    template <int G, int P>
    __device__ __forceinline__ void and_one(const TileT &tile, uint32_t (&acc)[T_WORDS], uint32_t r) {
        constexpr int PL = cls_plane(P);
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            uint32_t s;
            if constexpr (TileT::HAS_V && PL == 6) s = alignbit(tile.w[4][t + G + 1], tile.w[4][t + G], r) ^ alignbit(tile.w[5][t + G + 1], tile.w[5][t + G], r);
            else s = alignbit(tile.w[PL][t + G + 1], tile.w[PL][t + G], r);
            if constexpr (!cls_neg(P)) acc[t] &= s;
            else if constexpr (!TileT::HAS_V) acc[t] &= ~s;
            else acc[t] = acc[t] & ~s & alignbit(tile.w[TileT::VP][t + G + 1], tile.w[TileT::VP][t + G], r);
        }
    }
    template <int G, int P, bool R0 = false>
    __device__ __forceinline__ void and_in(const TileT &tile, uint32_t r) {
        constexpr int GR = R0 ? 2 * K::GN - G : 2 * K::GN - 1 - G;
        and_one<G, P>(tile, accf, r);
        and_one<GR, cls_mirror(P)>(tile, accr, R0 ? 0u : 32u - r);
    }
    // a constraint from a tail descriptor: both strands' shifts come with it
    template <int G, int P>
    __device__ __forceinline__ void and_in(const TileT &tile, uint32_t r, uint32_t rr) {
        and_one<G, P>(tile, accf, r);
        and_one<2 * K::GN - 1 - G, cls_mirror(P)>(tile, accr, rr);
    }
    // the leaf of class word c (0..19, counted from dword 9): compares and branches, wave-uniform.
    // Each case passes its accumulators through a comment of its own (pin): left alike, the compiler sinks the ANDs of all
    // cases into one block behind the switch and every leaf hands it eight shifted words in eight more registers.
    template <int I>
    __device__ __forceinline__ void pin() {
        static_assert(T_WORDS == 4, "eight accumulator words");
        asm("; leaf %8" : "+v"(accf[0]), "+v"(accf[1]), "+v"(accf[2]), "+v"(accf[3]), "+v"(accr[0]), "+v"(accr[1]), "+v"(accr[2]), "+v"(accr[3]) : "n"(I));
    }
    __device__ __forceinline__ void class_leaf(uint32_t c, const TileT &tile, uint32_t r, uint32_t rr) {
#define NM_LEAF_CASE(i) case i: and_in<(i) / 10, 4 + (i) % 10>(tile, r, rr); pin<i>(); break;
#define NM_LEAF_CASES5(i) NM_LEAF_CASE(i) NM_LEAF_CASE(i + 1) NM_LEAF_CASE(i + 2) NM_LEAF_CASE(i + 3) NM_LEAF_CASE(i + 4)
        switch (c) {
            NM_LEAF_CASES5(0) NM_LEAF_CASES5(5) NM_LEAF_CASES5(10) NM_LEAF_CASES5(15)
            default: __builtin_unreachable();
        }
#undef NM_LEAF_CASES5
#undef NM_LEAF_CASE
        static_assert(CLS_CLASS_WORDS == 20, "one case per class word");
    }
    template <int G, int P>
    __device__ __forceinline__ void word(uint32_t mm, const TileT &tile) {
        if (JointWalk<K>::template r0_possible<G>() && (mm & 1u)) {     // wave-uniform
            mm &= ~1u;
            and_in<G, P, true>(tile, 0u);
        }
        while (mm) {                                                    // wave-uniform
            const uint32_t r = __builtin_ctz(mm);
            mm &= mm - 1;
            and_in<G, P>(tile, r);
        }
    }
    // the four class words behind summary bits 4 Q .. 4 Q + 3, skipped on the quad's own bit: a one-bit test is s_bitcmp1_b32 +
    // s_cbranch where the four-bit mask is s_and_b32 + s_cmp_eq_u32 + s_cbranch, and a scalar instruction of this walk costs
    // its issue cycle whether a branch is taken or not (profiles/r18/walk_order.md)
    template <int Q>
    __device__ __forceinline__ void quad(const uint32_t (&m)[CLS_PROG_DW], const TileT &tile) {
        if (m[CLS_SUMMARY_DW] & (1u << (CLS_QUAD_BIT + Q))) {           // wave-uniform
            word<(4 * Q + 0) / 10, 4 + (4 * Q + 0) % 10>(m[CLS_WORDS_DW + 4 * Q + 0], tile);
            word<(4 * Q + 1) / 10, 4 + (4 * Q + 1) % 10>(m[CLS_WORDS_DW + 4 * Q + 1], tile);
            word<(4 * Q + 2) / 10, 4 + (4 * Q + 2) % 10>(m[CLS_WORDS_DW + 4 * Q + 2], tile);
            word<(4 * Q + 3) / 10, 4 + (4 * Q + 3) % 10>(m[CLS_WORDS_DW + 4 * Q + 3], tile);
        }
    }
    // no word of these variants has an unshifted constraint: the head (below) has no r = 0 form
    static_assert(K::GN == 1 && !JointWalk<K>::template r0_possible<0>() && !JointWalk<K>::template r0_possible<1>(),
                  "class walks: narrow, the modified position folded");
    // literal word W of a head shifted into place, forward or as its reverse twin (r: that strand's shift)
    template <int W, bool REV>
    __device__ __forceinline__ uint32_t head_word(const TileT &tile, int t, uint32_t r) {
        constexpr int G = REV ? 2 * K::GN - 1 - W / 4 : W / 4, P = REV ? 3 - W % 4 : W % 4;
        return alignbit(tile.w[P][t + G + 1], tile.w[P][t + G], r);
    }
    // acc = canonical plane (& first literal (& second literal)), straight from the tile: no moves, one op per word
    template <int ID>
    __device__ __forceinline__ void head(const TileT &tile, uint32_t r1, uint32_t r2, uint32_t rr1, uint32_t rr2) {
        constexpr int W1 = cls_head_w1(ID), W2 = cls_head_w2(ID);
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {                             // canonical first: plane 0 and its complement
            uint32_t f = tile.w[0][t + K::GN], b = tile.w[3][t + K::GN];
            if constexpr (W1 >= 0) { f &= head_word<W1, false>(tile, t, r1); b &= head_word<W1, true>(tile, t, rr1); }
            if constexpr (W2 >= 0) { f &= head_word<W2, false>(tile, t, r2); b &= head_word<W2, true>(tile, t, rr2); }
            accf[t] = f;
            accr[t] = b;
        }
    }
    __device__ __forceinline__ void walk(const uint32_t (&m)[CLS_PROG_DW], const TileT &tile, const uint32_t (&)[T_WORDS],
                                         const uint32_t (&)[T_WORDS]) {
        const uint32_t r1 = m[CLS_HEAD_FWD_DW], r2 = r1 >> 8;           // (v_alignbit takes the low five bits of a shift)
        const uint32_t rr1 = m[CLS_HEAD_REV_DW], rr2 = rr1 >> 8;
        // dense ids, the plain moves an ordinary case: as `default:` the compiler hoists them in front of the compares
#define NM_HEAD_CASE(i) case i: head<i>(tile, r1, r2, rr1, rr2); break;
#define NM_HEAD_CASES5(i) NM_HEAD_CASE(i) NM_HEAD_CASE(i + 1) NM_HEAD_CASE(i + 2) NM_HEAD_CASE(i + 3) NM_HEAD_CASE(i + 4)
        switch (m[CLS_HEAD_DW]) {                                       // wave-uniform, once per candidate
            NM_HEAD_CASES5(0) NM_HEAD_CASES5(5) NM_HEAD_CASES5(10) NM_HEAD_CASES5(15) NM_HEAD_CASES5(20)
            NM_HEAD_CASES5(25) NM_HEAD_CASES5(30) NM_HEAD_CASES5(35) NM_HEAD_CASES5(40)
            default: __builtin_unreachable();
        }
#undef NM_HEAD_CASES5
#undef NM_HEAD_CASE
        static_assert(CLS_HEADS == 45, "one case per head id");
        if (m[CLS_HEAD_FWD_DW] >> 16) {                                 // wave-uniform: a literal beyond the head
            word<0, 0>(m[0], tile); word<0, 1>(m[1], tile); word<0, 2>(m[2], tile); word<0, 3>(m[3], tile);
            word<1, 0>(m[4], tile); word<1, 1>(m[5], tile); word<1, 2>(m[6], tile); word<1, 3>(m[7], tile);
        }
        if (m[CLS_SUMMARY_DW]) {                                        // wave-uniform: 20 class words skipped at once
            if (m[CLS_SUMMARY_DW] & (1u << CLS_ONE_CLASS_BIT)) {        // exactly one class constraint: its word is the lowest set bit
                const uint32_t r = m[CLS_SUMMARY_DW] >> CLS_ONE_CLASS_R_BIT;
                class_leaf((uint32_t)__builtin_ctz(m[CLS_SUMMARY_DW]), tile, r, 32u - r);
            } else {
                quad<0>(m, tile); quad<1>(m, tile); quad<2>(m, tile); quad<3>(m, tile); quad<4>(m, tile);
            }
        }
    }
};

template <class K>
__device__ __forceinline__ void eval_strand(cu32p prog, const Tile<K> &tile, uint32_t (&acc)[T_WORDS]) {
    uint32_t m[K::PDW];
#pragma unroll
    for (int i = 0; i < K::PDW; ++i) m[i] = prog[i];
    eval_masks<K>(m, tile, acc);
}

// ---- host: one stripped motif -> per-strand constraint masks ---------------------------------------------------------
inline uint32_t comp_mask(uint32_t m) { return ((m & 1) << 3) | ((m & 2) << 1) | ((m & 4) >> 1) | ((m & 8) >> 3); }

// Compile one stripped motif into the per-strand constraint masks of the general path (accumulator starting from all
// ones: the modified position's own constraint is part of the program).  Layout: prog[strand * 48 + gi * 8 + plane],
// gi = floor(d / 32) + 3 (six word-groups: offsets in [-96, 95]), bit r = d mod 32.  *reach_class: 0 when every offset lies
// in [-32, 31], 1 in [-64, 63], 2 beyond (the Variant<G, G, ...> with G = class + 1 reads exactly those groups).
constexpr int PROG6_DW = 96;
inline int compile_program(const uint8_t *masks, uint32_t len, uint32_t modpos, uint32_t *prog, int *reach_class) {
    if (len == 0 || len > NM_MAX_MOTIF_LEN) return fail(NM_ERANGE, "motif length %u outside 1..%d", len, NM_MAX_MOTIF_LEN);
    if (modpos >= len) return fail(NM_EINVAL, "mod_position %u outside motif of length %u", modpos, len);
    memset(prog, 0, PROG6_DW * sizeof(uint32_t));
    bool any = false;
    *reach_class = 0;
    for (uint32_t j = 0; j < len; ++j) {
        const uint32_t m = masks[j] & 15u;
        if (m == 0) return fail(NM_EINVAL, "empty base set at motif position %u", j);
        if (m == 15u) continue;
        any = true;
        for (int strand = 0; strand < 2; ++strand) {
            const int d = strand == 0 ? (int)j - (int)modpos : (int)modpos - (int)j;
            const uint32_t set = strand == 0 ? m : comp_mask(m);
            const int gi = (d >> 5) + 3;                            // arithmetic shift = floor
            const uint32_t r = (uint32_t)d & 31u;
            if (gi < 0 || gi > 5) return fail(NM_ERANGE, "offset %d from the modified base is outside [-96, 95]", d);
            *reach_class = std::max(*reach_class, gi == 0 || gi == 5 ? 2 : gi == 1 || gi == 4 ? 1 : 0);
            uint32_t *row = prog + strand * 48 + gi * 8;
            if (__builtin_popcount(set) == 1) {
                row[__builtin_ctz(set)] |= 1u << r;                 // literal: plane of that base
            } else {
                uint32_t missing = (~set) & 15u;                    // 3-set: one "valid and not x"; 2-set: two of them
                while (missing) {
                    row[4 + __builtin_ctz(missing)] |= 1u << r;
                    missing &= missing - 1;
                }
            }
        }
    }
    if (!any) return fail(NM_EINVAL, "motif has no specified position");
    return NM_OK;
}

// The word-groups Variant<G, G, ...> reads (3 - G .. 2 + G) of a six-group program, as [strand][2 G][8 planes].
inline void slice_program(const uint32_t *full, int G, uint32_t *out) {
    for (int strand = 0; strand < 2; ++strand)
        memcpy(out + strand * 2 * G * 8, full + strand * 48 + (3 - G) * 8, (size_t)2 * G * 8 * sizeof(uint32_t));
}

// ---- candidate records -> constraint programs (nmscan.hip: compile_kernel / common_kernel / compile_common_kernel; nmwindows.hip: the
// speculative children of the search compile their own)
// Compile the staged candidates into constraint programs ON THE DEVICE: one thread per candidate.  A literal is one
// constraint on an is-X plane, a 3-set one on a valid-not-X plane, a 2-set two of those; the reverse strand takes
// the complemented set at the negated offset (motif.py:260-266).  Program layout: [strand][word-group][plane] with
// the word-groups the launched variant reads (narrow: groups 1..2, wide: 0..3) and its planes (np = 4: literal-only
// batch, is-X planes; np = 8); bit r of a word = offset 32 g + r.
// fold_modpos: the modified position's own constraint is left out (compact batches start the accumulator from the
// canonical plane instead).
// prog_slot: where in `programs` the program goes (default: slot k)
__device__ __forceinline__ void compile_one(uint32_t k, const CandRec *__restrict__ rec, const uint8_t *__restrict__ masks,
                                            uint32_t *__restrict__ programs, int wide, int np, int fold_modpos, uint32_t prog_slot = 0xFFFFFFFFu) {
    const int groups = 2 + 2 * wide, g0 = 1 - wide;        // wide: 0 narrow (word-groups 1..2), 1 wide (0..3), 2 extra wide (-1..4)
    const int pdw = 2 * groups * np;
    uint32_t *prog = programs + (size_t)(prog_slot == 0xFFFFFFFFu ? k : prog_slot) * pdw;
    for (int i = 0; i < pdw; ++i) prog[i] = 0;
    const CandRec c = rec[k];
    const uint8_t *m = masks + c.mask_off;
    for (int j = 0; j < c.len; ++j) {
        const uint32_t set_f = m[j] & 15u;
        if (set_f == 15u || (fold_modpos && j == c.modpos)) continue;
        for (int strand = 0; strand < 2; ++strand) {
            const int d = strand == 0 ? j - (int)c.modpos : (int)c.modpos - j;
            const uint32_t set = strand == 0 ? set_f
                                             : (((set_f & 1) << 3) | ((set_f & 2) << 1) | ((set_f & 4) >> 1) | ((set_f & 8) >> 3));
            const int g = (d >> 5) + 2 - g0;
            const uint32_t bit = 1u << ((uint32_t)d & 31u);
            uint32_t *row = prog + (strand * groups + g) * np;
            if (__popc(set) == 1) {
                row[__ffs(set) - 1] |= bit;
            } else {                                    // never reached with np = 4: the host checked the batch
                uint32_t missing = (~set) & 15u;
                while (missing) {
                    row[4 + __ffs(missing) - 1] |= bit;
                    missing &= missing - 1;
                }
            }
        }
    }
}

// The class layout (CLS variants: narrow, compact, so the modified position is folded and offsets lie in [-31, 31]): the
// forward half only, one constraint per set of one, two or three bases, and the summary dword (layout: ClassWalk).
// use_head: the first two literals become the head of the walk; without it every literal stays in its word (id 44).
// tail: CLS_TAIL_CLASS set: a lone class constraint is flagged in the summary; clear: it is found through its quad.
__device__ __forceinline__ void compile_one_classes(uint32_t k, const CandRec *__restrict__ rec, const uint8_t *__restrict__ masks,
                                                    uint32_t *__restrict__ programs, uint32_t c_slots, bool use_head, int tail) {
    uint32_t *prog = programs + (size_t)k * CLS_PROG_DW;
    for (int i = 0; i < CLS_PROG_DW; ++i) prog[i] = 0;
    const CandRec c = rec[k];
    const uint8_t *m = masks + c.mask_off;
    const bool swap = ((c_slots >> c.slot) & 1u) != 0;                      // c_slots: bit s = mod slot s has canonical base C
    uint32_t n_cls = 0, cls_r = 0;
    for (int j = 0; j < c.len; ++j) {
        uint32_t set = m[j] & 15u;
        if (set == 15u || j == c.modpos) continue;
        if (swap) set = cls_swap_set(set);              // the tile of a C slot is built from (H, ~L)
        const int d = j - (int)c.modpos;
        const int g = (d >> 5) + 1;
        if (g < 0 || g > 1) continue;                   // (the host sends no such offset to a narrow variant)
        const int p = cls_word_of_set(set);
        prog[cls_dword(g, p)] |= 1u << ((uint32_t)d & 31u);
        if (p >= 4) {
            prog[CLS_SUMMARY_DW] |= 1u << (10 * g + p - 4) | 1u << (CLS_QUAD_BIT + (10 * g + p - 4) / 4);
            n_cls += 1;
            cls_r = (uint32_t)d & 31u;
        }
    }
    if (n_cls == 1 && (tail & CLS_TAIL_CLASS)) prog[CLS_SUMMARY_DW] |= 1u << CLS_ONE_CLASS_BIT | cls_r << CLS_ONE_CLASS_R_BIT;
    // the head: after the swap, the first two literal constraints in walk order leave their words
    int w1 = -1, w2 = -1;
    uint32_t r1 = 0, r2 = 0, left = 0;
    for (int w = 0; w < CLS_LIT_WORDS; ++w) {
        uint32_t mm = prog[w];
        while (use_head && mm && w2 < 0) {
            const uint32_t r = (uint32_t)__ffs(mm) - 1u;
            mm &= mm - 1;
            if (w1 < 0) { w1 = w; r1 = r; }
            else { w2 = w; r2 = r; }
        }
        prog[w] = mm;
        left |= mm;
    }
    prog[CLS_HEAD_DW] = (uint32_t)cls_head_id(w1, w2);
    prog[CLS_HEAD_FWD_DW] = r1 | r2 << 8 | (left ? 1u << 16 : 0u);
    prog[CLS_HEAD_REV_DW] = ((32u - r1) & 31u) | ((32u - r2) & 31u) << 8;
}

// Light batches (a round of the greedy search): the constraints shared by ALL candidates of a (slot, bin) group — the
// parent of sibling children (find_motifs_bin.py:1116-1135), the motif under its parents in a pruning round
// (:1408-1432) — become the group's COMMON program (index n_prog + group), evaluated once per tile; the candidates keep
// the rest.  One thread per group; groups of 1 or of more than max_group candidates are left alone (range.z = ~0).
// programs: the candidates' programs (global memory, or the LDS copy compile_common_kernel works on); commons: where the
// common program of entry g goes (global memory, program index n_prog + g)
__device__ __forceinline__ void common_one(uint32_t g, uint4 *__restrict__ range, uint32_t *programs, uint32_t *commons, uint32_t pdw,
                                           uint32_t n_prog, uint32_t max_group) {
    uint4 r = range[g];
    r.z = 0xFFFFFFFFu;
    r.w = 0;
    if (r.y >= 2 && r.y <= max_group) {
        uint32_t *common = commons + (size_t)g * pdw;
        uint32_t any = 0;
        for (uint32_t i = 0; i < pdw; ++i) {
            uint32_t c = programs[(size_t)r.x * pdw + i];
            for (uint32_t k = 1; k < r.y; ++k) c &= programs[(size_t)(r.x + k) * pdw + i];
            common[i] = c;
            any |= c;
        }
        if (any) {
            // siblings: every candidate keeps at most ONE constraint per strand -> its program shrinks to two
            // descriptors (mask index << 5 | r; index = dwords per strand when nothing is left) and range.w = 1
            bool single = true;
            const uint32_t sdw = pdw / 2;
            for (uint32_t k = 0; k < r.y; ++k) {
                uint32_t *prog = programs + (size_t)(r.x + k) * pdw;
                for (uint32_t i = 0; i < pdw; ++i) prog[i] &= ~common[i];
                for (uint32_t st = 0; st < 2; ++st) {
                    uint32_t bits = 0;
                    for (uint32_t i = 0; i < sdw; ++i) bits += __popc(prog[st * sdw + i]);
                    if (bits > 1) single = false;
                }
            }
            if (single) {
                for (uint32_t k = 0; k < r.y; ++k) {
                    uint32_t *prog = programs + (size_t)(r.x + k) * pdw;
                    uint32_t desc[2];
                    for (uint32_t st = 0; st < 2; ++st) {
                        desc[st] = sdw << 5;
                        for (uint32_t i = 0; i < sdw; ++i)
                            if (prog[st * sdw + i]) desc[st] = (i << 5) | (uint32_t)(__ffs(prog[st * sdw + i]) - 1);
                    }
                    prog[0] = desc[0];
                    prog[1] = desc[1];
                }
                r.w = 1;
            }
            r.z = n_prog + g;
        }
    }
    range[g] = r;
}


}  // namespace nmdetail

// ---- the scoring kernel ------------------------------------------------------------------------------------------------
// score_kernel and what it is made of, for the two translation units that instantiate it (they define
// NM_SCORE_KERNEL_SOURCE before including this header): nmscan.hip — every variant but the class-plane ones — and
// nmscore_classes.hip, which is nothing but this header with NM_SCORE_CLASSES_UNIT defined and exists because of its
// compiler flags.  They are declared HERE, in the line below that build.py reads, so that the kernel's source and what
// decides its register count and its branches stay in one file:
//
// NM_UNIT_FLAGS nmscore_classes.hip: -fno-slp-vectorize -mllvm -structurizecfg-skip-uniform-regions -mllvm -enable-tail-merge=0
//
// The SLP vectorizer pairs the eight accumulator words of the class walk and, through them, the words of the tile into
// <2 x i32> values; those want aligned register pairs, the halo words get copied into place (v_pk_mov_b32, v_mov_b32), and
// the class variants end at 86 - 94 VGPRs (5 waves per SIMD), or at 80 with scratch when held to 6 waves.  Without that
// pass: 80 VGPRs, no scratch, 6 waves, no copy of a plane word.  The pass cannot be switched off per function.
// The head switch of ClassWalk::walk is a 45-way scalar compare tree whose leaves join in one block.  The structurizer
// runs over uniform control flow as well and turns every level of that join into a flag (s_mov_b64 / s_andn2_b64 vcc, exec /
// s_cbranch_vccnz, 44 per body): measured 4.5 % slower than no head at all.  -structurizecfg-skip-uniform-regions leaves
// uniform regions as compares and branches (74 / 78 VGPRs).  Branch folding then merges the ends of leaves into shared
// tails behind one more taken branch per walk (1 % of the kernel): -enable-tail-merge=0.  profiles/r17/head_pair.md.
// Every other variant keeps the flags and the code it had.
#ifdef NM_SCORE_KERNEL_SOURCE

namespace nmdetail {

struct ScoreArgs {
    Planes seq;
    StatePlanes st[NM_MAX_MOD_SLOTS];
    const uint4 *segments;      // {first chunk, n chunks, bin, 0}; a batch that walks a work list: {first entry, n entries, bin, 0}
    uint32_t n_segments;
    uint32_t split_log2;        // every segment is cut into 1 << split_log2 pieces
    uint32_t pieces_per_run, j_big, fine_log2;   // per run of pieces: the first j_big go whole, the rest in 1 << fine_log2 parts
    uint32_t n_bins;
    const uint4 *cand_range;    // [active_slot_index][bin] -> {begin, count, common program or ~0, -} into programs
    const uint32_t *programs;   // [n_prog][2 * (GN + GP) * NP], sorted by (slot, bin); CLS variants: [n_prog][CLS_PROG_DW], the class layout
    const uint32_t *orig_index; // [n_cand] sorted -> caller order
    unsigned long long *out;    // [n_cand][2]; per-contig mode: [rows][2], row = row_base[candidate] + rank of the contig in its bin
    const uint32_t *chunk_rank; // per chunk: rank of its contig within its bin (per-contig mode)
    const uint64_t *row_base;   // [n_prog] sorted order (per-contig mode)
    uint32_t active_slot[NM_MAX_MOD_SLOTS];
    uint32_t slot_is_c[NM_MAX_MOD_SLOTS];   // canonical base of the slot is C (else A)
    const uint32_t *work_list;  // heavy variants that are not per-contig: the entries the segments index (nmscore_worklist.h),
    const uint32_t *strip_rows; // and the 64 strips of every packed row
};

// the CLS variants (Variant<1, 1, true, 1, false, false, PC, true, PARK>): instantiated by nmscore_classes.hip
// stop: an event bound to the dispatch itself (hipExtLaunchKernelGGL: complete when the kernel is, its time the kernel's end), or NULL
void launch_score_classes(const ScoreArgs &a, uint32_t gx, uint32_t gy, bool per_contig, bool park, hipStream_t s, hipEvent_t stop = nullptr);

}  // namespace nmdetail

namespace {      // (a kernel has internal linkage in the translation unit that instantiates it)

using namespace nmdetail;

// acc = base & (the ONE constraint `desc` = (mask index << 5) | r of a strand): the residual of a sibling child once the
// parent's constraints are in `base`.  The mask index selects registers, so it is dispatched through a switch.
template <class K, int I = 0>
__device__ __forceinline__ void apply_single(uint32_t idx, uint32_t r, const Tile<K> &tile, const uint32_t (&base)[T_WORDS],
                                             uint32_t (&acc)[T_WORDS]) {
    if constexpr (I < K::PDW) {
        if (idx == I) {
            constexpr int g = I / K::NP, p = I % K::NP;
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) acc[t] = base[t] & alignbit(tile.w[p][t + g + 1], tile.w[p][t + g], r);
        } else {
            apply_single<K, I + 1>(idx, r, tile, base, acc);
        }
    } else {
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) acc[t] = base[t];      // idx == PDW: no constraint left on this strand
    }
}

// Candidate k's two counters of this wave: one (candidate, contig) row of the count table (PC), or the lane's LDS slots.
template <class K>
__device__ __forceinline__ void emit_counts(const ScoreArgs &a, uint32_t n_mod, uint32_t n_non, uint32_t k0, uint32_t k,
                                            uint32_t *lds_acc, uint32_t lds_row0, int lane, uint32_t contig_rank) {
    if (K::PC) {
        // per-contig counters (motif_model_contig per contig, find_motifs_bin.py:1285-1331): a chunk lies inside ONE
        // contig, so the wave's sum goes straight to that (candidate, contig) row
        if constexpr (K::CLS) {
            // the sum is wanted in lane 0 only: five ds_swizzle butterflies (the lane pattern is an immediate) and the upper
            // half through v_readlane, where __shfl_xor holds seven lane-index registers through every walk of the chunk
#define NM_SWZ_ADD(o)                                                                         \
            n_mod += (uint32_t)__builtin_amdgcn_ds_swizzle((int)n_mod, ((o) << 10) | 0x1f); \
            n_non += (uint32_t)__builtin_amdgcn_ds_swizzle((int)n_non, ((o) << 10) | 0x1f);
            NM_SWZ_ADD(16) NM_SWZ_ADD(8) NM_SWZ_ADD(4) NM_SWZ_ADD(2) NM_SWZ_ADD(1)
#undef NM_SWZ_ADD
            n_mod += (uint32_t)__builtin_amdgcn_readlane((int)n_mod, 32);
            n_non += (uint32_t)__builtin_amdgcn_readlane((int)n_non, 32);
        } else {
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                n_mod += __shfl_xor(n_mod, o);
                n_non += __shfl_xor(n_non, o);
            }
        }
        if (lane == 0 && (n_mod | n_non)) {
            unsigned long long *row = a.out + (a.row_base[k0 + k] + contig_rank) * 2;
            if (n_mod) atomicAdd(row, (unsigned long long)n_mod);
            if (n_non) atomicAdd(row + 1, (unsigned long long)n_non);
        }
        return;
    }
    atomicAdd(&lds_acc[((k * K::NS + lds_row0) * 2 + 0) * 64 + lane], n_mod);
    atomicAdd(&lds_acc[((k * K::NS + lds_row0) * 2 + 1) * 64 + lane], n_non);
}

// Heavy batches (the non-CF variants): both strands of a candidate from its forward masks (JointWalk, nmscan_device.h), one
// s_load_dwordx16 per candidate.
template <class K, int CAN, class TileT>
__device__ __forceinline__ void score_heavy(const ScoreArgs &a, const TileT &tile, const uint32_t (&sw)[K::NST][T_WORDS],
                                            uint32_t k0, uint32_t nb, uint32_t *lds_acc, uint32_t lds_row0, int lane,
                                            uint32_t contig_rank) {
    constexpr int PF = CAN == 0 ? 0 : 1;   // plane of the canonical base: A or C
    constexpr int PR = CAN == 0 ? 3 : 2;   // plane of its complement:     T or G
    uint32_t basef[T_WORDS], baser[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        // compact batches: the canonical literal at the modified position is left out of the program, the plane is the
        // walk's base
        basef[t] = K::COMPACT ? tile.w[PF][t + K::GN] : 0xFFFFFFFFu;
        baser[t] = K::COMPACT ? tile.w[PR][t + K::GN] : 0xFFFFFFFFu;
    }
    // CLS: the class program (forward half, 32 dwords: two s_load_dwordx16) and its walk over the class planes
    constexpr int MDW = K::CLS ? CLS_PROG_DW : K::PDW;
    static_assert(!K::CLS || CLS_PROG_DW == 2 * K::PDW, "a class program takes the room of both halves of a plain one");
    std::conditional_t<K::CLS, ClassWalk<K, TileT>, JointWalk<K>> jw;
    // PARK: the state words leave their registers here, once per entry, for the thread's own slot behind the counter rows
    // ([plane][threadIdx.x]: a lane reads only what it wrote, and a wave's LDS operations complete in order — no barrier);
    // the compiler barrier keeps the stored registers from being handed to the reads below
    auto park_slot = [&]() { return reinterpret_cast<uint4 *>(lds_acc + K::ROWS * 2 * 64) + threadIdx.x; };
    if constexpr (K::PARK) {
        uint4 *const park = park_slot();
        park[0] = make_uint4(sw[0][0], sw[0][1], sw[0][2], sw[0][3]);
        park[256] = make_uint4(sw[1][0], sw[1][1], sw[1][2], sw[1][3]);
        asm volatile("" ::: "memory");
    }
    // PARK: the next candidate's program is asked for behind the walk instead of at the top of the next one, into the scalar
    // registers the walk has finished with.  Where the two s_load_dwordx16 land is the scheduler's choice: as built (ROCm 7.2) they
    // sink below the reads of the parked words and the finalize, in front of the two ds_add_u32, and the next walk still starts
    // with its s_waitcnt lgkmcnt(0); the finalize waits for the LDS reads alone (profiles/r27/park_state.md: measured, not explained)
    auto fetch_ahead = [&](uint32_t k, uint32_t (&m)[MDW]) {
        typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
        typedef const u32x16 __attribute__((address_space(4))) *cu32x16p;
        const cu32x16p prog = (cu32x16p)(a.programs + (size_t)(k0 + k) * (2 * K::PDW));
        const u32x16 lo = prog[0], hi = prog[1];
#pragma unroll
        for (int i = 0; i < 16; ++i) { m[i] = lo[i]; m[16 + i] = hi[i]; }
    };
    [[maybe_unused]] uint32_t ahead[MDW];
    if constexpr (K::PARK) fetch_ahead(0, ahead);
    for (uint32_t k = 0; k < nb; ++k) {
        cu32p prog = (cu32p)(a.programs + (size_t)(k0 + k) * (2 * K::PDW));
        uint32_t m[MDW];
        if constexpr (K::PARK) {
#pragma unroll
            for (int i = 0; i < MDW; ++i) m[i] = ahead[i];
        } else if constexpr (K::CLS) {     // two loads of 16 dwords each, whatever the walk looks at first
            typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
            typedef const u32x16 __attribute__((address_space(4))) *cu32x16p;
            const u32x16 lo = ((cu32x16p)prog)[0], hi = ((cu32x16p)prog)[1];
#pragma unroll
            for (int i = 0; i < 16; ++i) { m[i] = lo[i]; m[16 + i] = hi[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < MDW; ++i) m[i] = prog[i];
        }
        jw.walk(m, tile, basef, baser);
        // PARK: the words come back behind the walk's last constraint (two ds_read_b128; the barrier keeps them from rising into the walk)
        [[maybe_unused]] uint32_t pw[2][T_WORDS];
        if constexpr (K::PARK) {
            asm volatile("" ::: "memory");
            fetch_ahead(min(k + 1, nb - 1), ahead);
            const uint4 *const park = park_slot();
            const uint4 pm = park[0], pu = park[256];
            pw[0][0] = pm.x; pw[0][1] = pm.y; pw[0][2] = pm.z; pw[0][3] = pm.w;
            pw[1][0] = pu.x; pw[1][1] = pu.y; pw[1][2] = pu.z; pw[1][3] = pu.w;
        }
        auto state = [&](int i, int t) -> uint32_t {           // M (0) or U (1) of word t
            if constexpr (K::PARK) return pw[i][t];
            else return sw[i][t];
        };
        uint32_t n_mod = 0, n_non = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            if (K::COMPACT) {
                const uint32_t sites = jw.accf[t] | jw.accr[t];  // forward sites sit on the canonical base, reverse on its complement
                n_mod += __popc(sites & state(0, t));
                n_non += __popc(sites & state(1, t));
                // CLS: v_bcnt_u32_b32 adds to its second operand; pinned between the words the two counters stay two chains
                // of four v_bcnt (left alone the compiler sums each counter as a tree and joins it with a v_add3_u32)
                if constexpr (K::CLS) { asm("" : "+v"(n_mod)); asm("" : "+v"(n_non)); }
            } else {
                n_mod += __popc(jw.accf[t] & sw[0][t]) + __popc(jw.accr[t] & sw[K::COMPACT ? 0 : 2][t]);
                n_non += __popc(jw.accf[t] & sw[1][t]) + __popc(jw.accr[t] & sw[K::COMPACT ? 1 : 3][t]);
            }
        }
        emit_counts<K>(a, n_mod, n_non, k0, k, lds_acc, lds_row0, lane, contig_rank);
    }
}

// One slot's candidates [k0, k0 + nb) against the tile this wave holds: match masks, site counts, per-lane counts into
// LDS rows k * NS + lds_row0 (lds_row0 = the slot's index in the workgroup).  CAN: canonical base of the slot, 0 = A (reverse-strand sites sit on T), 1 = C (reverse on G).
// common != ~0u: program index of the constraints shared by all nb candidates (their own programs hold the rest).
template <class K, int CAN, class TileT>
__device__ __forceinline__ void score_candidates(const ScoreArgs &a, const TileT &tile, const uint32_t (&sw)[K::NST][T_WORDS],
                                                 uint32_t k0, uint32_t nb, uint32_t common, bool siblings, uint32_t *lds_acc,
                                                 uint32_t lds_row0, int lane, uint32_t contig_rank = 0) {
    if constexpr (!K::CF) {
        score_heavy<K, CAN>(a, tile, sw, k0, nb, lds_acc, lds_row0, lane, contig_rank);
        return;
    } else {
    constexpr int PF = CAN == 0 ? 0 : 1;   // plane of the canonical base: A or C
    constexpr int PR = CAN == 0 ? 3 : 2;   // plane of its complement:     T or G
    uint32_t basef[T_WORDS], baser[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        // compact batches: every candidate has the canonical literal at its modified position, the compiler leaves
        // that constraint out of the program and it becomes the accumulator's initial value
        basef[t] = K::COMPACT ? tile.w[PF][t + K::GN] : 0xFFFFFFFFu;
        baser[t] = K::COMPACT ? tile.w[PR][t + K::GN] : 0xFFFFFFFFu;
    }
    if (common != 0xFFFFFFFFu) {                                             // wave-uniform
        cu32p prog = (cu32p)(a.programs + (size_t)common * (2 * K::PDW));
        eval_strand<K>(prog, tile, basef);
        eval_strand<K>(prog + K::PDW, tile, baser);
    }
    // Scalar loads of the masks are software-pipelined at strand granularity: the reverse masks of candidate k are
    // requested before its forward strand is evaluated, the forward masks of candidate k + 1 before its reverse strand —
    // two sets of SGPRs like before, but a load's latency hides behind ~40 vector instructions instead of standing in
    // front of every strand.
    uint32_t mf[K::PDW], mr[K::PDW];
    if (!siblings) {
        cu32p prog = (cu32p)(a.programs + (size_t)k0 * (2 * K::PDW));
#pragma unroll
        for (int i = 0; i < K::PDW; ++i) mf[i] = prog[i];
    }
    for (uint32_t k = 0; k < nb; ++k) {
        cu32p prog = (cu32p)(a.programs + (size_t)(k0 + k) * (2 * K::PDW));
        uint32_t accf[T_WORDS], accr[T_WORDS];
        if (siblings) {                                                      // wave-uniform: one constraint per strand left
            const uint32_t df = prog[0], dr = prog[1];
            apply_single<K>(df >> 5, df & 31u, tile, basef, accf);
            apply_single<K>(dr >> 5, dr & 31u, tile, baser, accr);
        } else {
#pragma unroll
            for (int i = 0; i < K::PDW; ++i) mr[i] = prog[K::PDW + i];
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) accf[t] = basef[t];
            eval_masks<K>(mf, tile, accf);
            cu32p next = (cu32p)(a.programs + (size_t)(k0 + min(k + 1, nb - 1)) * (2 * K::PDW));
#pragma unroll
            for (int i = 0; i < K::PDW; ++i) mf[i] = next[i];
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) accr[t] = baser[t];
            eval_masks<K>(mr, tile, accr);
        }
        uint32_t n_mod = 0, n_non = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            if (K::COMPACT) {
                const uint32_t sites = accf[t] | accr[t];       // forward sites sit on the canonical base, reverse on its complement
                n_mod += __popc(sites & sw[0][t]);
                n_non += __popc(sites & sw[1][t]);
            } else {
                n_mod += __popc(accf[t] & sw[0][t]) + __popc(accr[t] & sw[K::COMPACT ? 0 : 2][t]);
                n_non += __popc(accf[t] & sw[1][t]) + __popc(accr[t] & sw[K::COMPACT ? 1 : 3][t]);
            }
        }
        emit_counts<K>(a, n_mod, n_non, k0, k, lds_acc, lds_row0, lane, contig_rank);
    }
    }
}

template <class T>
struct TileTag { using type = T; };

// With NS > 1 a tile's sequence planes are loaded and expanded once and serve the candidates of all NS slots (each slot
// brings its own state planes); with NS = 1 the slot comes from blockIdx.y.  A pass handles up to ROWS / NS candidates (ROWS = BMAX but for PARK)
// per slot; LDS rows are [candidate k][slot j].
// One PIECE of work: the chunks [sg.x, sg.x + sg.y) of bin sg.z, all candidates of the workgroup's slot column(s), counters
// accumulated in LDS and flushed to the count table at the end.  Called once per workgroup by score_kernel (piece = a
// segment or a part of one).
template <class K>
__device__ __forceinline__ void score_piece(const ScoreArgs &a, const uint4 sg, const StatePlanes (&stp)[K::NS], const bool (&is_c)[K::NS],
                                            uint32_t *lds_acc, const int lane, const uint32_t wave) {
    constexpr int NS = K::NS;
    constexpr uint32_t H = K::ROWS / NS;
    // the wave's first chunk is requested before anything else of the segment is looked at (candidate ranges, LDS
    // clearing, the barrier): a workgroup lives for four chunks per wave, its start-up chain would otherwise sit
    // in front of every fourth memory round trip
    constexpr bool EARLY = K::CF && K::LIT;          // (the 8-plane light tiles would drop from 5 to 4 waves per SIMD)
    RawChunk<K> first;
    if (EARLY && wave < sg.y) first.load(a.seq, stp, sg.x + wave, lane);
    uint4 range[NS];                                // {first program, candidates, common program or ~0, siblings}
    uint32_t most = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const uint32_t slot_i = NS == 1 ? blockIdx.y : (uint32_t)j;
        range[j] = a.cand_range[(size_t)slot_i * a.n_bins + sg.z];
        range[j].x = __builtin_amdgcn_readfirstlane(range[j].x);
        range[j].y = __builtin_amdgcn_readfirstlane(range[j].y);
        range[j].z = __builtin_amdgcn_readfirstlane(range[j].z);
        range[j].w = __builtin_amdgcn_readfirstlane(range[j].w);
        most = max(most, range[j].y);
    }
    if (most == 0) return;
    // CLS: the flip of the class tile, from the slot's canonical base (a scalar of the workgroup)
    const uint32_t cm = K::CLS ? __builtin_amdgcn_readfirstlane(is_c[0] ? 0xFFFFFFFFu : 0u) : 0u;

    // one chunk of one pass: tile, then every slot's candidates of this pass
    auto score_tile = [&](auto tile_tag, const RawChunk<K> &cur, uint32_t pass0, uint32_t chunk) {
        typename decltype(tile_tag)::type tile;
        if constexpr (K::CLS) tile.expand(cur, cm);
        else tile.expand(cur);
        const uint32_t rank = K::PC ? ((cu32p)a.chunk_rank)[chunk] : 0u;
        // one slot at a time with the slot index a compile-time constant: left to `#pragma unroll`, the optimizer gave up on
        // the NS = 2 non-literal bodies ("loop not unrolled") and indexed cur.s[j] / range[j] / is_c[j] through private
        // memory — 192-288 bytes of scratch per lane in five variants (round-3 review)
        auto one_slot = [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (range[j].y <= pass0) return;                         // wave-uniform
            const uint32_t nbj = min(H, range[j].y - pass0);
            if constexpr (K::CLS)          // (one body: the tile is flipped so that plane 0 is the slot's canonical base)
                score_candidates<K, 0>(a, tile, cur.s[j], range[j].x + pass0, nbj, range[j].z, range[j].w != 0, lds_acc, j, lane, rank);
            else if (K::COMPACT && is_c[j])
                score_candidates<K, 1>(a, tile, cur.s[j], range[j].x + pass0, nbj, range[j].z, range[j].w != 0, lds_acc, j, lane, rank);
            else
                score_candidates<K, 0>(a, tile, cur.s[j], range[j].x + pass0, nbj, range[j].z, range[j].w != 0, lds_acc, j, lane, rank);
        };
        one_slot(std::integral_constant<int, 0>{});
        if constexpr (NS > 1) one_slot(std::integral_constant<int, 1>{});
        static_assert(NS <= 2, "slot fusion is written for one or two slots");
    };
    // CLS: two bodies, chosen per chunk by the wave-uniform needs_v byte the load already read — the all-valid chunk
    // never looks at V, the boundary chunk (a contig's first and last) holds V where the other holds X
    auto score_chunk = [&](const RawChunk<K> &cur, uint32_t pass0, uint32_t chunk) {
        if constexpr (K::CLS) {
            if (cur.need_v) score_tile(TileTag<ClassTile<K, true>>{}, cur, pass0, chunk);
            else score_tile(TileTag<ClassTile<K, false>>{}, cur, pass0, chunk);
        } else {
            score_tile(TileTag<Tile<K>>{}, cur, pass0, chunk);
        }
    };
    auto clear_rows = [&](uint32_t rows_hi) {
        if (K::PC) return;
        for (uint32_t i = threadIdx.x; i < rows_hi * 128; i += 256) lds_acc[i] = 0;
        __syncthreads();
    };
    // 4 threads per counter, 16 lane-slots each, then a 4-lane butterfly; one 64-bit atomic per counter
    auto flush_rows = [&](uint32_t rows_hi, uint32_t pass0) {
        if (K::PC) return;
        __syncthreads();
        uint32_t first_idx = threadIdx.x;
        // the class kernels sit at their 80 registers: hoisted out of the segment loop, the row and the address a thread
        // flushes to stay live through every walk and go to scratch; behind this they are worked out here, once a flush
        if constexpr (K::CLS) asm volatile("" : "+v"(first_idx));
        for (uint32_t idx = first_idx; idx < rows_hi * 8; idx += 256) {
            const uint32_t i = idx >> 2, q = idx & 3;               // i = counter row: (k * NS + j) * 2 + which
            const uint32_t j = (i >> 1) % NS, k = (i >> 1) / NS;
            uint32_t s = 0;
#pragma unroll 4
            for (int jj = 0; jj < 16; ++jj) s += lds_acc[i * 64 + q * 16 + jj];
            // PARK: the lane pattern of a swizzle is an immediate, where __shfl_xor holds the lane index through every walk (in
            // scratch at 72 registers).  The only reason for the second path is that register: if the PARK kernel no longer
            // compiles to 72 VGPRs without scratch (73 is 6 waves: the unparked kernel plus an LDS round trip a walk), look here first
            if constexpr (K::PARK) {
                s += (uint32_t)__builtin_amdgcn_ds_swizzle((int)s, (1 << 10) | 0x1f);
                s += (uint32_t)__builtin_amdgcn_ds_swizzle((int)s, (2 << 10) | 0x1f);
            } else {
                s += __shfl_xor(s, 1);
                s += __shfl_xor(s, 2);
            }
            if (q == 0 && s) {
                uint4 rj = range[0];
#pragma unroll
                for (int t = 1; t < NS; ++t)
                    if (j == (uint32_t)t) rj = range[t];
                if (pass0 + k < rj.y) {
                    const uint32_t orig = a.orig_index[rj.x + pass0 + k];
                    atomicAdd(a.out + (size_t)orig * 2 + (i & 1), (unsigned long long)s);
                }
            }
        }
        __syncthreads();
    };
    // LDS rows in use in a pass: row = k * NS + j for candidate k of slot j
    uint32_t pass0 = 0;
    if (EARLY) {                                                     // pass 0 with the chunk already under way
        const uint32_t rows_hi = NS * min(H, most);
        clear_rows(rows_hi);
        if (wave < sg.y) score_chunk(first, 0, sg.x + wave);
        for (uint32_t ck = wave + 4; ck < sg.y; ck += 4) {
            RawChunk<K> cur;
            cur.load(a.seq, stp, sg.x + ck, lane);
            score_chunk(cur, 0, sg.x + ck);
        }
        flush_rows(rows_hi, 0);
        pass0 = H;
    }
    constexpr bool LIST = !K::CF && !K::PC;          // sg is a range of work-list entries (one scalar load each, where the needs_v byte was)
    for (; pass0 < most; pass0 += H) {
        const uint32_t rows_hi = NS * min(H, most - pass0);
        clear_rows(rows_hi);
        for (uint32_t ck = wave; ck < sg.y; ck += 4) {
            RawChunk<K> cur;
            // PARK: what the loads derive from the lane (its word offset, its place in a packed row) is worked out per entry;
            // hoisted, it stays live through every walk of the segment and goes to scratch.  Compiler-dependent like the swizzles
            // of flush_rows: after a compiler change check 72 VGPRs, ScratchSize 0, Occupancy 7 in the resource-usage remark
            int load_lane = lane;
            if constexpr (K::PARK) asm volatile("" : "+v"(load_lane));
            if constexpr (LIST) cur.load_entry(a.seq, stp, ((cu32p)a.work_list)[sg.x + ck], a.strip_rows, load_lane);
            else cur.load(a.seq, stp, sg.x + ck, load_lane);
            score_chunk(cur, pass0, LIST ? 0u : sg.x + ck);
        }
        flush_rows(rows_hi, pass0);
    }
}

// (CLS: a negative constraint of the boundary-chunk body shifts two planes; asked for 6 waves the scheduler keeps its
// temporaries inside the 80 VGPRs of the 8-plane variant, without scratch)
// (PARK: seven; the per-contig twin asked for seven without parking spills)
#define NM_SCORE_BOUNDS __launch_bounds__(256, (K::GN + K::GP > 2 ? 2 : (K::LIT ? NM_LIT_WAVES : (K::CLS ? (K::PARK ? 7 : 6) : 4))))

// per-slot facts are read from the kernel arguments once per workgroup
#define NM_SLOT_SETUP                                                                                               \
    const int lane = threadIdx.x & 63;                                                                              \
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); /* provably uniform: chunk indices stay scalar */ \
    StatePlanes stp[K::NS];                                                                                         \
    bool is_c[K::NS];                                                                                               \
    _Pragma("unroll") for (int j = 0; j < K::NS; ++j) {                                                             \
        const uint32_t slot = a.active_slot[K::NS == 1 ? blockIdx.y : (uint32_t)j];                                 \
        stp[j] = a.st[slot];                                                                                        \
        is_c[j] = a.slot_is_c[slot] != 0;                                                                           \
    }

template <class K>
__global__ NM_SCORE_BOUNDS void score_kernel(ScoreArgs a) {
    // the counter rows, and behind them the park area of a PARK variant: [2][256] uint4, outside every row a pass clears or flushes
    __shared__ alignas(16) uint32_t lds_acc[K::ROWS * 2 * 64 + (K::PARK ? 2 * 256 * 4 : 0)];
    // the workgroup's piece of the segment table (nmscore_plan.h: plan_block_piece and plan_cut_piece, shared with the host check —
    // the XCD-aware runs, the split and the finer cut of the pieces dispatched last)
    const PlanGrid grid{a.n_segments, a.split_log2, a.pieces_per_run, a.j_big, a.fine_log2};
    uint32_t piece, sub, n_sub;
    if (!plan_block_piece(grid, K::CF, blockIdx.x, &piece, &sub, &n_sub)) return;
    // a heavy variant reads its segment through the constant address space (a scalar load: the workgroup's first dependent read, the
    // candidate range of the segment's bin, starts from an SGPR); a streaming CF variant keeps the vector load it had
    // (profiles/r23/tail_pack.md: neither choice is worth more than the run-to-run spread)
    typedef const uint4 __attribute__((address_space(4))) *cu4p;
    uint4 sg;
    if constexpr (K::CF) sg = a.segments[piece >> a.split_log2];
    else {
        const cu4p seg = (cu4p)a.segments + (piece >> a.split_log2);
        sg.x = seg->x; sg.y = seg->y; sg.z = seg->z; sg.w = 0;
    }
    sg.x = __builtin_amdgcn_readfirstlane(sg.x);   // everything below is wave-uniform: keep it in SGPRs
    sg.y = __builtin_amdgcn_readfirstlane(sg.y);
    sg.z = __builtin_amdgcn_readfirstlane(sg.z);
    if (!plan_cut_piece(grid, piece, sub, n_sub, &sg.x, &sg.y)) return;
    NM_SLOT_SETUP
    score_piece<K>(a, sg, stp, is_c, lds_acc, lane, wave);
}

}  // namespace

#ifdef NM_SCORE_CLASSES_UNIT
namespace nmdetail {

template <class K>
static void launch_classes_variant(const ScoreArgs &a, uint32_t gx, uint32_t gy, hipStream_t s, hipEvent_t stop) {
    if (stop) hipExtLaunchKernelGGL((score_kernel<K>), dim3(gx, gy), dim3(256), 0, s, nullptr, stop, 0, a);
    else hipLaunchKernelGGL((score_kernel<K>), dim3(gx, gy), dim3(256), 0, s, a);
}

void launch_score_classes(const ScoreArgs &a, uint32_t gx, uint32_t gy, bool per_contig, bool park, hipStream_t s, hipEvent_t stop) {
    if (per_contig) launch_classes_variant<Variant<1, 1, true, 1, false, false, true, true>>(a, gx, gy, s, stop);
    else if (park) launch_classes_variant<Variant<1, 1, true, 1, false, false, false, true, true>>(a, gx, gy, s, stop);
    else launch_classes_variant<Variant<1, 1, true, 1, false, false, false, true>>(a, gx, gy, s, stop);
}

}  // namespace nmdetail
#endif  // NM_SCORE_CLASSES_UNIT

#endif  // NM_SCORE_KERNEL_SOURCE
