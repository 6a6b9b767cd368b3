// Methylation profile around a motif's sites: for every occurrence of every candidate of a batch, the state of every position within
// `radius` of its modified base, on both strands and under every target classification of the call.  The four record exports read the
// modified base only (nmstrands.hip: plus ONE shifted position of one slot); this unit answers whether mod_position is the right one,
// whether a call is bleed from the neighbouring base and whether the site belongs to another mod type.
// An occurrence is nm_motif_sites' (nmsites.hip): own modified base at '+' coordinate p, occurrence strand s.  Offset o counts in the
// motif's reading direction, relative strand r: 0 the occurrence's strand, 1 the other.  The probe is (p + o, s ^ r) for s = 0 and
// (p - o, s ^ r) for s = 1; under a target with canonical base B it is mod (methylated plane), nomod (unmethylated and not methylated),
// nocall (neither, and the contig's letter read on the probed strand is B) or other (the rest; derived on the host from the number of
// occurrences).  The count half of the scaffold of nmexport.h — no scan, no fill, no records:
//   per work item = (candidate, chunk of its bin) the sequence planes are loaded once and the constraint program is walked once per
//   strand.  Then, per target (wave-uniform loop over a staged table): T_WORDS + 2 dwords of MP UP MM UM, the lane's four words plus
//   one either side, and the matching words of the tile's is-B / is-complement(B) planes.  A shift of sh positions along '+' is one
//   v_alignbit of two neighbouring registers (radius <= 31), register indices stay static, nothing goes to scratch.  One shift serves
//   offset sh of the '+' occurrences and offset -sh of the '-' ones: X = (MP, UP, is-B) is their same / opposite strand, Y = (MM, UM,
//   is-complement(B)) their opposite / same one.
// The state planes have a zero pad chunk at either end and every contig is followed by GAP_BP invalid positions without a call, so a
// probe past a contig's end finds no state and no letter: other, without a special case.
// Reduction: a wave counts at most 8192 occurrences, two counts share a dword; six dwords per (target, shift) go through the xor
// butterfly and lane 0 adds the non-zero ones to the candidate's row.
#include "nmexport.h"

using namespace nmdetail;

namespace {

struct ProfileArgs : ExportArgs {
    const unsigned long long *target_planes; // [n_targets][4] MP UP MM UM
    const uint32_t *target_base;             // per target 0: canonical base A, 1: C (a dword each: scalar loads)
    uint32_t n_targets, radius;
    unsigned long long *sites;               // [n_cand][2] occurrences on '+', on '-'
    unsigned long long *table;               // [n_cand][n_targets][2 radius + 1][2][2][3]
};

// the lane's T_WORDS words of a plane plus one word either side
struct HaloWords {
    uint32_t w[T_WORDS + 2];
    __device__ __forceinline__ void load(const uint32_t *plane, size_t base) {
        const uint4 q = *reinterpret_cast<const uint4 *>(plane + base);
        w[0] = plane[base - 1];
        w[1] = q.x; w[2] = q.y; w[3] = q.z; w[4] = q.w;
        w[T_WORDS + 1] = plane[base + T_WORDS];
    }
};

// the three counted classes of the probes of `acc` in (m, u, letter): mod, nomod, nocall
__device__ __forceinline__ void count3(uint32_t acc, uint32_t m, uint32_t u, uint32_t letter, uint32_t &c0, uint32_t &c1, uint32_t &c2) {
    c0 += __popc(acc & m);
    c1 += __popc(acc & u & ~m);
    c2 += __popc(acc & letter & ~(m | u));
}

struct TargetWords {
    uint32_t mp[T_WORDS + 2], up[T_WORDS + 2], mm[T_WORDS + 2], um[T_WORDS + 2], lb[T_WORDS + 2], lc[T_WORDS + 2];
};

// One shift of one target: the twelve counts, packed in pairs, reduced over the wave and added to the rows of offset +sh ('+'
// occurrences, row_f) and -sh ('-' occurrences, row_r).  A row = [2 occurrence strands][2 relative strands][3].
template <bool UP>
__device__ __forceinline__ void profile_shift(const TargetWords &x, const uint32_t (&af)[T_WORDS], const uint32_t (&ar)[T_WORDS], uint32_t bits, int lane,
                                              unsigned long long *row_f, unsigned long long *row_r) {
    uint32_t c[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) c[j] = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        const uint32_t mp = shifted<UP>(x.mp, t, bits), up = shifted<UP>(x.up, t, bits), lb = shifted<UP>(x.lb, t, bits);
        const uint32_t mm = shifted<UP>(x.mm, t, bits), um = shifted<UP>(x.um, t, bits), lc = shifted<UP>(x.lc, t, bits);
        count3(af[t], mp, up, lb, c[0], c[1], c[2]);                     // '+' occurrence, same strand
        count3(af[t], mm, um, lc, c[3], c[4], c[5]);                     // '+' occurrence, opposite strand
        count3(ar[t], mm, um, lc, c[6], c[7], c[8]);                     // '-' occurrence, same strand
        count3(ar[t], mp, up, lb, c[9], c[10], c[11]);                   // '-' occurrence, opposite strand
    }
    uint32_t p[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) p[j] = c[j] | (c[j + 6] << 16);           // (a '+' count, the '-' count of the same column)
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) p[j] += __shfl_xor(p[j], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const uint32_t f = p[j] & 0xFFFFu, r = p[j] >> 16;
            if (f) atomicAdd(row_f + j, (unsigned long long)f);
            if (r) atomicAdd(row_r + 6 + j, (unsigned long long)r);
        }
    }
}

template <int G>
__global__ __launch_bounds__(256) void profile_kernel(ProfileArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<false>(a, w)) return;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.target_planes)};           // RawChunk wants a slot: its state words are not used here
    // (the prologue written out, not find_occurrences: through the helper the kernel has the same registers and 7 more instructions, and
    // took 0.8 - 1.2 % longer in four of four runs against the parent, beyond the parent's own spread: profiles/r19/export_prologue.md)
    RawChunk<K> raw;
    raw.load(a.seq, stp, w.chunk, lane);
    Tile<K> tile;
    tile.expand(raw);
    uint32_t af[T_WORDS], ar[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) af[t] = ar[t] = 0xFFFFFFFFu;
    const cu32p prog = (cu32p)(a.programs + (size_t)k * PROG6_DW);
    eval_strand<K>(prog, tile, af);
    eval_strand<K>(prog + K::PDW, tile, ar);
    uint32_t nf = 0, nr = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        nf += __popc(af[t]);
        nr += __popc(ar[t]);
    }
    uint32_t n = nf | (nr << 16);
    for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
    if (n == 0) return;                                                  // wave-uniform: no occurrence in this chunk, nothing to add
    if (lane == 0) {
        if (n & 0xFFFFu) atomicAdd(a.sites + (size_t)k * 2, (unsigned long long)(n & 0xFFFFu));
        if (n >> 16) atomicAdd(a.sites + (size_t)k * 2 + 1, (unsigned long long)(n >> 16));
    }
    const int R = (int)a.radius;
    const uint32_t nt = a.n_targets;
    const size_t base = (size_t)w.chunk * CHUNK_WORDS + (size_t)lane * T_WORDS;
    unsigned long long *cand_rows = a.table + (size_t)k * nt * (2 * R + 1) * 12;
    for (uint32_t ti = 0; ti < nt; ++ti) {                               // wave-uniform
        const StatePlanes sp = slot_planes(a.target_planes + (size_t)ti * 4);
        HaloWords mp, up, mm, um;
        mp.load(sp.MP, base);
        up.load(sp.UP, base);
        mm.load(sp.MM, base);
        um.load(sp.UM, base);
        const bool is_c = ((cu32p)a.target_base)[ti] != 0;               // scalar load
        TargetWords x;
#pragma unroll
        for (int j = 0; j < T_WORDS + 2; ++j) {
            x.mp[j] = mp.w[j];
            x.up[j] = up.w[j];
            x.mm[j] = mm.w[j];
            x.um[j] = um.w[j];
            // is-A / is-T for a target on A, is-C / is-G on C: the words of the tile that lie one word either side of the lane's own
            x.lb[j] = is_c ? tile.w[1][G - 1 + j] : tile.w[0][G - 1 + j];
            x.lc[j] = is_c ? tile.w[2][G - 1 + j] : tile.w[3][G - 1 + j];
        }
        unsigned long long *rows = cand_rows + (size_t)ti * (2 * R + 1) * 12;
        for (int sh = 0; sh <= R; ++sh)
            profile_shift<true>(x, af, ar, (uint32_t)sh, lane, rows + (size_t)(R + sh) * 12, rows + (size_t)(R - sh) * 12);
        for (int sh = -1; sh >= -R; --sh)
            profile_shift<false>(x, af, ar, (uint32_t)(32 + sh), lane, rows + (size_t)(R + sh) * 12, rows + (size_t)(R - sh) * 12);
    }
}

constexpr ExportKernels<ProfileArgs> profile_kernels = {profile_kernel<1>, profile_kernel<2>, profile_kernel<3>};
using ProfileBatch = ExportBatch<ProfileArgs>;

}  // namespace

int nm_motif_profile_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_len, const uint8_t *cand_modpos,
                           const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t n_targets, const uint8_t *target_slot, uint32_t radius,
                           uint64_t *cand_sites, int64_t *counts) {
    if (!target_slot || (n_cand && (!cand_bin || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !cand_sites || !counts)))
        return fail(NM_EINVAL, "NULL argument");
    if (radius > NM_PROFILE_MAX_RADIUS) return fail(NM_EINVAL, "radius %u above NM_PROFILE_MAX_RADIUS = %d", radius, NM_PROFILE_MAX_RADIUS);
    if (n_targets == 0 || n_targets > NM_MAX_MOD_SLOTS) return fail(NM_EINVAL, "n_targets %u outside 1..%d", n_targets, NM_MAX_MOD_SLOTS);
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) return NM_OK;
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    std::vector<unsigned long long> planes((size_t)n_targets * 4, 0);
    std::vector<uint32_t> tbase(n_targets, 0);
    for (uint32_t t = 0; t < n_targets; ++t) {
        const uint32_t slot = target_slot[t];
        const int rc = slot_state_planes(c, "target_slot", t, slot, planes.data() + (size_t)t * 4);
        if (rc) return rc;
        const uint8_t can = c->slots[slot].canonical;
        if (can != 'A' && can != 'C') return fail(NM_ESTATE, "target_slot[%u] = %u: canonical base %u is neither A nor C", t, slot, (unsigned)can);
        tbase[t] = can == 'C';
    }
    Staged st;
    int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, nullptr, nullptr, false, st, no_check);
    if (rc) return rc;
    const size_t row = (size_t)n_targets * (2 * radius + 1) * 12;
    ProfileBatch pb;
    ProfileArgs &a = pb.base;
    a.n_targets = n_targets;
    a.radius = radius;
    rc = export_begin(pb, c, n_cand, cand_bin, st.width.data(), st.programs,
                      {{&a.target_planes, planes.data(), planes.size() * 8}, {&a.target_base, tbase.data(), tbase.size() * 4}},
                      {{&a.sites, (size_t)n_cand * 16}, {&a.table, (size_t)n_cand * row * 8}}, profile_kernels, false);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(cand_sites, a.sites, (size_t)n_cand * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(counts, a.table, (size_t)n_cand * row * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}
