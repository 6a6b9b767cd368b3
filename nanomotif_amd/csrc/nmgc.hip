// Motif methylation STRATIFIED BY LOCAL GC CONTENT: for every candidate of a batch and every contig of its bin, per occurrence strand
// and state (mod / nomod / nocall), how the sites are distributed over g = the number of G or C among the W = 2 half + 1 contig letters
// centred on the modified base (g = 0..W; G | C is closed under complement, so g does not depend on the strand).  A site whose window
// leaves the contig or holds a letter that is not A, C, G or T has no g and is counted in one more cell, `edge`.  A noise motif is
// methylated where the local GC is high; a methyltransferase's motif whatever its surroundings.
// An occurrence is nm_motif_sites' (nmsites.hip).  The count half of the scaffold of nmexport.h — no scan, no fill, no records — as
// nmfractions.hip uses it:
//   per work item = (candidate, chunk of its bin) the loads and the two walks of find_occurrences; the match masks are split into
//   three state words per strand; a work item without an occurrence returns (wave-uniform).
// The window sum is NOT a loop over the window per site.  x = the GC plane (is-C | is-G) over the lane's T_WORDS + 2 words (its own
// and one of halo either side, enough for half <= 31), first moved `half` positions up so that a window starts at its site; then the
// sums S1 = x, S2(p) = S1(p) + S1(p + 1), S4(p) = S2(p) + S2(p + 2), ... are built bit-sliced — a sum of up to 2^k is k + 1 words of
// one bit per position each, two of them added with a ripple of full adders, a shift is one v_alignbit per word as in shifted<> — and
// the sum over W positions is put together from the binary digits of W, lowest first: digit k adds S(2^k) at the offset the lower
// digits have covered, so no shift exceeds 31.  The validity plane (the OR of the four letter planes; positions past a contig's end
// and N are in none) goes the same way with AND for +.  Every contig is followed by GAP_BP >= 32 invalid positions: a window never sees
// the neighbouring contig's letters, it meets an invalid position first.  After that a lane walks its site bits and reads the six
// counter bits at the site's position: the cost per site does not depend on W, the cost per work item grows with the digits of W only.
// Reduction on chip first: every wave owns [2][3][W + 2] 32-bit counters in LDS (a wave holds at most 8192 sites per strand); the
// flush is one 64-bit global atomic per non-zero counter into the (candidate, contig) row — atomics, not stores: a contig of several
// chunks takes contributions from several work items.  The LDS region is wave-private and waves of a block leave at different places,
// so there is no workgroup barrier: LDS operations of one wave execute in order, a wave-level fence keeps the compiler from moving them.
#include "nmexport.h"

using namespace nmdetail;

namespace {

constexpr int GC_MAX_W = 2 * NM_GC_MAX_HALF + 1;                    // 63: a sum fits six bit planes
constexpr int GC_BITS = 6;
constexpr int GC_MAX_CELLS = 6 * (GC_MAX_W + 2);                    // [2 strands][3 states][W + 2]
constexpr int GC_NW = T_WORDS + 2;
static_assert(GC_MAX_W < (1 << GC_BITS) && NM_GC_MAX_HALF < 32 && GAP_BP > NM_GC_MAX_HALF, "one halo word either side, six counter bits");

struct GcArgs : ExportArgs {
    const uint32_t *cand_row0;               // first row of the candidate in the table
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    uint32_t half;                           // 0..NM_GC_MAX_HALF
    uint32_t n_rows;                         // rows of the table
    unsigned long long *table;               // [n_rows][2][3][2 half + 2]
};

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// word t of a GC_NW-word plane seen `sh` (0..31) positions further along '+'; beyond the last word there is nothing
__device__ __forceinline__ uint32_t ahead(const uint32_t (&w)[GC_NW], int t, uint32_t sh) {
    return alignbit(t + 1 < GC_NW ? w[t + 1] : 0u, w[t], sh);
}

__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }

// The windowed sum of one plane: cnt[j][t] = bit j of the number of set positions among the W starting at each position of the
// lane's word t of `y` (y[t + 1]..: what lies ahead); W is wave-uniform, every register index static.
__device__ __forceinline__ void window_sum(const uint32_t (&y)[GC_NW], uint32_t W, uint32_t (&cnt)[GC_BITS][T_WORDS]) {
    uint32_t P[GC_BITS][GC_NW];                                           // S(2^k): k + 1 planes in use at step k
#pragma unroll
    for (int j = 0; j < GC_BITS; ++j) {
#pragma unroll
        for (int t = 0; t < GC_NW; ++t) P[j][t] = j == 0 ? y[t] : 0u;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) cnt[j][t] = 0u;
    }
    uint32_t off = 0;                                                     // positions the lower digits of W cover
#pragma unroll
    for (int k = 0; k < GC_BITS; ++k) {
        if (W >> k & 1u) {                                                // cnt (< 2^k, k planes) += S(2^k) at `off` (k + 1 planes)
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) {
                uint32_t carry = 0;
#pragma unroll
                for (int j = 0; j <= k; ++j) {
                    const uint32_t a = j < k ? cnt[j][t] : 0u, b = ahead(P[j], t, off);
                    cnt[j][t] = a ^ b ^ carry;
                    carry = maj3(a, b, carry);
                }
            }
            off += 1u << k;
        }
        if (k + 1 < GC_BITS && (W >> (k + 1)) != 0) {                     // S(2^(k+1))(p) = S(2^k)(p) + S(2^k)(p + 2^k), ascending words in place
#pragma unroll
            for (int t = 0; t < GC_NW; ++t) {
                uint32_t b[GC_BITS], carry = 0;
#pragma unroll
                for (int j = 0; j <= k; ++j) b[j] = ahead(P[j], t, 1u << k);
#pragma unroll
                for (int j = 0; j <= k; ++j) {
                    const uint32_t a = P[j][t];
                    P[j][t] = a ^ b[j] ^ carry;
                    carry = maj3(a, b[j], carry);
                }
                P[k + 1][t] = carry;
            }
        }
    }
}

// The same for "all W positions set": one plane, AND for +.
__device__ __forceinline__ void window_all(const uint32_t (&y)[GC_NW], uint32_t W, uint32_t (&all)[T_WORDS]) {
    uint32_t P[GC_NW];
#pragma unroll
    for (int t = 0; t < GC_NW; ++t) P[t] = y[t];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) all[t] = 0xFFFFFFFFu;
    uint32_t off = 0;
#pragma unroll
    for (int k = 0; k < GC_BITS; ++k) {
        if (W >> k & 1u) {
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) all[t] &= ahead(P, t, off);
            off += 1u << k;
        }
        if (k + 1 < GC_BITS && (W >> (k + 1)) != 0) {
#pragma unroll
            for (int t = 0; t < GC_NW; ++t) P[t] &= ahead(P, t, 1u << k);
        }
    }
}

// y[t] = the plane `x` (x[0]: the halo word below the lane's own) seen from `half` positions ahead of it: bit b of y[t] is the
// position `half` below bit b of the lane's word t; y[T_WORDS], y[T_WORDS + 1]: what follows
__device__ __forceinline__ void window_start(const uint32_t (&x)[GC_NW], uint32_t half, uint32_t (&y)[GC_NW]) {
#pragma unroll
    for (int t = 0; t < GC_NW; ++t) {
        const uint32_t hi = t + 1 < GC_NW ? x[t + 1] : 0u;
        y[t] = half ? alignbit(hi, x[t], 32u - half) : hi;
    }
}

template <int G>
__global__ __launch_bounds__(256) void gc_kernel(GcArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    __shared__ uint32_t lds[4][GC_MAX_CELLS];
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<false>(a, w)) return;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.cand_planes + (size_t)k * 4)};
    RawChunk<K> raw;
    Tile<K> tile;
    uint32_t af[T_WORDS], ar[T_WORDS];
    find_occurrences<K>(a, w, stp, lane, raw, tile, af, ar);
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) any |= af[t] | ar[t];
    if (!__any((int)(any != 0))) return;                                 // wave-uniform: no occurrence in this chunk, nothing to add
    const uint32_t half = a.half, W = 2 * half + 1, stride = W + 2, cells = 6 * stride;
    uint32_t *hist = lds[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];   // this wave's [2][3][W + 2] counters
    for (uint32_t j = (uint32_t)lane; j < cells; j += 64) hist[j] = 0;
    wave_fence();
    // the GC plane and the validity plane over the lane's own words and one either side, moved to the windows' first positions
    uint32_t cnt[GC_BITS][T_WORDS], all[T_WORDS];
    {
        uint32_t gc[GC_NW], valid[GC_NW], y[GC_NW];                       // (both taken before the sums: the tile is dead from here)
#pragma unroll
        for (int j = 0; j < GC_NW; ++j) {
            gc[j] = tile.w[1][G - 1 + j] | tile.w[2][G - 1 + j];
            valid[j] = gc[j] | tile.w[0][G - 1 + j] | tile.w[3][G - 1 + j];
        }
        window_start(valid, half, y);
        window_all(y, W, all);
        window_start(gc, half, y);
        window_sum(y, W, cnt);
    }
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t f[3], r[3];
        split_states(raw.s[0], t, af[t], ar[t], f, r);
        uint32_t both = af[t] | ar[t];
        while (both) {                                                   // cost per site: six bit reads, one or two LDS atomics
            const uint32_t b = __builtin_ctz(both), bit = 1u << b;
            both &= both - 1;
            uint32_t g = 0;
#pragma unroll
            for (int j = 0; j < GC_BITS; ++j) g |= (cnt[j][t] >> b & 1u) << j;
            const uint32_t cell = (all[t] & bit) ? g : W + 1;
            if (af[t] & bit) atomicAdd(hist + ((f[0] & bit) ? 0u : (f[1] & bit) ? 1u : 2u) * stride + cell, 1u);
            if (ar[t] & bit) atomicAdd(hist + (3u + ((r[0] & bit) ? 0u : (r[1] & bit) ? 1u : 2u)) * stride + cell, 1u);
        }
    }
    wave_fence();
    const uint32_t row = ((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk];
    if (row >= a.n_rows) return;
    unsigned long long *out = a.table + (size_t)row * cells;
    for (uint32_t j = (uint32_t)lane; j < cells; j += 64) {
        const uint32_t n = hist[j];
        if (n) atomicAdd(out + j, (unsigned long long)n);
    }
}

constexpr ExportKernels<GcArgs> gc_kernels = {gc_kernel<1>, gc_kernel<2>, gc_kernel<3>};
using GcBatch = ExportBatch<GcArgs>;

}  // namespace

int nm_motif_gc_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                      const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t half,
                      const uint64_t *cand_row0, int64_t *counts) {
    if (!cand_row0 || (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !counts)))
        return fail(NM_EINVAL, "NULL argument");
    if (half > NM_GC_MAX_HALF) return fail(NM_EINVAL, "half %u above NM_GC_MAX_HALF = %d", half, NM_GC_MAX_HALF);
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) return NM_OK;
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    Staged st;
    int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, cand_mod_slot, cand_row0, false, st, no_check);
    if (rc) return rc;
    const uint64_t rows = st.rows;
    if (rows == 0) return NM_OK;                                          // every candidate in a bin without a contig
    const size_t row_bytes = (size_t)6 * (2 * half + 3) * 8;
    GcBatch gb;
    GcArgs &a = gb.base;
    a.half = half;
    a.n_rows = (uint32_t)rows;
    rc = export_begin(gb, c, n_cand, cand_bin, st.width.data(), st.programs,
                      {{&a.cand_row0, st.row0.data(), st.row0.size() * 4}, {&a.cand_planes, st.planes.data(), st.planes.size() * 8}},
                      {{&a.table, (size_t)rows * row_bytes}}, gc_kernels, false);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(counts, a.table, (size_t)rows * row_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}
