// Per-site READ-FRACTION CHANGE between two pileups: for every candidate of a batch, every occurrence on the contigs of its bin JOINED
// across two read-statistics slots (samples A and B) — which of the two carry a kept record under its modified base, and, where both do,
// in which direction and by how much n_modified / n_valid_cov moved.  nm_motif_compare reads the thresholded state planes and loses the
// fraction behind the class; nm_motif_fractions_count run twice gives the marginals of the joint table; this unit makes the join on the
// device: two independent rank lookups (nmreadstats_device.h) under one occurrence walk, the decision on exact integers, a joint
// histogram reduced in wave-private LDS (as nmfractions.hip) and a record export that carries four gathered values (as nmpileup.hip).
//   per work item = (candidate, chunk of its bin) the prologue of pileup_kernel with the four PRESENCE planes PA+ PB+ PA- PB- in the four
//   state slots; one walk per strand; a work item without an occurrence returns (wave-uniform).  Per strand
//     paired = acc & PA & PB,  only_a = acc & PA & ~PB,  only_b = acc & ~PA & PB,  bare = acc & ~(PA | PB).
//   The samples' value indices advance independently: own rank table, own lanes-before sum, own in-word popcount; every lane makes the
//   four first_record_index calls before the lanes part.
//   judge  (vA, mA), (vB, mB):  x = mB vA, y = mA vB in 64 bits (exact, below 2^62); up x > y, down x < y; SHIFTED iff x != y and
//          1000 |x - y| >= t vA vB — in 64 bits while |x - y| and vA vB stay below 2^54, in 128 bits beyond.  No floating point.
//   count  the joint histogram into this wave's [2][B B] LDS counters with LDS atomics, the twelve sums per strand through a shuffle tree;
//          flush: the lanes stride over the 2 B B counters and add the non-zero ones with 64-bit global atomics, lane 0 adds the sums
//          (atomics, not stores: a contig of several chunks takes several work items).  The records under `select` and t go to the item
//          table, so the count pass gathers too.  Without a table (the sites call) the histogram and the sums are skipped.
//   fill   the paired sites are judged again into one record mask and one direction mask per strand and word; then pileup_kernel<FILL>'s
//          loop with two gathers and four value columns.  A record outside the window writes nothing and gathers nothing.
#include "nmexport.h"
#include "nmreadstats_device.h"

using namespace nmdetail;

namespace {

struct ShiftArgs : ExportArgs {
    const uint32_t *cand_row0;               // first row of the candidate in the (candidate, contig) table
    const unsigned long long *cand_planes;   // [n_cand][4] presence planes PA+ PB+ PA- PB- of the candidate's two read-statistics slots
    const uint32_t *cand_slot;               // [n_cand][2] those slots (A, B): the indices into rs
    const RsSlot *rs;                        // [NM_MAX_MOD_SLOTS]
    uint32_t n_bins;                         // NM_SHIFT_MIN_BINS..NM_SHIFT_MAX_BINS (count call)
    uint32_t permille;                       // min_delta_permille, 0..1000
    uint32_t select;                         // NM_SHIFT_UP | NM_SHIFT_DOWN: the directions that become records
    uint32_t n_rows;                         // rows of the table
    unsigned long long *table;               // count pass: [n_rows][2][n_bins * n_bins + NM_SHIFT_EXTRA], NULL in the sites call
    uint32_t *out_valid_a, *out_mod_a, *out_valid_b, *out_mod_b;   // fill pass: the four gathered columns
};

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Direction and shift of one paired site: 0 equal, NM_SHIFT_UP, NM_SHIFT_DOWN; bit 2 (4) = shifted at t permille.
__device__ __forceinline__ uint32_t judge(const uint2 va, const uint2 vb, uint32_t t) {
    const uint64_t x = (uint64_t)vb.y * va.x, y = (uint64_t)va.y * vb.x;
    if (x == y) return 0u;
    const uint32_t dir = x > y ? (uint32_t)NM_SHIFT_UP : (uint32_t)NM_SHIFT_DOWN;
    const uint64_t d = x > y ? x - y : y - x, vv = (uint64_t)va.x * vb.x;
    bool shifted;
    if (((d | vv) >> 54) == 0) shifted = 1000ull * d >= (uint64_t)t * vv;        // both sides below 2^64
    else shifted = (unsigned __int128)1000u * d >= (unsigned __int128)t * vv;    // up to 2^72
    return dir | (shifted ? 4u : 0u);
}

// min(B - 1, m B / v): in 32 bits whenever the product fits (B <= 16)
__device__ __forceinline__ uint32_t bin_of(const uint2 v, uint32_t nb) {
    const uint32_t q = v.y < (1u << 27) ? v.y * nb / v.x : (uint32_t)((uint64_t)v.y * nb / v.x);
    return q < nb - 1 ? q : nb - 1;
}

// f(t, bit, value in A, value in B) for every paired site of one strand (acc & pa & pb) in ascending position; ia / ib:
// first_record_index of pa / of pb.
template <class F>
__device__ __forceinline__ void for_each_pair(const uint32_t (&acc)[T_WORDS], const uint32_t (&pa)[T_WORDS], const uint32_t (&pb)[T_WORDS], const uint2 *val_a,
                                              const uint2 *val_b, uint64_t ia, uint64_t ib, F f) {
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t x = acc[t] & pa[t] & pb[t];
        while (x) {
            const uint32_t bit = x & (0u - x);
            x &= x - 1;
            f(t, bit, val_a[ia + __popc(pa[t] & (bit - 1u))], val_b[ib + __popc(pb[t] & (bit - 1u))]);
        }
        ia += __popc(pa[t]);
        ib += __popc(pb[t]);
    }
}

template <int G, bool FILL>
__global__ __launch_bounds__(256) void shift_kernel(ShiftArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<FILL>(a, w)) return;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.cand_planes + (size_t)k * 4)};     // PA+ PB+ PA- PB- in the places of MP UP MM UM
    RawChunk<K> raw;
    raw.load(a.seq, stp, w.chunk, lane);
    Tile<K> tile;
    tile.expand(raw);
    uint32_t acc[2][T_WORDS];
    walk_strands<K>(a.programs + (size_t)k * PROG6_DW, tile, acc[0], acc[1]);
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) any |= acc[0][t] | acc[1][t];
    if (!__any((int)(any != 0))) return;                                 // wave-uniform: no occurrence in this chunk, its item count stays 0
    const uint32_t contig = ((cu32p)a.chunk_contig)[w.chunk];
    const RsSlot rsa = a.rs[((cu32p)a.cand_slot)[2 * k]], rsb = a.rs[((cu32p)a.cand_slot)[2 * k + 1]];
    const uint32_t tmin = a.permille, select = a.select;
    // value index of the lane's first record per strand and sample (lane shuffles: every lane calls, before the lanes part)
    uint64_t ia[2], ib[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        ia[s] = first_record_index(raw.s[0][2 * s], rsa.base[s], rsa.rank[s], contig, w.chunk, lane);
        ib[s] = first_record_index(raw.s[0][2 * s + 1], rsb.base[s], rsb.rank[s], contig, w.chunk, lane);
    }
    if constexpr (!FILL) {
        __shared__ uint32_t lds[4][2 * NM_SHIFT_MAX_BINS * NM_SHIFT_MAX_BINS];
        const bool tabled = a.table != nullptr;                          // wave-uniform
        const uint32_t nb = a.n_bins, cells = nb * nb;
        uint32_t *hist = lds[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];   // this wave's [2][cells] counters
        if (tabled) {
            for (uint32_t j = (uint32_t)lane; j < 2 * cells; j += 64) hist[j] = 0;
            wave_fence();
        }
        const uint32_t row = ((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk];
        const uint32_t stride = cells + NM_SHIFT_EXTRA;
        uint32_t n_rec = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t (&pa)[T_WORDS] = raw.s[0][2 * s], (&pb)[T_WORDS] = raw.s[0][2 * s + 1];
            uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};                     // occurrences, paired, only_a, only_b, up, down, shift_up, shift_down
            uint64_t sum[4] = {0, 0, 0, 0};                               // valid_a, mod_a, valid_b, mod_b over the paired sites
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) {
                c[0] += __popc(acc[s][t]);
                c[1] += __popc(acc[s][t] & pa[t] & pb[t]);
                c[2] += __popc(acc[s][t] & pa[t] & ~pb[t]);
                c[3] += __popc(acc[s][t] & ~pa[t] & pb[t]);
            }
            uint32_t *h = hist + s * cells;
            for_each_pair(acc[s], pa, pb, rsa.val[s], rsb.val[s], ia[s], ib[s], [&](int, uint32_t, const uint2 va, const uint2 vb) {
                const uint32_t j = judge(va, vb, tmin);
                n_rec += ((j & 4u) && (j & select)) ? 1u : 0u;
                if (tabled) {
                    sum[0] += va.x; sum[1] += va.y; sum[2] += vb.x; sum[3] += vb.y;
                    c[4] += j & 1u; c[5] += (j >> 1) & 1u;
                    c[6] += (j & 4u) ? (j & 1u) : 0u; c[7] += (j & 4u) ? ((j >> 1) & 1u) : 0u;
                    atomicAdd(h + bin_of(va, nb) * nb + bin_of(vb, nb), 1u);
                }
            });
            if (tabled) {                                                 // wave-uniform
                for (int o = 32; o; o >>= 1) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) c[j] += __shfl_xor(c[j], o);
#pragma unroll
                    for (int j = 0; j < 4; ++j) sum[j] += __shfl_xor(sum[j], o);
                }
                if (lane == 0 && row < a.n_rows) {
                    unsigned long long *sums = a.table + ((size_t)row * 2 + s) * stride + cells;
                    const unsigned long long v[NM_SHIFT_EXTRA] = {c[0], c[1], c[2], c[3], sum[0], sum[1], sum[2], sum[3], c[4], c[5], c[6], c[7]};
#pragma unroll
                    for (int j = 0; j < NM_SHIFT_EXTRA; ++j)
                        if (v[j]) atomicAdd(sums + j, v[j]);
                }
            }
        }
        for (int o = 32; o; o >>= 1) n_rec += __shfl_xor(n_rec, o);
        if (lane == 0) a.item_cnt[w.item] = n_rec;
        if (tabled && row < a.n_rows) {
            wave_fence();
            unsigned long long *out = a.table + (size_t)row * 2 * stride;
            for (uint32_t j = (uint32_t)lane; j < 2 * cells; j += 64) {
                const uint32_t n = hist[j], s = j >= cells ? 1u : 0u;
                if (n) atomicAdd(out + s * stride + (j - s * cells), (unsigned long long)n);
            }
        }
        return;
    } else {
        // the records of the lane: per strand and word the shifted paired sites under select, and which of them go down
        uint32_t rec[2][T_WORDS], down[2][T_WORDS];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) rec[s][t] = down[s][t] = 0;
            for_each_pair(acc[s], raw.s[0][2 * s], raw.s[0][2 * s + 1], rsa.val[s], rsb.val[s], ia[s], ib[s], [&](int t, uint32_t bit, const uint2 va, const uint2 vb) {
                const uint32_t j = judge(va, vb, tmin);
#pragma unroll
                for (int u = 0; u < T_WORDS; ++u) {                       // (no register array is indexed by a variable)
                    if ((j & 4u) && (j & select)) rec[s][u] |= u == t ? bit : 0u;
                    if (j & (uint32_t)NM_SHIFT_DOWN) down[s][u] |= u == t ? bit : 0u;
                }
            });
        }
        // rank of the lane's first record = prefix of the item + records of the lanes before it (emit_records' first half)
        uint32_t mine = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) mine += __popc(rec[0][t]) + __popc(rec[1][t]);
        uint32_t incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        unsigned long long at = w.off0 + (incl - mine) - a.first;       // relative to the window: one unsigned comparison covers both ends
        const uint32_t pos0 = (w.chunk - ((cu32p)a.contig_chunk)[contig]) * (uint32_t)CHUNK_BP + (uint32_t)lane * (T_WORDS * 32);
        auto put = [&](uint32_t pos, uint32_t code, uint32_t pwa, uint32_t pwb, uint32_t bit, const uint2 *val_a, const uint2 *val_b, uint64_t xa, uint64_t xb) {
            if (at < a.capacity) {
                const uint2 va = val_a[xa + __popc(pwa & (bit - 1u))], vb = val_b[xb + __popc(pwb & (bit - 1u))];
                a.out_contig[at] = contig;
                a.out_pos[at] = pos;
                a.out_code[at] = (uint8_t)code;
                a.out_valid_a[at] = va.x;
                a.out_mod_a[at] = va.y;
                a.out_valid_b[at] = vb.x;
                a.out_mod_b[at] = vb.y;
            }
            ++at;
        };
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            const uint32_t f = rec[0][t], r = rec[1][t];
            uint32_t both = f | r;
            while (both) {                                              // ascending position, '+' before '-'
                const uint32_t b = __builtin_ctz(both), bit = 1u << b;
                both &= both - 1;
                const uint32_t pos = pos0 + t * 32 + b;
                if (f & bit) put(pos, (down[0][t] & bit) ? (uint32_t)NM_SHIFT_CODE_DOWN : 0u, raw.s[0][0][t], raw.s[0][1][t], bit, rsa.val[0], rsb.val[0], ia[0], ib[0]);
                if (r & bit)
                    put(pos, (uint32_t)NM_SHIFT_MINUS | ((down[1][t] & bit) ? (uint32_t)NM_SHIFT_CODE_DOWN : 0u), raw.s[0][2][t], raw.s[0][3][t], bit, rsa.val[1], rsb.val[1],
                        ia[1], ib[1]);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                ia[s] += __popc(raw.s[0][2 * s][t]);
                ib[s] += __popc(raw.s[0][2 * s + 1][t]);
            }
        }
    }
}

template <bool FILL>
constexpr ExportKernels<ShiftArgs> shift_kernels = {shift_kernel<1, FILL>, shift_kernel<2, FILL>, shift_kernel<3, FILL>};
using ShiftBatch = ExportBatch<ShiftArgs>;

int check_permille(uint32_t t) {
    if (t > 1000u) return fail(NM_EINVAL, "min_delta_permille %u: a number in [0, 1000]", t);
    return NM_OK;
}

// validate the batch, compile its programs, stage the tables and enqueue the count pass: with n_bins the (candidate, contig) table laid
// out here (*rows: its rows), without (the sites call) the prefix + gather
int shift_begin(ShiftBatch &sb, nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *slot_a, const uint8_t *slot_b, const uint8_t *cand_len,
                const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t n_bins, uint32_t permille, uint32_t select,
                uint64_t *rows) {
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    const bool tabled = n_bins != 0;
    std::vector<uint32_t> slots((size_t)n_cand * 2, 0);
    std::vector<unsigned long long> planes((size_t)n_cand * 4, 0);
    std::vector<RsSlot> rs(NM_MAX_MOD_SLOTS, RsSlot{});
    Staged st;
    const int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, nullptr, nullptr, tabled, st,
                                    [&](uint32_t k, uint32_t, uint64_t &) {                    // the candidate's two read-statistics slots, A first
                                        unsigned long long pa[2], pb[2];
                                        slots[2 * k] = slot_a[k];
                                        slots[2 * k + 1] = slot_b[k];
                                        if (const int r = stage_readstats_slot(c, k, slot_a[k], rs.data(), pa)) return r;
                                        if (const int r = stage_readstats_slot(c, k, slot_b[k], rs.data(), pb)) return r;
                                        unsigned long long *p = planes.data() + (size_t)k * 4;
                                        p[0] = pa[0]; p[1] = pb[0]; p[2] = pa[1]; p[3] = pb[1];
                                        return (int)NM_OK;
                                    });
    if (rc) return rc;
    if (rows) *rows = st.rows;
    if (tabled && st.rows == 0) return NM_OK;                             // every candidate in a bin without a contig
    ShiftArgs &a = sb.base;
    a.n_bins = n_bins;
    a.permille = permille;
    a.select = select;
    a.n_rows = (uint32_t)st.rows;
    std::vector<ExportTable> reserved;
    if (tabled) reserved.push_back({&a.table, (size_t)st.rows * 2 * (n_bins * n_bins + NM_SHIFT_EXTRA) * 8});
    return export_begin(sb, c, n_cand, cand_bin, st.width.data(), st.programs,
                        {{&a.cand_row0, st.row0.data(), st.row0.size() * 4},
                         {&a.cand_planes, planes.data(), planes.size() * 8},
                         {&a.cand_slot, slots.data(), slots.size() * 4},
                         {&a.rs, rs.data(), rs.size() * sizeof(RsSlot)}},
                        reserved, shift_kernels<false>, !tabled);
}

// export_window of nmexport.h with seven columns: the owners' offsets to the host, the window clamped to the call's total, the fill
// pass, and the window's records to the host.
int shift_window(ShiftBatch &sb, uint32_t n_cand, uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                 uint32_t *const (&site_val)[4], uint64_t *cand_offset, uint64_t *n_written) {
    nm_ctx *c = sb.c;
    HIP_TRY(hipMemcpyAsync(cand_offset, sb.d_owner_offset, (size_t)(n_cand + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = cand_offset[n_cand];
    const uint64_t n = first_record >= total ? 0 : std::min<uint64_t>(capacity, total - first_record);
    if (n == 0) return NM_OK;
    uint8_t *d_out = nullptr;                                             // contig | pos | valid_a | mod_a | valid_b | mod_b | code of the window's records
    const size_t col = align16((size_t)n * 4);
    HIP_TRY(dev_malloc(&d_out, 6 * col + (size_t)n));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)dev_free(p); } } guard{d_out, c};
    ShiftArgs a = sb.base;
    a.first = first_record;
    a.capacity = n;
    a.out_contig = reinterpret_cast<uint32_t *>(d_out);
    a.out_pos = reinterpret_cast<uint32_t *>(d_out + col);
    uint32_t **const out_val[4] = {&a.out_valid_a, &a.out_mod_a, &a.out_valid_b, &a.out_mod_b};
    for (int j = 0; j < 4; ++j) *out_val[j] = reinterpret_cast<uint32_t *>(d_out + (2 + j) * col);
    a.out_code = d_out + 6 * col;
    const int rc = sb.launch(shift_kernels<true>, a);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(site_contig, a.out_contig, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_pos, a.out_pos, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    for (int j = 0; j < 4; ++j) HIP_TRY(hipMemcpyAsync(site_val[j], *out_val[j], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_code, a.out_code, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_written = n;
    return NM_OK;
}

}  // namespace

int nm_motif_shift_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_rs_slot_a, const uint8_t *cand_rs_slot_b,
                         const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t n_bins,
                         uint32_t min_delta_permille, uint64_t *counts) {
    if (n_cand && (!cand_bin || !cand_rs_slot_a || !cand_rs_slot_b || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !counts))
        return fail(NM_EINVAL, "NULL argument");
    if (n_bins < NM_SHIFT_MIN_BINS || n_bins > NM_SHIFT_MAX_BINS)
        return fail(NM_EINVAL, "n_bins %u: a number in [%d, %d]", n_bins, NM_SHIFT_MIN_BINS, NM_SHIFT_MAX_BINS);
    if (const int rc = check_permille(min_delta_permille)) return rc;
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) return NM_OK;
    ShiftBatch sb;
    uint64_t rows = 0;
    const int rc = shift_begin(sb, c, n_cand, cand_bin, cand_rs_slot_a, cand_rs_slot_b, cand_len, cand_modpos, cand_mask_offset, cand_masks, n_bins,
                               min_delta_permille, NM_SHIFT_UP | NM_SHIFT_DOWN, &rows);
    if (rc || rows == 0) return rc;
    HIP_TRY(hipMemcpyAsync(counts, sb.base.table, (size_t)rows * 2 * (n_bins * n_bins + NM_SHIFT_EXTRA) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}

int nm_motif_shift_sites(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_rs_slot_a, const uint8_t *cand_rs_slot_b,
                         const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                         uint32_t min_delta_permille, uint32_t select, uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos,
                         uint8_t *site_code, uint32_t *site_valid_a, uint32_t *site_mod_a, uint32_t *site_valid_b, uint32_t *site_mod_b, uint64_t *cand_offset,
                         uint64_t *n_written) {
    if (!cand_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code || !site_valid_a || !site_mod_a || !site_valid_b || !site_mod_b)) ||
        (n_cand && (!cand_bin || !cand_rs_slot_a || !cand_rs_slot_b || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks)))
        return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (const int rc = check_permille(min_delta_permille)) return rc;
    if (select == 0 || (select & ~(uint32_t)(NM_SHIFT_UP | NM_SHIFT_DOWN)))
        return fail(NM_EINVAL, "select %u: a non-empty combination of NM_SHIFT_UP / NM_SHIFT_DOWN", select);
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) {
        cand_offset[0] = 0;
        return NM_OK;
    }
    ShiftBatch sb;
    const int rc = shift_begin(sb, c, n_cand, cand_bin, cand_rs_slot_a, cand_rs_slot_b, cand_len, cand_modpos, cand_mask_offset, cand_masks, 0, min_delta_permille,
                               select, nullptr);
    if (rc) return rc;
    uint32_t *const val[4] = {site_valid_a, site_mod_a, site_valid_b, site_mod_b};
    return shift_window(sb, n_cand, first_record, capacity, site_contig, site_pos, site_code, val, cand_offset, n_written);
}
