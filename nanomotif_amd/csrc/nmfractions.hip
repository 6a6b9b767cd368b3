// Read-fraction HISTOGRAMS at motif sites: for every candidate of a batch and every contig of its bin, per strand, how the sites'
// n_modified / n_valid_cov are distributed over n_bins equal bins of [0, 1], with the occurrences, the sum of n_valid_cov and the sum of
// n_modified beside them.  The six exports before this one read the thresholded state planes (mod / nomod / nocall); the number behind
// the class lives in the read statistics of nmmeth.hip, whose other consumer reduces a (motif, contig) to a median and two means.  The
// count half of the scaffold of nmexport.h (no scan, no fill, no records), as nmtracks.hip uses it, joined with the rank lookup of
// nmreadstats_device.h:
//   per work item = (candidate, chunk of its bin) the loads and the two walks of sites_kernel with the PRESENCE planes of the
//   candidate's read-statistics slot in the state slots (cm_scan_kernel's trick); a work item without an occurrence returns
//   (wave-uniform).  A site = an occurrence whose modified base carries a kept record: acc & presence.
// Bin of a site: min(n_bins - 1, n_modified * n_bins / n_valid_cov) in integers — no floating point, the host computes the same.
// Reduction on chip first: every wave owns 2 x n_bins 32-bit counters in LDS (a wave holds at most 8192 sites per strand), the lanes
// walk their site bits, gather the values and add 1 to their bin with an LDS atomic; the three sums per strand go through a shuffle
// tree.  Flush: lane j reads counter j and adds a non-zero one to the (candidate, contig) row with one 64-bit global atomic — a row is
// 2 x (n_bins + 3) x 8 <= 1072 contiguous bytes — and lane 0 adds the sums.  Atomics, not stores: a contig of several chunks takes
// contributions from several work items.  The LDS region is wave-private and waves of a block leave at different places, so there is
// no workgroup barrier: LDS operations of one wave execute in order, a wave-level fence keeps the compiler from moving them.
#include "nmexport.h"
#include "nmreadstats_device.h"

using namespace nmdetail;

namespace {

struct FractionsArgs : ExportArgs {
    const uint32_t *cand_row0;               // first row of the candidate in the table
    const unsigned long long *cand_planes;   // [n_cand][2] presence planes P+ P- of the candidate's read-statistics slot
    const uint32_t *cand_slot;               // [n_cand] that slot: the index into rs
    const RsSlot *rs;                        // [NM_MAX_MOD_SLOTS]
    uint32_t n_bins;                         // NM_FRACTIONS_MIN_BINS..NM_FRACTIONS_MAX_BINS
    uint32_t n_rows;                         // rows of the table
    unsigned long long *table;               // [n_rows][2][n_bins + NM_FRACTIONS_EXTRA]
};

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int G>
__global__ __launch_bounds__(256) void fractions_kernel(FractionsArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    __shared__ uint32_t lds[4][2 * NM_FRACTIONS_MAX_BINS];
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<false>(a, w)) return;
    const uint32_t k = w.owner;
    const unsigned long long *pl = a.cand_planes + (size_t)k * 2;
    const uint32_t *Pp = reinterpret_cast<const uint32_t *>(pl[0]), *Pm = reinterpret_cast<const uint32_t *>(pl[1]);
    const StatePlanes stp[1] = {StatePlanes{nullptr, nullptr, Pp, Pp, Pm, Pm}};
    // (find_occurrences in its two parts: in one piece the kernel allocates 77 VGPRs for 79 at G = 1, profiles/r19/export_prologue.md)
    RawChunk<K> raw;
    raw.load(a.seq, stp, w.chunk, lane);
    Tile<K> tile;
    tile.expand(raw);
    uint32_t acc[2][T_WORDS];
    walk_strands<K>(a.programs + (size_t)k * PROG6_DW, tile, acc[0], acc[1]);
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) any |= acc[0][t] | acc[1][t];
    if (!__any((int)(any != 0))) return;                                 // wave-uniform: no occurrence in this chunk, nothing to add
    const uint32_t nb = a.n_bins;
    const uint32_t contig = ((cu32p)a.chunk_contig)[w.chunk];
    const RsSlot rs = a.rs[((cu32p)a.cand_slot)[k]];
    uint32_t *hist = lds[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];   // this wave's [2][nb] counters
    hist[lane] = 0;
    hist[lane + 64] = 0;
    wave_fence();
    uint32_t occ[2] = {0, 0};
    uint64_t sum_valid[2] = {0, 0}, sum_mod[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint32_t (&pw)[T_WORDS] = raw.s[0][s * 2];
        uint32_t sites[T_WORDS];
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            sites[t] = acc[s][t] & pw[t];
            occ[s] += __popc(acc[s][t]);
        }
        const uint64_t first = first_record_index(pw, rs.base[s], rs.rank[s], contig, w.chunk, lane);
        uint32_t *h = hist + s * nb;
        for_each_site_value(pw, sites, rs.val[s], first, [&](const uint2 v) {
            sum_valid[s] += v.x;
            sum_mod[s] += v.y;
            // n_modified * n_bins / n_valid_cov: in 32 bits whenever the product fits (n_bins <= 64)
            const uint32_t q = v.y < (1u << 26) ? v.y * nb / v.x : (uint32_t)((uint64_t)v.y * nb / v.x);
            atomicAdd(h + (q < nb - 1 ? q : nb - 1), 1u);
        });
    }
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            occ[s] += __shfl_xor(occ[s], o);
            sum_valid[s] += __shfl_xor(sum_valid[s], o);
            sum_mod[s] += __shfl_xor(sum_mod[s], o);
        }
    }
    wave_fence();
    const uint32_t row = ((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk];
    if (row >= a.n_rows) return;
    const uint32_t stride = nb + NM_FRACTIONS_EXTRA;
    unsigned long long *out = a.table + (size_t)row * 2 * stride;
    for (uint32_t j = (uint32_t)lane; j < 2 * nb; j += 64) {
        const uint32_t n = hist[j], s = j >= nb ? 1u : 0u;
        if (n) atomicAdd(out + s * stride + (j - s * nb), (unsigned long long)n);
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned long long *sums = out + s * stride + nb;
            if (occ[s]) atomicAdd(sums, (unsigned long long)occ[s]);
            if (sum_valid[s]) atomicAdd(sums + 1, (unsigned long long)sum_valid[s]);
            if (sum_mod[s]) atomicAdd(sums + 2, (unsigned long long)sum_mod[s]);
        }
    }
}

constexpr ExportKernels<FractionsArgs> fractions_kernels = {fractions_kernel<1>, fractions_kernel<2>, fractions_kernel<3>};
using FractionsBatch = ExportBatch<FractionsArgs>;

}  // namespace

int nm_motif_fractions_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_rs_slot, const uint8_t *cand_len,
                             const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t n_bins,
                             uint64_t *counts) {
    if (n_cand && (!cand_bin || !cand_rs_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !counts))
        return fail(NM_EINVAL, "NULL argument");
    if (n_bins < NM_FRACTIONS_MIN_BINS || n_bins > NM_FRACTIONS_MAX_BINS)
        return fail(NM_EINVAL, "n_bins %u: a number in [%d, %d]", n_bins, NM_FRACTIONS_MIN_BINS, NM_FRACTIONS_MAX_BINS);
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) return NM_OK;
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    std::vector<uint32_t> slots(n_cand, 0);
    std::vector<unsigned long long> planes((size_t)n_cand * 2, 0);
    std::vector<RsSlot> rs(NM_MAX_MOD_SLOTS, RsSlot{});
    Staged st;
    int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, nullptr, nullptr, true, st,
                              [&](uint32_t k, uint32_t, uint64_t &) {                          // the candidate's read-statistics slot
                                  slots[k] = cand_rs_slot[k];
                                  return stage_readstats_slot(c, k, slots[k], rs.data(), planes.data() + (size_t)k * 2);
                              });
    if (rc) return rc;
    const uint64_t rows = st.rows;
    if (rows == 0) return NM_OK;                                          // every candidate in a bin without a contig
    const size_t row_bytes = (size_t)2 * (n_bins + NM_FRACTIONS_EXTRA) * 8;
    FractionsBatch fb;
    FractionsArgs &a = fb.base;
    a.n_bins = n_bins;
    a.n_rows = (uint32_t)rows;
    rc = export_begin(fb, c, n_cand, cand_bin, st.width.data(), st.programs,
                      {{&a.cand_row0, st.row0.data(), st.row0.size() * 4},
                       {&a.cand_planes, planes.data(), planes.size() * 8},
                       {&a.cand_slot, slots.data(), slots.size() * 4},
                       {&a.rs, rs.data(), rs.size() * sizeof(RsSlot)}},
                      {{&a.table, (size_t)rows * row_bytes}}, fractions_kernels, false);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(counts, a.table, (size_t)rows * row_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}
