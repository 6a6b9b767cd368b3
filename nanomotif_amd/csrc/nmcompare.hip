// Two-sample comparison: every occurrence of every candidate of a batch, classified by its state in TWO resident mod slots (the
// same assembly sequenced twice: slot A, slot B).  The reference has no counterpart; the nearest is two runs of
// motif_model_contig(..., save_motif_positions=True) (find_motifs_bin.py:1285-1331) joined on the host.  An occurrence and its
// state in a slot are nm_motif_sites' (nmsites.hip); transition t = 3 * state_a + state_b.  The count / scan / fill scaffold of
// nmexport.h, with
//   count  per work item = (candidate, chunk of its bin): the chunk's sequence planes are loaded ONCE and the constraint program is
//          walked ONCE per strand for both samples — only the eight state planes differ; nine disjoint classes per strand go into
//          the (candidate, contig) table, the number of records under transition_set into the work item's slot
//   fill   a record per occurrence whose transition is in transition_set; its code is the transition, NM_COMPARE_MINUS on the
//          reverse strand
#include "nmexport.h"

using namespace nmdetail;

namespace {

struct CompareArgs : ExportArgs {
    const uint32_t *cand_row0;           // first row of the candidate in the (candidate, contig) table
    const unsigned long long *cand_planes;   // [n_cand][8] MP UP MM UM of slot A, then of slot B
    uint32_t transition_set;             // bit t = transition t is exported
    unsigned long long *table;           // count pass: [row][18], may be NULL
};

template <int G, bool FILL>
__global__ __launch_bounds__(256) void compare_kernel(CompareArgs a) {
    using K = Variant<G, G, false, 2, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<FILL>(a, w)) return;
    const uint32_t k = w.owner;
    const unsigned long long *pl = a.cand_planes + (size_t)k * 8;
    const StatePlanes stp[2] = {slot_planes(pl), slot_planes(pl + 4)};
    RawChunk<K> raw;
    Tile<K> tile;
    uint32_t af[T_WORDS], ar[T_WORDS];
    find_occurrences<K>(a, w, stp, lane, raw, tile, af, ar);             // sequence planes once, one walk per strand: both serve both samples
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
            a.item_cnt[w.item] = n;
            if (a.table) {
                unsigned long long *row = a.table + ((size_t)((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk]) * 18;
#pragma unroll
                for (int j = 0; j < 18; ++j)
                    if (c[j]) atomicAdd(row + j, (unsigned long long)c[j]);
            }
        }
        return;
    }
    emit_records(
        a, w, lane,
        [&](int t, uint32_t &f, uint32_t &r) {
            f = pick9(set, af[t], States(raw.s[0][0][t], raw.s[0][1][t]), States(raw.s[1][0][t], raw.s[1][1][t]));
            r = pick9(set, ar[t], States(raw.s[0][2][t], raw.s[0][3][t]), States(raw.s[1][2][t], raw.s[1][3][t]));
        },
        [&](int t, uint32_t bit, bool minus) {
            const int p = minus ? 2 : 0;
            return (minus ? (uint32_t)NM_COMPARE_MINUS : 0u) | transition_of(bit, States(raw.s[0][p][t], raw.s[0][p + 1][t]), States(raw.s[1][p][t], raw.s[1][p + 1][t]));
        });
}

template <bool FILL>
constexpr ExportKernels<CompareArgs> compare_kernels = {compare_kernel<1, FILL>, compare_kernel<2, FILL>, compare_kernel<3, FILL>};
using CompareBatch = ExportBatch<CompareArgs>;

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
    if (row_offset && row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
    std::vector<unsigned long long> planes((size_t)n_cand * 8, 0);
    Staged st;
    const int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, nullptr, row_offset, false, st,
                                    [&](uint32_t k, uint32_t, uint64_t &) {                // the two slots of the candidate
                                        const int ra = slot_state_planes(c, "cand_slot_a", k, cand_slot_a[k], planes.data() + (size_t)k * 8);
                                        return ra ? ra : slot_state_planes(c, "cand_slot_b", k, cand_slot_b[k], planes.data() + (size_t)k * 8 + 4);
                                    });
    if (rc) return rc;
    CompareArgs &a = cb.base;
    a.transition_set = transition_set;
    std::vector<ExportTable> reserved;
    if (row_offset) reserved.push_back({&a.table, (size_t)st.rows * 144});
    return export_begin(cb, c, n_cand, cand_bin, st.width.data(), st.programs,
                        {{&a.cand_row0, st.row0.data(), st.row0.size() * 4}, {&a.cand_planes, planes.data(), planes.size() * 8}}, reserved,
                        compare_kernels<false>, with_scan);
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
    const int rc = compare_begin(cb, c, n_cand, cand_bin, cand_slot_a, cand_slot_b, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr,
                                 transition_set, true);
    if (rc) return rc;
    return export_window(cb, compare_kernels<true>, n_cand, first_record, capacity, site_contig, site_pos, site_code, cand_offset, n_written);
}
