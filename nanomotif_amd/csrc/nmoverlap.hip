// How the motifs of one (bin, mod type) RELATE on the sequence: for every candidate of a batch and every contig of its bin, per
// occurrence strand and state (mod / nomod / nocall), its own sites, the sites it shares with each of a list of PARTNER motifs, and
// the rest — its sites that no partner has.  The rest is the number that settles a parent against its children ("how methylated is
// GATC outside RGATCY"): a set difference on the occurrence sets, which no marginal gives.  The reference decides nesting by the
// motifs' spelling only (remove_sub_motifs / merge_motifs, postprocess.py).
// A site is nm_motif_sites' (nmsites.hip): same eval_strand over the same tile, no second matcher.  The count half of the scaffold of
// nmexport.h — no scan, no fill, no records:
//   per work item = (candidate, chunk of its bin) the loads and the two walks of find_occurrences; block 0 is split_states of them.  A
//   work item without an occurrence returns (wave-uniform): every block of it adds nothing.
//   then a wave-uniform loop over the candidate's partners, coverage_kernel's second walk: the partner's accumulators start from the
//   owner's occurrences instead of all ones, so one walk per strand leaves the INTERSECTION; any |= it.  The partner programs are
//   wave-uniform and come through the scalar cache.  A partner that shares nothing in the chunk — the usual case for unrelated motifs
//   — is found by one ballot and skips the six popcounts, the fold over the wave and the atomics.
//   the rest block is the owner's occurrences & ~any.
// A candidate runs at the width (word-groups G = 1, 2, 3 either side of the modified base) of the widest among itself and its partners,
// every program sliced to that width: at most 3 launches whatever the call holds.  Rows are per (block, contig): a contig of several
// chunks takes contributions from several work items, hence 64-bit atomics from lane 0, one per non-zero counter.
#include "nmexport.h"

using namespace nmdetail;

namespace {

struct OverlapArgs : ExportArgs {
    const uint32_t *cand_row0;               // first row of the candidate in the table
    const uint32_t *cand_stride;             // rows of one block of the candidate = resident contigs of its bin
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    const uint32_t *cand_part0;              // [n_cand + 1] first partner of a candidate
    const uint32_t *part_programs;           // [n_part][PROG6_DW] sliced to the width the partner's candidate runs at
    uint32_t n_rows;                         // rows of the table
    unsigned long long *table;               // [n_rows][6]
};

// the six state counts of the occurrences xf ('+') / xr ('-') of the work item added to `row` (wave-uniform)
__device__ __forceinline__ void add_block(const OverlapArgs &a, uint32_t row, int lane, const uint32_t (&s)[4][T_WORDS], const uint32_t (&xf)[T_WORDS],
                                          const uint32_t (&xr)[T_WORDS]) {
    uint32_t c[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t f[3], r[3];
        split_states(s, t, xf[t], xr[t], f, r);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            c[i] += __popc(f[i]);
            c[3 + i] += __popc(r[i]);
        }
    }
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) c[j] += __shfl_xor(c[j], o);
    }
    if (lane == 0 && row < a.n_rows) {
        unsigned long long *out = a.table + (size_t)row * 6;
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (c[j]) atomicAdd(out + j, (unsigned long long)c[j]);
    }
}

template <int G>
__global__ __launch_bounds__(256) void overlap_kernel(OverlapArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<false>(a, w)) return;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.cand_planes + (size_t)k * 4)};
    RawChunk<K> raw;
    Tile<K> tile;
    uint32_t af[T_WORDS], ar[T_WORDS];
    find_occurrences<K>(a, w, stp, lane, raw, tile, af, ar);
    uint32_t own = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) own |= af[t] | ar[t];
    if (__ballot(own != 0) == 0) return;                                 // wave-uniform: no occurrence in this chunk, no block gains anything
    const uint32_t stride = ((cu32p)a.cand_stride)[k], row0 = ((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk];
    const uint32_t p0 = ((cu32p)a.cand_part0)[k], p1 = ((cu32p)a.cand_part0)[k + 1];
    add_block(a, row0, lane, raw.s[0], af, ar);
    uint32_t anyf[T_WORDS], anyr[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) anyf[t] = anyr[t] = 0u;
    uint32_t row = row0;
    for (uint32_t q = p0; q < p1; ++q) {                                 // wave-uniform
        row += stride;
        uint32_t xf[T_WORDS], xr[T_WORDS];                               // (start from the owner's occurrences: the walk leaves the intersection)
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) { xf[t] = af[t]; xr[t] = ar[t]; }
        const cu32p prog = (cu32p)(a.part_programs + (size_t)q * PROG6_DW);
        eval_strand<K>(prog, tile, xf);
        eval_strand<K>(prog + K::PDW, tile, xr);
        uint32_t hit = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            anyf[t] |= xf[t];
            anyr[t] |= xr[t];
            hit |= xf[t] | xr[t];
        }
        if (__ballot(hit != 0) == 0) continue;                           // nothing shared in this chunk: the common case
        add_block(a, row, lane, raw.s[0], xf, xr);
    }
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) { anyf[t] = af[t] & ~anyf[t]; anyr[t] = ar[t] & ~anyr[t]; }
    add_block(a, row + stride, lane, raw.s[0], anyf, anyr);
}

constexpr ExportKernels<OverlapArgs> overlap_kernels = {overlap_kernel<1>, overlap_kernel<2>, overlap_kernel<3>};
using OverlapBatch = ExportBatch<OverlapArgs>;

}  // namespace

int nm_motif_overlap_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                           const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, const uint32_t *cand_partner_offset,
                           const uint8_t *part_len, const uint8_t *part_modpos, const uint32_t *part_mask_offset, const uint8_t *part_masks,
                           const uint64_t *cand_row0, int64_t *counts) {
    if (!cand_row0 || !cand_partner_offset ||
        (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !counts)))
        return fail(NM_EINVAL, "NULL argument");
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) return NM_OK;
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    const Motifs partners{part_len, part_modpos, part_mask_offset, part_masks};
    std::vector<uint8_t> part_width(n_cand, 0);                            // widest reach class among a candidate's partners
    // the unit's check, between the mod slot and the candidate's own program: the partner prefix, P_k, the partners' programs in order
    auto check = [&](uint32_t k, uint32_t, uint64_t &need) {
        if (k == 0 && cand_partner_offset[0] != 0) return fail(NM_EINVAL, "cand_partner_offset[0] must be 0");
        const uint32_t q0 = cand_partner_offset[k], q1 = cand_partner_offset[k + 1];
        if (q1 < q0) return fail(NM_EINVAL, "candidate %u: cand_partner_offset descends (%u after %u)", k, q1, q0);
        if (q1 - q0 > NM_OVERLAP_MAX_PARTNERS)
            return fail(NM_EINVAL, "candidate %u: %u partners, above NM_OVERLAP_MAX_PARTNERS = %d", k, q1 - q0, NM_OVERLAP_MAX_PARTNERS);
        if (q1 > q0 && (!part_len || !part_modpos || !part_mask_offset || !part_masks)) return fail(NM_EINVAL, "NULL argument (partners)");
        uint32_t full[PROG6_DW];
        int width = 0, reach = 0;
        for (uint32_t q = q0; q < q1; ++q) {
            if (part_len[q] == 0 || part_len[q] > NM_MAX_MOTIF_LEN)
                return fail(NM_ERANGE, "candidate %u: partner %u: motif length %u outside 1..%d", k, q - q0, (unsigned)part_len[q], NM_MAX_MOTIF_LEN);
            const int rc = compile_motif(partners, q, full, &reach);
            if (rc) return rc;
            width = std::max(width, reach);
        }
        part_width[k] = (uint8_t)width;
        need *= (uint64_t)(q1 - q0) + 2;
        return (int)NM_OK;
    };
    const Candidates cd{n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}};
    Staged st;
    int rc = stage_candidates(c, cd, cand_mod_slot, cand_row0, false, st, check);
    if (rc) return rc;
    const uint64_t rows = st.rows;
    if (rows == 0) return NM_OK;                                          // every candidate in a bin without a contig
    // a candidate and its partners run at the widest reach class among them: every program sliced to THAT width, not to its own
    const uint32_t n_part = cand_partner_offset[n_cand];
    std::vector<uint32_t> part_programs((size_t)n_part * PROG6_DW, 0), stride(n_cand, 0);
    uint32_t full[PROG6_DW];
    int reach = 0;
    for (uint32_t k = 0; k < n_cand; ++k) {
        stride[k] = c->bin_ncontigs[cand_bin[k]];
        const int width = std::max<int>(st.width[k], part_width[k]);
        if (width != st.width[k]) {
            (void)compile_motif(cd.motifs, k, full, &reach);
            std::fill_n(st.programs.data() + (size_t)k * PROG6_DW, PROG6_DW, 0u);
            slice_program(full, width + 1, st.programs.data() + (size_t)k * PROG6_DW);
            st.width[k] = (uint8_t)width;
        }
        for (uint32_t q = cand_partner_offset[k]; q < cand_partner_offset[k + 1]; ++q) {
            (void)compile_motif(partners, q, full, &reach);
            slice_program(full, width + 1, part_programs.data() + (size_t)q * PROG6_DW);
        }
    }
    OverlapBatch ob;
    OverlapArgs &a = ob.base;
    a.n_rows = (uint32_t)rows;
    rc = export_begin(ob, c, n_cand, cand_bin, st.width.data(), st.programs,
                      {{&a.cand_row0, st.row0.data(), st.row0.size() * 4},
                       {&a.cand_stride, stride.data(), stride.size() * 4},
                       {&a.cand_planes, st.planes.data(), st.planes.size() * 8},
                       {&a.cand_part0, cand_partner_offset, (size_t)(n_cand + 1) * 4},
                       {&a.part_programs, part_programs.data(), part_programs.size() * 4}},
                      {{&a.table, (size_t)rows * 48}}, overlap_kernels, false);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(counts, a.table, (size_t)rows * 48, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}
