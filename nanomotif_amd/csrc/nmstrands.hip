// Both-strand state of a motif site: every occurrence of every candidate of a batch, classified by the state of its OWN modified base
// and by the state of its PARTNER — the modified base the other strand's methyltransferase target carries inside the same site, d
// positions along '+' and on the opposite strand (d = 0: the same position).  modkit has pileup-hemi for CpG; the reference only pairs a
// motif with its complement by name (join_motif_complements) and never looks at the sites.  An occurrence and the state of a
// (position, strand) are nm_motif_sites' (nmsites.hip); pair t = 3 * own + partner.  The count / scan / fill scaffold of nmexport.h, with
//   count  per work item = (candidate, chunk of its bin): the sequence planes and the chunk's own four state planes are loaded once and the
//          constraint program is walked once per strand; the partner's state comes from the OPPOSITE strand's planes shifted by +d
//          (occurrences on '+': MM / UM) or -d (occurrences on '-': MP / UP), nine disjoint classes per strand go into the
//          (candidate, contig) table, the number of records under pair_set into the work item's slot
//   fill   a record per occurrence whose pair is in pair_set; its code is the pair, NM_STRANDS_MINUS on the reverse strand
// The shift is wave-uniform (one candidate per wave): its word part goes into the load address, T_WORDS + 1 dwords per plane, its bit
// part through v_alignbit — register indices stay static, nothing goes to scratch.  The state planes have the sequence planes' layout with
// a zero pad chunk at either end (nm_upload_contigs, alloc_slot_planes) and |d| <= 128 (int8), so the shifted reads stay inside the allocation.
#include "nmexport.h"

using namespace nmdetail;

namespace {

struct StrandsArgs : ExportArgs {
    const uint32_t *cand_row0;           // first row of the candidate in the (candidate, contig) table
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    const int32_t *cand_partner;         // partner offset d of the candidate (a dword each: a scalar load, no vector round trip before the shifted reads)
    uint32_t pair_set;                   // bit t = pair t is exported
    unsigned long long *table;           // count pass: [row][18], may be NULL
};

// T_WORDS words of a plane as seen `shift` positions further along '+': word t holds the positions 32 t + shift .. 32 t + shift + 31 of
// the lane's tile.  `at` = index of the lane's first word plus floor(shift / 32) (wave-uniform part in the address), bits = shift mod 32.
struct ShiftedWords {
    uint32_t w[T_WORDS + 1];
    __device__ __forceinline__ void load(const uint32_t *plane, size_t at) {
#pragma unroll
        for (int j = 0; j <= T_WORDS; ++j) w[j] = plane[at + j];
    }
    __device__ __forceinline__ uint32_t word(int t, uint32_t bits) const { return alignbit(w[t + 1], w[t], bits); }
};

template <int G, bool FILL>
__global__ __launch_bounds__(256) void strands_kernel(StrandsArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<FILL>(a, w)) return;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.cand_planes + (size_t)k * 4)};
    const int d = (int)((cu32p)a.cand_partner)[k];                       // scalar load: wave-uniform
    const int wf = d >> 5, wr = (-d) >> 5;                               // arithmetic shifts = floor
    const uint32_t bf = (uint32_t)d & 31u, br = (uint32_t)(-d) & 31u;
    // the partner's planes first (of '+' occurrences on '-', of '-' ones on '+'): RawChunk::load waits for its needs_v byte before it
    // branches, and what is in flight by then shares that one round trip
    const size_t base = (size_t)w.chunk * CHUNK_WORDS + (size_t)lane * T_WORDS;
    ShiftedWords qfm, qfu, qrm, qru;
    qfm.load(stp[0].MM, base + (ptrdiff_t)wf);
    qfu.load(stp[0].UM, base + (ptrdiff_t)wf);
    qrm.load(stp[0].MP, base + (ptrdiff_t)wr);
    qru.load(stp[0].UP, base + (ptrdiff_t)wr);
    // (the prologue written out, not find_occurrences: through the helper the fill variants allocate other registers — 105 / 117 VGPRs for
    // 106 / 119 at G = 1 / 2, 40 more instructions at G = 3 — and no trace exercises them: profiles/r19/export_prologue.md)
    RawChunk<K> raw;
    raw.load(a.seq, stp, w.chunk, lane);                                 // sequence planes, the chunk's own state words
    Tile<K> tile;
    tile.expand(raw);
    uint32_t af[T_WORDS], ar[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) af[t] = ar[t] = 0xFFFFFFFFu;
    const cu32p prog = (cu32p)(a.programs + (size_t)k * PROG6_DW);
    eval_strand<K>(prog, tile, af);
    eval_strand<K>(prog + K::PDW, tile, ar);
    uint32_t pfm[T_WORDS], pfu[T_WORDS], prm[T_WORDS], pru[T_WORDS];     // partner M / U aligned with the own positions
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        pfm[t] = qfm.word(t, bf);
        pfu[t] = qfu.word(t, bf);
        prm[t] = qrm.word(t, br);
        pru[t] = qru.word(t, br);
    }
    const uint32_t set = a.pair_set;
    if (!FILL) {
        uint32_t c[18], n = 0;
#pragma unroll
        for (int j = 0; j < 18; ++j) c[j] = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            const States fo(raw.s[0][0][t], raw.s[0][1][t]), fp(pfm[t], pfu[t]);
            const States ro(raw.s[0][2][t], raw.s[0][3][t]), rp(prm[t], pru[t]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint32_t fi = af[t] & fo.s[i], ri = ar[t] & ro.s[i];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    c[3 * i + j] += __popc(fi & fp.s[j]);
                    c[9 + 3 * i + j] += __popc(ri & rp.s[j]);
                }
            }
            n += __popc(pick9(set, af[t], fo, fp)) + __popc(pick9(set, ar[t], ro, rp));
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
            f = pick9(set, af[t], States(raw.s[0][0][t], raw.s[0][1][t]), States(pfm[t], pfu[t]));
            r = pick9(set, ar[t], States(raw.s[0][2][t], raw.s[0][3][t]), States(prm[t], pru[t]));
        },
        [&](int t, uint32_t bit, bool minus) {
            return minus ? (uint32_t)NM_STRANDS_MINUS | transition_of(bit, States(raw.s[0][2][t], raw.s[0][3][t]), States(prm[t], pru[t]))
                         : transition_of(bit, States(raw.s[0][0][t], raw.s[0][1][t]), States(pfm[t], pfu[t]));
        });
}

template <bool FILL>
constexpr ExportKernels<StrandsArgs> strands_kernels = {strands_kernel<1, FILL>, strands_kernel<2, FILL>, strands_kernel<3, FILL>};
using StrandsBatch = ExportBatch<StrandsArgs>;

// validate the batch, compile its programs, stage the tables and enqueue the count pass (and, with_scan, the prefix + gather)
int strands_begin(StrandsBatch &sb, nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const int8_t *cand_partner_offset,
                  const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                  const uint64_t *row_offset, uint32_t pair_set, bool with_scan) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_partner_offset || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks))
        return fail(NM_EINVAL, "NULL argument");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (pair_set == 0 || (pair_set & ~NM_STRANDS_ALL))
        return fail(NM_EINVAL, "pair_set %u: a non-empty combination of the bits 0..8 (bit 3 * own state + partner state)", pair_set);
    if (row_offset && row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
    std::vector<int32_t> partner(cand_partner_offset, cand_partner_offset + n_cand);
    Staged st;
    const int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, cand_mod_slot, row_offset, false, st,
                                    [&](uint32_t k, uint32_t, uint64_t &) {
                                        // the partner lies inside the occurrence's span: inside the contig, and no further from the own base than the program reaches
                                        const int at = (int)cand_modpos[k] + partner[k];
                                        if (at >= 0 && at < (int)cand_len[k]) return (int)NM_OK;
                                        return fail(NM_EINVAL, "candidate %u: partner offset %d from mod_position %u lies outside the motif of length %u", k, partner[k],
                                                    (unsigned)cand_modpos[k], (unsigned)cand_len[k]);
                                    });
    if (rc) return rc;
    StrandsArgs &a = sb.base;
    a.pair_set = pair_set;
    std::vector<ExportTable> reserved;
    if (row_offset) reserved.push_back({&a.table, (size_t)st.rows * 144});
    return export_begin(sb, c, n_cand, cand_bin, st.width.data(), st.programs,
                        {{&a.cand_row0, st.row0.data(), st.row0.size() * 4},
                         {&a.cand_planes, st.planes.data(), st.planes.size() * 8},
                         {&a.cand_partner, partner.data(), partner.size() * 4}},
                        reserved, strands_kernels<false>, with_scan);
}

}  // namespace

int nm_motif_strands_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const int8_t *cand_partner_offset,
                           const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                           uint32_t pair_set, const uint64_t *row_offset, uint64_t *cand_total, int64_t *contig_counts) {
    if (!row_offset || (n_cand && (!cand_total || !contig_counts))) return fail(NM_EINVAL, "NULL argument");
    if (n_cand == 0) return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    StrandsBatch sb;
    const int rc = strands_begin(sb, c, n_cand, cand_bin, cand_mod_slot, cand_partner_offset, cand_len, cand_modpos, cand_mask_offset, cand_masks, row_offset,
                                 pair_set, false);
    if (rc) return rc;
    const uint64_t rows = row_offset[n_cand];
    if (rows) HIP_TRY(hipMemcpyAsync(contig_counts, sb.base.table, (size_t)rows * 144, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_cand; ++k) {                               // the totals are sums of the table's selected pairs
        uint64_t n = 0;
        for (uint64_t r = row_offset[k]; r < row_offset[k + 1]; ++r)
            for (int j = 0; j < 18; ++j)
                if (pair_set >> (j % 9) & 1u) n += (uint64_t)contig_counts[r * 18 + j];
        cand_total[k] = n;
    }
    return NM_OK;
}

int nm_motif_strands_sites(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const int8_t *cand_partner_offset,
                           const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                           uint32_t pair_set, uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                           uint64_t *cand_offset, uint64_t *n_written) {
    if (!cand_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code))) return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (n_cand == 0) {
        cand_offset[0] = 0;
        return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    }
    StrandsBatch sb;
    const int rc = strands_begin(sb, c, n_cand, cand_bin, cand_mod_slot, cand_partner_offset, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr,
                                 pair_set, true);
    if (rc) return rc;
    return export_window(sb, strands_kernels<true>, n_cand, first_record, capacity, site_contig, site_pos, site_code, cand_offset, n_written);
}
