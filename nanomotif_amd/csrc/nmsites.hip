// Batched per-site export: WHERE every candidate of a batch occurs on the contigs of its bin, and in which state
// (methylated / unmethylated / no call) each occurrence is.  The building block in the reference is
// motif_model_contig(..., save_motif_positions=True) (find_motifs_bin.py:1285-1331: index_meth_fwd / index_nonmeth_fwd /
// index_meth_rev / index_nonmeth_rev, found by utils.py:44-67 subseq_indices); nm_hit_positions serves one (motif, contig,
// array) per call, this unit a whole batch of candidates x every contig of their bins x both strands in a fixed number of
// launches: the count / scan / fill scaffold of nmexport.h, with
//   count  per work item = (candidate, chunk of its bin): load the chunk once, evaluate both strands, count the three
//          disjoint classes acc & M, acc & U, acc & ~(M | U) per strand; the number of records the work item will write
//          goes to its slot of the item table, the six class counts into the (candidate, contig) table
//   fill   a record per occurrence whose state is in state_set; its code is the state, NM_SITES_MINUS on the reverse strand
#include "nmexport.h"

using namespace nmdetail;

namespace {

struct SitesArgs : ExportArgs {
    const uint32_t *cand_row0;           // first row of the candidate in the (candidate, contig) table
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    uint32_t state_set;                  // NM_SITES_MOD | NM_SITES_NOMOD | NM_SITES_NOCALL
    unsigned long long *table;           // count pass: [row][6], may be NULL
};

__device__ __forceinline__ uint32_t pick(uint32_t set, uint32_t m, uint32_t u, uint32_t n) {
    return ((set & 1u) ? m : 0u) | ((set & 2u) ? u : 0u) | ((set & 4u) ? n : 0u);
}

// sites_kernel keeps its prologue and its six-way split written out (not find_occurrences / split_states of nmexport.h): through them its
// count pass carried 4 v_mov_b32, 1 s_branch and 3 v_add3_u32 more and measured about 1 % slower than before; as written here it
// compiles to the instructions it had (profiles/r19/export_prologue.md).
template <int G, bool FILL>
__global__ __launch_bounds__(256) void sites_kernel(SitesArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<FILL>(a, w)) return;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.cand_planes + (size_t)k * 4)};
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
    const uint32_t set = a.state_set;
    if (!FILL) {
        uint32_t c[6] = {0, 0, 0, 0, 0, 0}, n = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            const uint32_t mp = raw.s[0][0][t], up = raw.s[0][1][t] & ~mp, mm = raw.s[0][2][t], um = raw.s[0][3][t] & ~mm;
            const uint32_t fm = af[t] & mp, fu = af[t] & up, fn = af[t] & ~(mp | up);
            const uint32_t rm = ar[t] & mm, ru = ar[t] & um, rn = ar[t] & ~(mm | um);
            c[0] += __popc(fm); c[1] += __popc(fu); c[2] += __popc(fn);
            c[3] += __popc(rm); c[4] += __popc(ru); c[5] += __popc(rn);
            n += __popc(pick(set, fm, fu, fn)) + __popc(pick(set, rm, ru, rn));
        }
        for (int o = 32; o; o >>= 1) {
            n += __shfl_xor(n, o);
#pragma unroll
            for (int j = 0; j < 6; ++j) c[j] += __shfl_xor(c[j], o);
        }
        if (lane == 0) {
            a.item_cnt[w.item] = n;
            if (a.table) {
                unsigned long long *row = a.table + ((size_t)((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk]) * 6;
#pragma unroll
                for (int j = 0; j < 6; ++j)
                    if (c[j]) atomicAdd(row + j, (unsigned long long)c[j]);
            }
        }
        return;
    }
    emit_records(
        a, w, lane,
        [&](int t, uint32_t &f, uint32_t &r) {
            const uint32_t mp = raw.s[0][0][t], up = raw.s[0][1][t] & ~mp, mm = raw.s[0][2][t], um = raw.s[0][3][t] & ~mm;
            f = pick(set, af[t] & mp, af[t] & up, af[t] & ~(mp | up));
            r = pick(set, ar[t] & mm, ar[t] & um, ar[t] & ~(mm | um));
        },
        [&](int t, uint32_t bit, bool minus) {
            const uint32_t m = raw.s[0][minus ? 2 : 0][t], u = raw.s[0][minus ? 3 : 1][t];   // (m first: a position called both ways is methylated)
            return (minus ? (uint32_t)NM_SITES_MINUS : 0u) | ((m & bit) ? 0u : (u & bit) ? 1u : 2u);
        });
}

template <bool FILL>
constexpr ExportKernels<SitesArgs> sites_kernels = {sites_kernel<1, FILL>, sites_kernel<2, FILL>, sites_kernel<3, FILL>};
using SitesBatch = ExportBatch<SitesArgs>;

// validate the batch, compile its programs, stage the tables and enqueue the count pass (and, with_scan, the prefix + gather)
int sites_begin(SitesBatch &sb, nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, const uint64_t *row_offset,
                uint32_t state_set, bool with_scan) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks)) return fail(NM_EINVAL, "NULL argument");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (state_set == 0 || (state_set & ~7u)) return fail(NM_EINVAL, "state_set %u: a non-empty combination of NM_SITES_MOD / NOMOD / NOCALL", state_set);
    if (row_offset && row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
    Staged st;
    const int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, cand_mod_slot, row_offset, false, st, no_check);
    if (rc) return rc;
    SitesArgs &a = sb.base;
    a.state_set = state_set;
    std::vector<ExportTable> reserved;
    if (row_offset) reserved.push_back({&a.table, (size_t)st.rows * 48});
    return export_begin(sb, c, n_cand, cand_bin, st.width.data(), st.programs,
                        {{&a.cand_row0, st.row0.data(), st.row0.size() * 4}, {&a.cand_planes, st.planes.data(), st.planes.size() * 8}}, reserved,
                        sites_kernels<false>, with_scan);
}

}  // namespace

int nm_motif_sites_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                         const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t state_set,
                         const uint64_t *row_offset, uint64_t *cand_total, int64_t *contig_counts) {
    if (!row_offset || (n_cand && (!cand_total || !contig_counts))) return fail(NM_EINVAL, "NULL argument");
    if (n_cand == 0) return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    SitesBatch sb;
    const int rc = sites_begin(sb, c, n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks, row_offset, state_set, false);
    if (rc) return rc;
    const uint64_t rows = row_offset[n_cand];
    if (rows) HIP_TRY(hipMemcpyAsync(contig_counts, sb.base.table, (size_t)rows * 48, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_cand; ++k) {                               // the totals are sums of the table's selected classes
        uint64_t n = 0;
        for (uint64_t r = row_offset[k]; r < row_offset[k + 1]; ++r)
            for (int j = 0; j < 6; ++j)
                if (state_set >> (j % 3) & 1u) n += (uint64_t)contig_counts[r * 6 + j];
        cand_total[k] = n;
    }
    return NM_OK;
}

int nm_motif_sites(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                   const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t state_set,
                   uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                   uint64_t *cand_offset, uint64_t *n_written) {
    if (!cand_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code))) return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (n_cand == 0) {
        cand_offset[0] = 0;
        return c ? NM_OK : fail(NM_EINVAL, "ctx is NULL");
    }
    SitesBatch sb;
    const int rc = sites_begin(sb, c, n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr, state_set, true);
    if (rc) return rc;
    return export_window(sb, sites_kernels<true>, n_cand, first_record, capacity, site_contig, site_pos, site_code, cand_offset, n_written);
}
