// Per-site READ COUNTS at motif sites: for every candidate of a batch, every occurrence on the contigs of its bin as a record that carries
// the n_valid_cov and n_modified of the pileup record under its modified base — the table behind motif_sites' state and behind
// motif_fractions' histograms, which people build with `modkit motif bed` + `bedtools intersect` against the bedMethyl file.  The first
// record export whose records carry gathered values: the count / scan / fill scaffold of nmexport.h joined with the rank lookup of
// nmreadstats_device.h.
//   per work item = (candidate, chunk of its bin) the prologue of fractions_kernel: the PRESENCE planes of the candidate's read-statistics
//   slot in the state slots, the chunk loaded, the tile expanded, one walk per strand; a work item without an occurrence returns
//   (wave-uniform).  Per strand  site = acc & presence  (the modified base carries a kept record),  bare = acc & ~presence.
//   count  the records under `select` into the item table, the four classes (fwd site, fwd bare, rev site, rev bare) into the
//          (candidate, contig) table with 64-bit atomics from lane 0: a contig of several chunks takes several work items
//   fill   the rank of a lane's first record as in emit_records; the loop is written out here because a record needs, beside its rank,
//          the VALUE INDEX of its strand: first_record_index + the presence bits of the lane's earlier words + popc(pw[t] & (bit - 1)).
//          Both strands' indices advance side by side in the one walk over f | r.  A record outside the window writes nothing and
//          gathers nothing; a bare occurrence writes 0 / 0 and gathers nothing.
#include "nmexport.h"
#include "nmreadstats_device.h"

using namespace nmdetail;

namespace {

struct PileupArgs : ExportArgs {
    const uint32_t *cand_row0;               // first row of the candidate in the (candidate, contig) table
    const unsigned long long *cand_planes;   // [n_cand][2] presence planes P+ P- of the candidate's read-statistics slot
    const uint32_t *cand_slot;               // [n_cand] that slot: the index into rs
    const RsSlot *rs;                        // [NM_MAX_MOD_SLOTS]
    uint32_t select;                         // NM_PILEUP_SITE | NM_PILEUP_BARE
    uint32_t n_rows;                         // rows of the table
    unsigned long long *table;               // count pass: [n_rows][4], may be NULL
    uint32_t *out_valid, *out_mod;           // fill pass: the two gathered columns, beside out_contig / out_pos / out_code
};

__device__ __forceinline__ uint32_t pick(uint32_t select, uint32_t site, uint32_t bare) {
    return ((select & NM_PILEUP_SITE) ? site : 0u) | ((select & NM_PILEUP_BARE) ? bare : 0u);
}

template <int G, bool FILL>
__global__ __launch_bounds__(256) void pileup_kernel(PileupArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<FILL>(a, w)) return;
    const uint32_t k = w.owner;
    const unsigned long long *pl = a.cand_planes + (size_t)k * 2;
    const uint32_t *Pp = reinterpret_cast<const uint32_t *>(pl[0]), *Pm = reinterpret_cast<const uint32_t *>(pl[1]);
    const StatePlanes stp[1] = {StatePlanes{nullptr, nullptr, Pp, Pp, Pm, Pm}};
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
    const uint32_t (&pf)[T_WORDS] = raw.s[0][0], (&pr)[T_WORDS] = raw.s[0][2];   // the presence words of '+' and of '-'
    const uint32_t select = a.select;
    if (!FILL) {
        uint32_t c[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            c[0] += __popc(acc[0][t] & pf[t]); c[1] += __popc(acc[0][t] & ~pf[t]);
            c[2] += __popc(acc[1][t] & pr[t]); c[3] += __popc(acc[1][t] & ~pr[t]);
        }
        for (int o = 32; o; o >>= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] += __shfl_xor(c[j], o);
        }
        if (lane == 0) {
            a.item_cnt[w.item] = ((select & NM_PILEUP_SITE) ? c[0] + c[2] : 0u) + ((select & NM_PILEUP_BARE) ? c[1] + c[3] : 0u);
            const uint32_t row = ((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk];
            if (a.table && row < a.n_rows) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c[j]) atomicAdd(a.table + (size_t)row * 4 + j, (unsigned long long)c[j]);
            }
        }
        return;
    }
    // rank of the lane's first record = prefix of the item + records of the lanes before it (emit_records' first half)
    uint32_t mine = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) mine += __popc(pick(select, acc[0][t] & pf[t], acc[0][t] & ~pf[t])) + __popc(pick(select, acc[1][t] & pr[t], acc[1][t] & ~pr[t]));
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    unsigned long long at = w.off0 + (incl - mine) - a.first;           // relative to the window: one unsigned comparison covers both ends
    const uint32_t contig = ((cu32p)a.chunk_contig)[w.chunk];
    const uint32_t pos0 = (w.chunk - ((cu32p)a.contig_chunk)[contig]) * (uint32_t)CHUNK_BP + (uint32_t)lane * (T_WORDS * 32);
    const RsSlot rs = a.rs[((cu32p)a.cand_slot)[k]];
    // value index of the lane's first record per strand (lane shuffles: every lane calls, before the lanes part)
    uint64_t idx_f = first_record_index(pf, rs.base[0], rs.rank[0], contig, w.chunk, lane);
    uint64_t idx_r = first_record_index(pr, rs.base[1], rs.rank[1], contig, w.chunk, lane);
    auto put = [&](uint32_t pos, uint32_t minus, uint32_t pw, uint32_t bit, const uint2 *val, uint64_t idx) {
        if (at < a.capacity) {
            uint2 v = make_uint2(0u, 0u);
            if (pw & bit) v = val[idx + __popc(pw & (bit - 1u))];          // a site: its record's (n_valid_cov, n_modified)
            a.out_contig[at] = contig;
            a.out_pos[at] = pos;
            a.out_code[at] = (uint8_t)(minus | ((pw & bit) ? 0u : (uint32_t)NM_PILEUP_CODE_BARE));
            a.out_valid[at] = v.x;
            a.out_mod[at] = v.y;
        }
        ++at;
    };
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        const uint32_t f = pick(select, acc[0][t] & pf[t], acc[0][t] & ~pf[t]), r = pick(select, acc[1][t] & pr[t], acc[1][t] & ~pr[t]);
        uint32_t both = f | r;
        while (both) {                                                  // ascending position, '+' before '-'
            const uint32_t b = __builtin_ctz(both), bit = 1u << b;
            both &= both - 1;
            const uint32_t pos = pos0 + t * 32 + b;
            if (f & bit) put(pos, 0u, pf[t], bit, rs.val[0], idx_f);
            if (r & bit) put(pos, (uint32_t)NM_PILEUP_MINUS, pr[t], bit, rs.val[1], idx_r);
        }
        idx_f += __popc(pf[t]);
        idx_r += __popc(pr[t]);
    }
}

template <bool FILL>
constexpr ExportKernels<PileupArgs> pileup_kernels = {pileup_kernel<1, FILL>, pileup_kernel<2, FILL>, pileup_kernel<3, FILL>};
using PileupBatch = ExportBatch<PileupArgs>;

// validate the batch, compile its programs, stage the tables and enqueue the count pass (and, with_scan, the prefix + gather)
int pileup_begin(PileupBatch &pb, nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_rs_slot, const uint8_t *cand_len,
                 const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, const uint64_t *row_offset, uint32_t select,
                 bool with_scan) {
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (row_offset && row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
    std::vector<uint32_t> slots(n_cand, 0);
    std::vector<unsigned long long> planes((size_t)n_cand * 2, 0);
    std::vector<RsSlot> rs(NM_MAX_MOD_SLOTS, RsSlot{});
    Staged st;
    const int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, nullptr, row_offset, false, st,
                                    [&](uint32_t k, uint32_t, uint64_t &) {                    // the candidate's read-statistics slot
                                        slots[k] = cand_rs_slot[k];
                                        return stage_readstats_slot(c, k, slots[k], rs.data(), planes.data() + (size_t)k * 2);
                                    });
    if (rc) return rc;
    PileupArgs &a = pb.base;
    a.select = select;
    a.n_rows = (uint32_t)st.rows;
    std::vector<ExportTable> reserved;
    if (row_offset) reserved.push_back({&a.table, (size_t)st.rows * 32});
    return export_begin(pb, c, n_cand, cand_bin, st.width.data(), st.programs,
                        {{&a.cand_row0, st.row0.data(), st.row0.size() * 4},
                         {&a.cand_planes, planes.data(), planes.size() * 8},
                         {&a.cand_slot, slots.data(), slots.size() * 4},
                         {&a.rs, rs.data(), rs.size() * sizeof(RsSlot)}},
                        reserved, pileup_kernels<false>, with_scan);
}

int check_select(uint32_t select) {
    if (select == 0 || (select & ~(uint32_t)(NM_PILEUP_SITE | NM_PILEUP_BARE)))
        return fail(NM_EINVAL, "select %u: a non-empty combination of NM_PILEUP_SITE / NM_PILEUP_BARE", select);
    return NM_OK;
}

// export_window of nmexport.h with five columns: the owners' offsets to the host, the window clamped to the call's total, the fill
// pass, and the window's records to the host.
int pileup_window(PileupBatch &pb, uint32_t n_cand, uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos,
                  uint8_t *site_code, uint32_t *site_valid, uint32_t *site_mod, uint64_t *cand_offset, uint64_t *n_written) {
    nm_ctx *c = pb.c;
    HIP_TRY(hipMemcpyAsync(cand_offset, pb.d_owner_offset, (size_t)(n_cand + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = cand_offset[n_cand];
    const uint64_t n = first_record >= total ? 0 : std::min<uint64_t>(capacity, total - first_record);
    if (n == 0) return NM_OK;
    uint8_t *d_out = nullptr;                                             // contig | pos | valid | mod | code of the window's records
    const size_t col = align16((size_t)n * 4);
    HIP_TRY(dev_malloc(&d_out, 4 * col + (size_t)n));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)dev_free(p); } } guard{d_out, c};
    PileupArgs a = pb.base;
    a.first = first_record;
    a.capacity = n;
    a.out_contig = reinterpret_cast<uint32_t *>(d_out);
    a.out_pos = reinterpret_cast<uint32_t *>(d_out + col);
    a.out_valid = reinterpret_cast<uint32_t *>(d_out + 2 * col);
    a.out_mod = reinterpret_cast<uint32_t *>(d_out + 3 * col);
    a.out_code = d_out + 4 * col;
    const int rc = pb.launch(pileup_kernels<true>, a);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(site_contig, a.out_contig, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_pos, a.out_pos, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_valid, a.out_valid, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_mod, a.out_mod, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_code, a.out_code, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_written = n;
    return NM_OK;
}

}  // namespace

int nm_motif_pileup_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_rs_slot, const uint8_t *cand_len,
                          const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t select,
                          const uint64_t *row_offset, uint64_t *cand_total, int64_t *contig_counts) {
    if (!row_offset || (n_cand && (!cand_bin || !cand_rs_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !cand_total || !contig_counts)))
        return fail(NM_EINVAL, "NULL argument");
    if (const int rc = check_select(select)) return rc;
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) return NM_OK;
    PileupBatch pb;
    const int rc = pileup_begin(pb, c, n_cand, cand_bin, cand_rs_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks, row_offset, select, false);
    if (rc) return rc;
    const uint64_t rows = row_offset[n_cand];
    if (rows) HIP_TRY(hipMemcpyAsync(contig_counts, pb.base.table, (size_t)rows * 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_cand; ++k) {                               // the totals are sums of the table's selected classes
        uint64_t n = 0;
        for (uint64_t r = row_offset[k]; r < row_offset[k + 1]; ++r)
            for (int j = 0; j < 4; ++j)
                if (select >> (j & 1) & 1u) n += (uint64_t)contig_counts[r * 4 + j];
        cand_total[k] = n;
    }
    return NM_OK;
}

int nm_motif_pileup_sites(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_rs_slot, const uint8_t *cand_len,
                          const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t select,
                          uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                          uint32_t *site_valid, uint32_t *site_mod, uint64_t *cand_offset, uint64_t *n_written) {
    if (!cand_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code || !site_valid || !site_mod)) ||
        (n_cand && (!cand_bin || !cand_rs_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks)))
        return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (const int rc = check_select(select)) return rc;
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) {
        cand_offset[0] = 0;
        return NM_OK;
    }
    PileupBatch pb;
    const int rc = pileup_begin(pb, c, n_cand, cand_bin, cand_rs_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks, nullptr, select, true);
    if (rc) return rc;
    return pileup_window(pb, n_cand, first_record, capacity, site_contig, site_pos, site_code, site_valid, site_mod, cand_offset, n_written);
}
