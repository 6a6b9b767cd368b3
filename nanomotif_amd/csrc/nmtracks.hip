// Motif methylation ALONG contigs: for every candidate of a batch and every window of window_bp positions of every contig of its bin,
// the six site counts of nm_motif_sites_count (fwd mod, fwd nomod, fwd nocall, rev mod, rev nomod, rev nocall).  The five exports before
// this one reduce a motif to a row per contig or per bin; sites_kernel holds acc & state per 32-position word and sums the words of a
// contig away — this unit keeps them apart by position.  The count half of the scaffold of nmexport.h (no scan, no fill, no records),
// as nmprofile.hip uses it:
//   per work item = (candidate, chunk of its bin) the loads and the two walks of sites_kernel; a work item without an occurrence
//   returns (wave-uniform).  A lane covers T_WORDS * 32 = 128 positions = NM_TRACKS_MIN_WINDOW and window_bp is a multiple of that, so
//   a lane belongs to exactly one window and the lanes of a window are a contiguous run of the wave: lane l of chunk q of a contig is
//   lane number g = q * 64 + l of the contig, its window g / (window_bp / 128).
// Reduction: a wave holds at most 8192 occurrences per class, so two counts share a dword; the three dwords go through a segmented
// inclusive scan over the lanes (a run's first lane is known from the window number, no head flag travels), and the last lane of every
// run adds its non-zero counts to the window's row of the zeroed table with 32-bit atomics.  Atomics, not stores: a window takes
// contributions from several work items whenever window_bp does not divide 8192 or exceeds it.  At window_bp = 128 every lane is the
// last of its run and the rows are 24 bytes apart: the wave's atomics fall on one contiguous stretch.
// A lane past the contig's end (the last chunk's tail, the gap) holds no occurrence and adds nothing; the row index is checked against
// the table all the same.
#include "nmexport.h"

using namespace nmdetail;

namespace {

struct TracksArgs : ExportArgs {
    const uint32_t *cand_row0;               // first row of the candidate in the table
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    const uint32_t *contig_win0;             // [n_contigs] first window of the contig, relative to the first window of its bin
    uint32_t lanes_per_window;               // window_bp / 128
    uint32_t n_rows;                         // rows of the table
    uint32_t *table;                         // [n_rows][6]
};

template <int G>
__global__ __launch_bounds__(256) void tracks_kernel(TracksArgs a) {
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
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) any |= af[t] | ar[t];
    if (!__any((int)(any != 0))) return;                                 // wave-uniform: no occurrence in this chunk, nothing to add
    uint32_t c[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t f[3], r[3];
        split_states(raw.s[0], t, af[t], ar[t], f, r);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            c[i] += __popc(f[i]);
            c[3 + i] += __popc(r[i]);
        }
    }
    uint32_t p[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = c[j] | (c[j + 3] << 16);          // (a '+' count, the '-' count of the same state)
    const uint32_t contig = ((cu32p)a.chunk_contig)[w.chunk];
    const uint32_t lane0 = (w.chunk - ((cu32p)a.contig_chunk)[contig]) * 64u;   // the contig's lane number of this wave's lane 0
    const uint32_t lpw = a.lanes_per_window;
    const uint32_t win = (lane0 + (uint32_t)lane) / lpw;
    int tail = lane;                                                     // last lane of this lane's run
    if (lpw > 1) {                                                       // wave-uniform
        const uint32_t first = win * lpw;                                // the run in the contig's lane numbers: [first, first + lpw)
        const int head = first > lane0 ? (int)(first - lane0) : 0;
        const uint32_t last = first + (lpw - 1) - lane0;                 // (first + lpw - 1 >= lane0 + lane: no wrap)
        tail = last > 63u ? 63 : (int)last;
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t up = __shfl_up(p[j], o);
                if (lane - o >= head) p[j] += up;
            }
        }
    }
    if (lane == tail && (p[0] | p[1] | p[2])) {
        const uint32_t row = ((cu32p)a.cand_row0)[k] + ((cu32p)a.contig_win0)[contig] + win;
        if (row < a.n_rows) {
            uint32_t *out = a.table + (size_t)row * 6;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t f = p[j] & 0xFFFFu, r = p[j] >> 16;
                if (f) atomicAdd(out + j, f);
                if (r) atomicAdd(out + 3 + j, r);
            }
        }
    }
}

constexpr ExportKernels<TracksArgs> tracks_kernels = {tracks_kernel<1>, tracks_kernel<2>, tracks_kernel<3>};
using TracksBatch = ExportBatch<TracksArgs>;

int check_window(uint32_t window_bp) {
    if (window_bp < NM_TRACKS_MIN_WINDOW || window_bp > NM_TRACKS_MAX_WINDOW || window_bp % NM_TRACKS_MIN_WINDOW)
        return fail(NM_EINVAL, "window_bp %u: a multiple of %d in [%d, 2^30]", window_bp, NM_TRACKS_MIN_WINDOW, NM_TRACKS_MIN_WINDOW);
    return NM_OK;
}

uint64_t windows_of(uint64_t len, uint32_t window_bp) { return std::max<uint64_t>(1, (len + window_bp - 1) / window_bp); }

// the resident contigs of a bin in nm_bin_contigs order
std::vector<uint32_t> contigs_of(const nm_ctx *c, uint32_t bin) {
    std::vector<uint32_t> ids(c->bin_ncontigs[bin], 0);
    for (uint32_t i = 0; i < c->n_contigs; ++i)
        if (c->contig_bin[i] == bin && c->contig_rank[i] < ids.size()) ids[c->contig_rank[i]] = i;
    return ids;
}

}  // namespace

int nm_tracks_windows(nm_ctx *c, uint32_t bin, uint32_t window_bp, uint64_t *contig_win_offset, uint32_t capacity, uint32_t *n_contigs) {
    if (!n_contigs) return fail(NM_EINVAL, "NULL argument");
    const int rc = check_window(window_bp);
    if (rc) return rc;
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (bin >= c->n_bins) return fail(NM_EINVAL, "bin %u >= n_bins %u", bin, c->n_bins);
    const std::vector<uint32_t> ids = contigs_of(c, bin);
    *n_contigs = (uint32_t)ids.size();
    if (!contig_win_offset) return NM_OK;
    if (capacity < ids.size()) return fail(NM_ERANGE, "capacity %u below the %zu resident contigs of bin %u", capacity, ids.size(), bin);
    uint64_t at = 0;
    for (size_t r = 0; r < ids.size(); ++r) {
        contig_win_offset[r] = at;
        at += windows_of(c->contig_len[ids[r]], window_bp);
    }
    contig_win_offset[ids.size()] = at;
    return NM_OK;
}

int nm_motif_tracks_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                          const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t window_bp,
                          const uint64_t *row_offset, uint32_t *window_counts) {
    if (!row_offset || (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !window_counts)))
        return fail(NM_EINVAL, "NULL argument");
    int rc = check_window(window_bp);
    if (rc) return rc;
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
    if (n_cand == 0) return NM_OK;
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    // the layout of nm_tracks_windows for every bin the batch names
    std::vector<uint32_t> win0(c->n_contigs, 0);
    std::vector<uint64_t> bin_windows(c->n_bins, 0);
    std::vector<uint8_t> bin_done(c->n_bins, 0);
    Staged st;
    rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, cand_mod_slot, row_offset, false, st,
                          [&](uint32_t, uint32_t bin, uint64_t &need) {                        // a candidate takes a row per window of its bin
                              if (!bin_done[bin]) {
                                  uint64_t at = 0;
                                  for (uint32_t i : contigs_of(c, bin)) {
                                      if (at >= 0xFFFFFFFFull) return fail(NM_ERANGE, "more than 2^32 windows in bin %u", bin);
                                      win0[i] = (uint32_t)at;
                                      at += windows_of(c->contig_len[i], window_bp);
                                  }
                                  bin_windows[bin] = at;
                                  bin_done[bin] = 1;
                              }
                              need = bin_windows[bin];
                              return (int)NM_OK;
                          });
    if (rc) return rc;
    const uint64_t rows = st.rows;
    if (rows == 0) return NM_OK;                                          // every candidate in a bin without a contig
    TracksBatch tb;
    TracksArgs &a = tb.base;
    a.lanes_per_window = window_bp / NM_TRACKS_MIN_WINDOW;
    a.n_rows = (uint32_t)rows;
    rc = export_begin(tb, c, n_cand, cand_bin, st.width.data(), st.programs,
                      {{&a.cand_row0, st.row0.data(), st.row0.size() * 4},
                       {&a.cand_planes, st.planes.data(), st.planes.size() * 8},
                       {&a.contig_win0, win0.data(), win0.size() * 4}},
                      {{&a.table, (size_t)rows * 24}}, tracks_kernels, false);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(window_counts, a.table, (size_t)rows * 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}
