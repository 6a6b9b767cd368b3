// Sequence context of a motif's sites by methylation state: for every occurrence of every candidate of a batch, the contig's letter at
// every position within `radius` of its modified base, counted apart by the state (mod / nomod / nocall) of the occurrence itself.
// The other exports accept the motif as given; this unit answers whether it is under-specified: the cell (offset o, letter X) is the
// row nm_motif_sites_count would give the motif narrowed to X at o, for every o and X at once.
// An occurrence is nm_motif_sites' (nmsites.hip): own modified base at '+' coordinate p, occurrence strand s, state read in the
// candidate's own slot on strand s at p.  Offset o counts in the motif's reading direction: the probe is p + o for s = 0 and p - o for
// s = 1, its letter the contig's read on strand s (the complement for s = 1).  The count half of the scaffold of nmexport.h — no scan,
// no fill, no records:
//   per work item = (candidate, chunk of its bin) the sequence planes and the slot's state words are loaded once and the constraint
//   program is walked once per strand; the two match masks are split into three state words each.  A shift of sh positions along '+'
//   is one v_alignbit of two neighbouring words of each is-A / is-C / is-G / is-T plane of the tile (radius <= 31; the tile holds one
//   word of halo either side for every width), and serves offset sh of the '+' occurrences and offset -sh of the '-' ones, for which
//   is-A counts as T, is-C as G, is-G as C and is-T as A.
// Every contig is followed by GAP_BP invalid positions, which are in none of the four planes: a probe past a contig's end has no
// letter, without a special case.  So has an N.
// Reduction: 24 counters per shift.  A wave counts at most 8192 occurrences, so a '+' count and the '-' count of the same (state,
// plane) share a dword; the twelve dwords are folded over the wave — the first two steps hand half of the dwords to the partner lane,
// 21 cross-lane moves instead of 72 — and lanes 0, 16, 32, 48 end up with three dwords each.  Where all work items of a workgroup
// belong to one candidate (the common case: a bin has many chunks) those lanes add into a table in LDS that the workgroup adds to the
// candidate's rows once; otherwise, and with NM_CONTEXT_WAVE_ATOMICS=1 (read per call), every wave adds to the rows itself.
#include "nmexport.h"

using namespace nmdetail;

namespace {

constexpr int CTX_ROW = 24;                  // counters per offset: [2 occurrence strands][3 states][4 letters]
constexpr int CTX_MAX_CELLS = (2 * NM_CONTEXT_MAX_RADIUS + 1) * CTX_ROW;

struct ContextArgs : ExportArgs {
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    uint32_t radius, wave_atomics;
    unsigned long long *states;              // [n_cand][2][3]
    unsigned long long *table;               // [n_cand][2 radius + 1][2][3][4]
};

// The wave's sums of twelve dwords per lane: lane 16 g (g = 0..3) returns those of p[6 (g >> 1) + 3 (g & 1) + j] in out[j].  The
// steps over lane bits 5 and 4 keep one half of the dwords and send the other; the four remaining steps are a plain butterfly.
__device__ __forceinline__ void fold12(const uint32_t (&p)[12], int lane, uint32_t (&out)[3]) {
    const bool hi5 = (lane & 32) != 0, hi4 = (lane & 16) != 0;
    uint32_t q[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t keep = hi5 ? p[j + 6] : p[j], send = hi5 ? p[j] : p[j + 6];
        q[j] = keep + __shfl_xor(send, 32);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint32_t keep = hi4 ? q[j + 3] : q[j], send = hi4 ? q[j] : q[j + 3];
        out[j] = keep + __shfl_xor(send, 16);
    }
    for (int o = 8; o; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[j] += __shfl_xor(out[j], o);
    }
}

// One shift: the 24 counts, packed in pairs, folded over the wave and added at off_f (the row of offset +sh, '+' occurrences) and
// off_r (the row of offset -sh, '-' occurrences: + 12, letters complemented) of the candidate's table, in LDS or in memory.
template <bool UP>
__device__ __forceinline__ void context_shift(const uint32_t (&lt)[4][T_WORDS + 2], const uint32_t (&fs)[3][T_WORDS], const uint32_t (&rs)[3][T_WORDS],
                                              uint32_t bits, int lane, uint32_t off_f, uint32_t off_r, bool in_lds, uint32_t *lds,
                                              unsigned long long *rows) {
    uint32_t cf[12], cr[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) cf[j] = cr[j] = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) {
            const uint32_t letter = shifted<UP>(lt[pl], t, bits);
#pragma unroll
            for (int st = 0; st < 3; ++st) {
                cf[st * 4 + pl] += __popc(fs[st][t] & letter);
                cr[st * 4 + pl] += __popc(rs[st][t] & letter);
            }
        }
    }
    uint32_t p[12], mine[3];
#pragma unroll
    for (int j = 0; j < 12; ++j) p[j] = cf[j] | (cr[j] << 16);
    fold12(p, lane, mine);
    if ((lane & 15) == 0) {
        const uint32_t first = 6u * (uint32_t)(lane >> 5) + 3u * (uint32_t)((lane >> 4) & 1);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t cell = first + j, f = mine[j] & 0xFFFFu, r = mine[j] >> 16;    // cell = 4 state + plane
            const uint32_t at_f = off_f + cell, at_r = off_r + (cell & ~3u) + (3u - (cell & 3u));
            if (in_lds) {
                if (f) atomicAdd(lds + at_f, f);
                if (r) atomicAdd(lds + at_r, r);
            } else {
                if (f) atomicAdd(rows + at_f, (unsigned long long)f);
                if (r) atomicAdd(rows + at_r, (unsigned long long)r);
            }
        }
    }
}

template <int G>
__device__ __forceinline__ void context_item(const ContextArgs &a, const WorkItem &w, int lane, bool in_lds, uint32_t *lds) {
    using K = Variant<G, G, false, 1, false, false>;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.cand_planes + (size_t)k * 4)};
    RawChunk<K> raw;
    Tile<K> tile;
    uint32_t af[T_WORDS], ar[T_WORDS];
    find_occurrences<K>(a, w, stp, lane, raw, tile, af, ar);
    uint32_t fs[3][T_WORDS], rs[3][T_WORDS], c[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t f[3], r[3];
        split_states(raw.s[0], t, af[t], ar[t], f, r);
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            fs[st][t] = f[st];
            rs[st][t] = r[st];
            c[st] += __popc(fs[st][t]);
            c[3 + st] += __popc(rs[st][t]);
        }
    }
    uint32_t n[3];
#pragma unroll
    for (int st = 0; st < 3; ++st) n[st] = c[st] | (c[3 + st] << 16);
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int st = 0; st < 3; ++st) n[st] += __shfl_xor(n[st], o);
    }
    if ((n[0] | n[1] | n[2]) == 0) return;                               // wave-uniform: no occurrence in this chunk, nothing to add
    if (lane == 0) {
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            if (n[st] & 0xFFFFu) atomicAdd(a.states + (size_t)k * 6 + st, (unsigned long long)(n[st] & 0xFFFFu));
            if (n[st] >> 16) atomicAdd(a.states + (size_t)k * 6 + 3 + st, (unsigned long long)(n[st] >> 16));
        }
    }
    // the words of the four letter planes that lie one word either side of the lane's own
    uint32_t lt[4][T_WORDS + 2];
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) {
#pragma unroll
        for (int j = 0; j < T_WORDS + 2; ++j) lt[pl][j] = tile.w[pl][G - 1 + j];
    }
    const uint32_t R = a.radius;
    unsigned long long *rows = a.table + (size_t)k * (2 * R + 1) * CTX_ROW;
    for (uint32_t sh = 0; sh <= R; ++sh)
        context_shift<true>(lt, fs, rs, sh, lane, (R + sh) * CTX_ROW, (R - sh) * CTX_ROW + 12, in_lds, lds, rows);
    for (uint32_t sh = 1; sh <= R; ++sh)
        context_shift<false>(lt, fs, rs, 32 - sh, lane, (R - sh) * CTX_ROW, (R + sh) * CTX_ROW + 12, in_lds, lds, rows);
}

template <int G>
__global__ __launch_bounds__(256) void context_kernel(ContextArgs a) {
    __shared__ uint32_t lds[CTX_MAX_CELLS];
    const int lane = threadIdx.x & 63;
    const uint32_t cells = (2 * a.radius + 1) * CTX_ROW;
    // workgroup-uniform: do the (up to four) work items of this workgroup belong to one candidate?  The prefix is ascending, so the
    // first and the last decide.
    const uint32_t it0 = blockIdx.x * 4, it1 = min(it0 + 3, a.n_items - 1);
    const uint32_t slot0 = class_slot(a, it0);
    const bool in_lds = !a.wave_atomics && class_slot(a, it1) == slot0;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < cells; i += 256) lds[i] = 0;
        __syncthreads();
    }
    WorkItem w;
    if (locate_item<false>(a, w)) context_item<G>(a, w, lane, in_lds, lds);
    if (in_lds) {
        __syncthreads();
        unsigned long long *rows = a.table + (size_t)((cu32p)a.cls_owner)[slot0] * cells;
        for (uint32_t i = threadIdx.x; i < cells; i += 256) {
            const uint32_t v = lds[i];
            if (v) atomicAdd(rows + i, (unsigned long long)v);
        }
    }
}

constexpr ExportKernels<ContextArgs> context_kernels = {context_kernel<1>, context_kernel<2>, context_kernel<3>};
using ContextBatch = ExportBatch<ContextArgs>;

}  // namespace

int nm_motif_context_count(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                           const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t radius,
                           uint64_t *cand_states, int64_t *counts) {
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !cand_states || !counts))
        return fail(NM_EINVAL, "NULL argument");
    if (radius > NM_CONTEXT_MAX_RADIUS) return fail(NM_EINVAL, "radius %u above NM_CONTEXT_MAX_RADIUS = %d", radius, NM_CONTEXT_MAX_RADIUS);
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand == 0) return NM_OK;
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    Staged st;
    int rc = stage_candidates(c, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, cand_mod_slot, nullptr, false, st, no_check);
    if (rc) return rc;
    const char *env = getenv("NM_CONTEXT_WAVE_ATOMICS");
    const size_t row = (size_t)(2 * radius + 1) * CTX_ROW;
    ContextBatch cb;
    ContextArgs &a = cb.base;
    a.radius = radius;
    a.wave_atomics = env && env[0] && env[0] != '0';
    rc = export_begin(cb, c, n_cand, cand_bin, st.width.data(), st.programs, {{&a.cand_planes, st.planes.data(), st.planes.size() * 8}},
                      {{&a.states, (size_t)n_cand * 48}, {&a.table, (size_t)n_cand * row * 8}}, context_kernels, false);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(cand_states, a.states, (size_t)n_cand * 48, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(counts, a.table, (size_t)n_cand * row * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}
