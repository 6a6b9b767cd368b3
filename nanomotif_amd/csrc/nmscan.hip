// libnmscan — MI355X (gfx950 / CDNA4) motif scan + methylation count engine.  C ABI: include/nmscan.h.
//
// Design (DESIGN.md has the long form):
//   * Assembly resident in HBM as three bit planes over one padded coordinate space: H, L (the two bits of
//     the base code, "bit-sliced 2-bit") and V (1 = A/C/G/T inside a contig).  Contigs are grouped by bin and
//     start on 8192-bp chunk boundaries with >= 96 invalid positions (GAP_BP) after each one, so a match can never
//     straddle two contigs and a chunk never straddles two bins.
//   * Per modification type two state planes M / U (methylated, unmethylated; the strand of a row is implied by
//     the base under it: '+' rows sit on the canonical base, '-' rows on its complement) — 0.5 byte per bp per
//     scoring step in total with H and L.  Four per-strand planes (MP, UP, MM, UM) back the general case
//     (motifs whose modified position is not the canonical literal).
//   * Scoring kernel: one wavefront owns one chunk (64 lanes x 4 consecutive 32-bit words = 8192 bp) held in
//     VGPRs as eight derived planes (is-A/C/G/T and valid-not-A/C/G/T) with one halo word each side.  A
//     candidate motif is a set of wave-uniform constraints "plane p must be set at offset d from the modified
//     base"; each costs one v_alignbit + one v_and per word, driven from SGPR bit masks (s_ff1 loop), no LDS
//     traffic and no divergent control flow.  Forward and reverse-complement sites are disjoint (canonical vs
//     complement base), so they are OR-ed and counted with two popcounts against M and U.
//   * Per-lane counts go to LDS with ds_add, are reduced once per workgroup segment and leave the CU as one
//     64-bit atomic per counter.
#define NM_SCORE_KERNEL_SOURCE
#include "nmscan_device.h"

using namespace nmdetail;

namespace {

thread_local std::string g_err;

// ------------------------------------------------------------------------------------------------------
// device code
// ------------------------------------------------------------------------------------------------------
// Pack: one workgroup per chunk, 64 positions per wave per step, wave ballot builds the plane words.
__global__ __launch_bounds__(256) void pack_kernel(const uint8_t *__restrict__ ascii,
                                                   const uint64_t *__restrict__ contig_src,
                                                   const uint64_t *__restrict__ contig_len,
                                                   const uint32_t *__restrict__ chunk_contig,
                                                   const uint32_t *__restrict__ chunk_first,
                                                   uint32_t *__restrict__ H, uint32_t *__restrict__ L,
                                                   uint32_t *__restrict__ V, unsigned long long *__restrict__ other) {
    const uint32_t chunk = blockIdx.x;
    const uint32_t contig = chunk_contig[chunk];
    if (contig == 0xFFFFFFFFu) return;                               // pad chunk, planes already zero
    const uint64_t beg = contig_src[contig], len = contig_len[contig];     // (src: where the contig's bytes start in `ascii`)
    const uint64_t local0 = (uint64_t)(chunk - chunk_first[contig]) * CHUNK_BP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int it = wave; it < CHUNK_BP / 64; it += 4) {
        const uint64_t p = local0 + (uint64_t)it * 64 + lane;
        uint8_t c = 0;
        if (p < len) c = ascii[beg + p] & 0xDF;                      // upper-case (seq.py:55)
        const bool valid = (c == 'A') | (c == 'C') | (c == 'G') | (c == 'T');
        const unsigned long long bv = __ballot(valid);
        const unsigned long long bh = __ballot(valid && (c & 4));    // A=00 C=01 G=11 T=10 as (H,L) = bits 2,1
        const unsigned long long bl = __ballot(valid && (c & 2));
        const unsigned long long bo = __ballot(p < len && !valid && c != 'N');   // IUPAC ambiguity codes etc.
        if (bo && lane == 0) atomicAdd(other, (unsigned long long)__popcll(bo));
        if (lane < 2) {
            const size_t w = (size_t)chunk * CHUNK_WORDS + (size_t)it * 2 + lane;
            H[w] = (uint32_t)(bh >> (32 * lane));
            L[w] = (uint32_t)(bl >> (32 * lane));
            V[w] = (uint32_t)(bv >> (32 * lane));
        }
    }
}

// needs_v[c] = 0 iff chunk c is entirely valid and so are the three words either side of it (the widest halo a variant reads).
__global__ void needs_v_kernel(const uint32_t *__restrict__ V, uint8_t *__restrict__ needs_v, uint32_t n_chunks) {
    const uint32_t c = blockIdx.x;
    __shared__ uint32_t all_and;
    if (threadIdx.x == 0) all_and = 0xFFFFFFFFu;
    __syncthreads();
    uint32_t v = V[(size_t)c * CHUNK_WORDS + threadIdx.x];
    if (threadIdx.x < 3) {
        if (c > 0) v &= V[(size_t)c * CHUNK_WORDS - 1 - threadIdx.x];
        else v = 0;
        if (c + 1 < n_chunks) v &= V[(size_t)(c + 1) * CHUNK_WORDS + threadIdx.x];
        else v = 0;
    }
    if (v != 0xFFFFFFFFu) atomicAnd(&all_and, v);
    __syncthreads();
    if (threadIdx.x == 0) needs_v[c] = all_and != 0xFFFFFFFFu;
}

// State build: one thread per pileup row; classification is the reference's float64 compare.
__global__ void state_kernel(uint64_t n_rows, const uint32_t *__restrict__ contig_id,
                             const uint32_t *__restrict__ position, const uint8_t *__restrict__ strand,
                             const double *__restrict__ frac, double low, double high,
                             const uint32_t *__restrict__ contig_chunk, const uint64_t *__restrict__ contig_len,
                             uint32_t n_contigs, uint32_t can_h, uint32_t can_l,
                             const uint32_t *__restrict__ H, const uint32_t *__restrict__ L,
                             const uint32_t *__restrict__ V, uint32_t *M, uint32_t *U, uint32_t *MP, uint32_t *UP,
                             uint32_t *MM, uint32_t *UM, unsigned int *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t cid = contig_id[i];
    const uint32_t pos = position[i];
    if (cid >= n_contigs || pos >= contig_len[cid]) { atomicOr(err, 1u); return; }
    const double f = frac[i];
    const bool meth = f >= high, non = f <= low;
    if (!meth && !non) return;
    const uint64_t g = (uint64_t)contig_chunk[cid] * CHUNK_BP + pos;
    const size_t w = g >> 5;
    const uint32_t bit = 1u << (g & 31);
    const bool plus = strand[i] == '+';
    if (!plus && strand[i] != '-') { atomicOr(err, 2u); return; }
    uint32_t *gen = plus ? (meth ? MP : UP) : (meth ? MM : UM);
    const uint32_t old = atomicOr(gen + w, bit);
    if (old & bit) atomicOr(err, 4u);                                // duplicate (contig, position, strand)
    // compact planes: keep the row only when the base under it is the one its strand implies
    const uint32_t h = (H[w] & bit) != 0, l = (L[w] & bit) != 0, v = (V[w] & bit) != 0;
    // complement in the (H,L) code: A(00)<->T(10), C(01)<->G(11) — H flips, L stays
    const uint32_t want_h = plus ? can_h : (can_h ^ 1u);
    if (v && h == want_h && l == can_l) atomicOr((meth ? M : U) + w, bit);
}

__global__ void compile_kernel(uint32_t n_prog, const CandRec *__restrict__ rec, const uint8_t *__restrict__ masks,
                               uint32_t *__restrict__ programs, int wide, int np, int fold_modpos, int classes, uint32_t c_slots) {
    // classes: write the class layout of the CLS variants (nmscan_device.h; wide, np and fold_modpos do not apply), 1 with the
    // fused head of a walk, 2 with every literal left in its word (NM_SCORE_HEAD=0), plus 4 x the tail descriptors to write
    // (CLS_TAIL_LITERALS | CLS_TAIL_CLASS, NM_SCORE_TAIL);
    // c_slots: bit s = mod slot s has canonical base C (the compiler swaps the base sets of such a candidate)
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_prog) return;
    if (classes) compile_one_classes(k, rec, masks, programs, c_slots, (classes & 3) == 1, classes >> 2);
    else compile_one(k, rec, masks, programs, wide, np, fold_modpos);
}

__global__ void common_kernel(uint32_t n_entries, uint4 *__restrict__ range, uint32_t *__restrict__ programs, uint32_t pdw,
                              uint32_t n_prog, uint32_t max_group) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n_entries) common_one(g, range, programs, programs + (size_t)n_prog * pdw, pdw, n_prog, max_group);
}

// Both steps in ONE launch for the small light batches of the search's long tail (a few dozen candidates, where a round
// is a chain of launch latencies): a single workgroup compiles, synchronises, and factors the groups.
__global__ __launch_bounds__(1024) void compile_common_kernel(uint32_t n_prog, const CandRec *__restrict__ rec,
                                                               const uint8_t *__restrict__ masks, uint32_t *__restrict__ programs, int wide,
                                                               int np, int fold_modpos, uint32_t n_entries, uint4 *__restrict__ range,
                                                               uint32_t pdw, uint32_t max_group, uint32_t lds_words) {
    // the candidates' programs are built and factored in LDS (a program is a chain of read-modify-writes: one dependent
    // round trip each in global memory) and leave in one coalesced copy; a batch too large for that works in place
    extern __shared__ uint32_t lds_programs[];
    uint32_t *work = lds_words ? lds_programs : programs;
    for (uint32_t k = threadIdx.x; k < n_prog; k += blockDim.x) compile_one(k, rec, masks, work, wide, np, fold_modpos);
    __threadfence_block();
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < n_entries; g += blockDim.x) common_one(g, range, work, programs + (size_t)n_prog * pdw, pdw, n_prog, max_group);
    if (lds_words) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_prog * pdw; i += blockDim.x) programs[i] = lds_programs[i];
    }
}

// ---- candidates that reach further than 95 positions from the modified base (a search frame above 191: the reference takes any
// --search_frame_size, find_motifs_bin.py:110-130): a plain, slow kernel — speed is irrelevant there.  One workgroup per (chunk of the
// candidate's bin, candidate), one thread per 32-position word; per specified motif position the plane words are FETCHED at the
// shifted address (no register tile), a site survives only while every constrained position lies inside its own contig
// (utils.py:44-67: a regex match cannot leave the string; beyond 96 positions the padding between contigs no longer guarantees it).
struct WideArgs {
    Planes seq;
    StatePlanes st[NM_MAX_MOD_SLOTS];
    const uint32_t *cand_bin, *cand_mask_off;
    const uint16_t *cand_len, *cand_modpos;
    const uint8_t *cand_slot, *masks;
    const uint32_t *bin_chunk0, *bin_nchunks, *chunk_contig, *contig_chunk;
    const uint64_t *contig_len;
    unsigned long long *out;
    long long n_words;
};

__device__ __forceinline__ uint32_t plane_bits_at(const uint32_t *__restrict__ pl, long long n_words, long long g) {      // the 32 bits of a plane from position g on
    const long long i = g >> 5;                                           // (arithmetic shift: floor)
    const uint32_t sh = (uint32_t)(g & 31);
    const uint32_t lo = i >= 0 && i < n_words ? pl[i] : 0u;
    const uint32_t hi = sh && i + 1 >= 0 && i + 1 < n_words ? pl[i + 1] : 0u;
    return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
}

__global__ __launch_bounds__(256) void score_wide_kernel(WideArgs a) {
    __shared__ unsigned int part[2][4];
    const uint32_t k = blockIdx.y, bin = a.cand_bin[k];
    if (blockIdx.x >= a.bin_nchunks[bin]) return;
    const uint32_t chunk = a.bin_chunk0[bin] + blockIdx.x, contig = a.chunk_contig[chunk];
    if (contig == 0xFFFFFFFFu) return;
    const uint32_t len = a.cand_len[k], mp = a.cand_modpos[k], slot = a.cand_slot[k];
    const uint8_t *m = a.masks + a.cand_mask_off[k];
    const size_t w = (size_t)chunk * CHUNK_WORDS + threadIdx.x;
    const long long g0 = (long long)w * 32;                               // global position of the word's bit 0
    const long long p0 = (long long)(chunk - a.contig_chunk[contig]) * CHUNK_BP + 32ll * threadIdx.x;      // ... inside its contig
    const long long clen = (long long)a.contig_len[contig];
    auto inside = [&](long long d) -> uint32_t {                          // bits b of the word with 0 <= p0 + b + d < clen
        const long long lo = -(p0 + d), hi = clen - (p0 + d);
        const long long l = lo < 0 ? 0 : lo, h = hi > 32 ? 32 : hi;
        if (h <= l) return 0u;
        const uint32_t upto_h = h >= 32 ? 0xFFFFFFFFu : ((1u << h) - 1u);
        return upto_h & ~(l ? ((1u << l) - 1u) : 0u);
    };
    uint32_t acc[2];
    for (int strand = 0; strand < 2; ++strand) {
        uint32_t s = inside(0);
        for (uint32_t j = 0; j < len && s; ++j) {
            const uint32_t set_f = m[j] & 15u;
            if (set_f == 15u) continue;
            const long long d = strand == 0 ? (long long)j - mp : (long long)mp - j;
            const uint32_t set = strand == 0 ? set_f : (((set_f & 1) << 3) | ((set_f & 2) << 1) | ((set_f & 4) >> 1) | ((set_f & 8) >> 3));
            const uint32_t ok = inside(d);
            if (!ok) { s = 0; break; }
            const uint32_t h = plane_bits_at(a.seq.H, a.n_words, g0 + d), l = plane_bits_at(a.seq.L, a.n_words, g0 + d), v = plane_bits_at(a.seq.V, a.n_words, g0 + d);
            uint32_t match = 0;                                           // A = 00, C = 01, G = 11, T = 10 as (H, L)
            if (set & NM_BASE_A) match |= ~h & ~l;
            if (set & NM_BASE_C) match |= ~h & l;
            if (set & NM_BASE_G) match |= h & l;
            if (set & NM_BASE_T) match |= h & ~l;
            s &= match & v & ok;
        }
        acc[strand] = s;
    }
    const StatePlanes &st = a.st[slot];
    unsigned int n_mod = __popc(acc[0] & st.MP[w]) + __popc(acc[1] & st.MM[w]);
    unsigned int n_non = __popc(acc[0] & st.UP[w]) + __popc(acc[1] & st.UM[w]);
    for (int o = 32; o; o >>= 1) { n_mod += __shfl_xor(n_mod, o); n_non += __shfl_xor(n_non, o); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = n_mod; part[1][threadIdx.x >> 6] = n_non; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int x = part[0][0] + part[0][1] + part[0][2] + part[0][3], y = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if (x) atomicAdd(a.out + 2 * (size_t)k, (unsigned long long)x);
        if (y) atomicAdd(a.out + 2 * (size_t)k + 1, (unsigned long long)y);
    }
}

// Site masks of one candidate over the chunks of one contig (general planes) for nm_hit_positions.
template <int GN, int GP>
__global__ __launch_bounds__(256) void hits_kernel(Planes seq, StatePlanes st, uint32_t chunk0, uint32_t n_chunks,
                                                   const uint32_t *__restrict__ prog, int which,
                                                   uint32_t *__restrict__ out) {
    using K = Variant<GN, GP, false, 1, false, false>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ck = blockIdx.x * 4 + wave;
    if (ck >= n_chunks) return;
    const uint32_t chunk = chunk0 + ck;
    const StatePlanes stp[1] = {st};
    RawChunk<K> raw;
    raw.load(seq, stp, chunk, lane);
    Tile<K> tile;
    tile.expand(raw);
    uint32_t acc[T_WORDS];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) acc[t] = 0xFFFFFFFFu;
    eval_strand<K>((cu32p)(prog + (which >= 2 ? K::PDW : 0)), tile, acc);
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        // (a select chain, not raw.s[0][which][t]: a register array indexed at run time lives in private memory)
        const uint32_t state = which == 0 ? raw.s[0][0][t] : which == 1 ? raw.s[0][1][t] : which == 2 ? raw.s[0][2][t] : raw.s[0][3][t];
        out[(size_t)ck * CHUNK_WORDS + lane * T_WORDS + t] = acc[t] & state;
    }
}

// nm_hit_positions, device-side compaction of the site masks hits_kernel wrote: only the hit INDICES cross PCIe.
// (1) set bits per chunk (256 words = one workgroup)
__global__ __launch_bounds__(256) void hits_count_kernel(const uint32_t *__restrict__ masks, uint32_t *__restrict__ chunk_cnt) {
    __shared__ uint32_t part[4];
    uint32_t n = __popc(masks[(size_t)blockIdx.x * CHUNK_WORDS + threadIdx.x]);
    for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// (2) exclusive prefix over the chunks (one workgroup walks them 256 at a time), total in off[n_chunks]
__global__ __launch_bounds__(256) void hits_scan_kernel(const uint32_t *__restrict__ chunk_cnt, uint32_t n_chunks, unsigned long long *__restrict__ off) {
    __shared__ unsigned long long buf[256];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_chunks; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long v = i < n_chunks ? chunk_cnt[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {                   // Hillis-Steele inclusive scan
            const unsigned long long add = threadIdx.x >= (unsigned)d ? buf[threadIdx.x - d] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n_chunks) off[i] = carry + buf[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += buf[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n_chunks] = carry;
}

// (3) every word writes the contig-local positions of its bits at its rank (ascending: words, then bits)
__global__ __launch_bounds__(256) void hits_scatter_kernel(const uint32_t *__restrict__ masks, const unsigned long long *__restrict__ off,
                                                           long long *__restrict__ out, unsigned long long capacity) {
    __shared__ uint32_t buf[256];
    uint32_t m = masks[(size_t)blockIdx.x * CHUNK_WORDS + threadIdx.x];
    const uint32_t n = __popc(m);
    buf[threadIdx.x] = n;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t add = threadIdx.x >= (unsigned)d ? buf[threadIdx.x - d] : 0;
        __syncthreads();
        buf[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long at = off[blockIdx.x] + buf[threadIdx.x] - n;
    const long long w0 = ((long long)blockIdx.x * CHUNK_WORDS + threadIdx.x) * 32;
    while (m && at < capacity) {
        out[at++] = w0 + (__ffs(m) - 1);
        m &= m - 1;
    }
}

}  // namespace


// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
namespace nmdetail {

static nm_alloc_fn g_alloc = nullptr;
static nm_free_fn g_free = nullptr;
static void *g_alloc_user = nullptr;
static int g_live_ctx = 0;          // contexts alive: the allocator pair may only change while there is none

hipError_t device_alloc(void **p, size_t bytes) {
    *p = nullptr;
    if (bytes == 0) return hipSuccess;
    if (g_alloc) return g_alloc(g_alloc_user, p, bytes) == 0 && *p ? hipSuccess : hipErrorOutOfMemory;
    return hipMalloc(p, bytes);
}

hipError_t device_free(void *p) {
    if (!p) return hipSuccess;
    if (g_free) return g_free(g_alloc_user, p) == 0 ? hipSuccess : hipErrorInvalidValue;
    return hipFree(p);
}

__global__ __launch_bounds__(256) void stage_in_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n_copy, uint4 *__restrict__ zero,
                                                       uint32_t n_zero) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (uint32_t k = i; k < n_copy; k += stride) dst[k] = src[k];
    for (uint32_t k = i; k < n_zero; k += stride) zero[k] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(256) void stage_out_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (uint32_t k = i; k < n; k += stride) dst[k] = src[k];
}

int stage_in(hipStream_t st, const void *h_src, void *d_dst, size_t bytes, void *d_zero, size_t zero_bytes) {
    const uint32_t n_copy = (uint32_t)((bytes + 15) / 16), n_zero = (uint32_t)((zero_bytes + 15) / 16);
    const uint32_t blocks = std::max(1u, std::min(256u, (std::max(n_copy, n_zero) + 255) / 256));
    hipLaunchKernelGGL(stage_in_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const uint4 *>(h_src), static_cast<uint4 *>(d_dst), n_copy,
                       static_cast<uint4 *>(d_zero), n_zero);
    HIP_TRY(hipGetLastError());
    return NM_OK;
}

int stage_out(hipStream_t st, const void *d_src, void *h_dst, size_t bytes) {
    const uint32_t n = (uint32_t)((bytes + 15) / 16);
    hipLaunchKernelGGL(stage_out_kernel, dim3(std::max(1u, std::min(256u, (n + 255) / 256))), dim3(256), 0, st, static_cast<const uint4 *>(d_src),
                       static_cast<uint4 *>(h_dst), n);
    HIP_TRY(hipGetLastError());
    return NM_OK;
}

int ensure_stage(nm_ctx *c, size_t bytes, int mode) {
    // A pair whose pinned half still holds the results of an open begin / end batch (nm_score_batch_begin,
    // nm_win_batch_w_begin) is never handed out: the next user would copy over — or, growing the pair, free — what
    // nm_*_end has yet to read.  At most two pairs are held at a time, so the walk always finds a free one.
    auto held = [&](int i) {
        for (int f = 0; f < NM_FLIGHTS; ++f)
            if ((c->score_wait[f].open && c->score_wait[f].stage == &c->stage[i]) || (c->win_wait[f].open && c->win_wait[f].stage == &c->stage[i]) ||
                (c->spec_wait[f].open && c->spec_wait[f].stage == &c->stage[i]))
                return true;
        return false;
    };
    int idx;
    std::unique_lock<std::mutex> lk(c->wait_mu);
    if (mode >= 2) idx = NM_STAGE_RING + (mode - 2);
    else if (mode == 1) {
        idx = c->stage_next_deep;
        for (int tries = 0; tries < NM_STAGE_RING && held(idx); ++tries) idx = (idx + 1) % NM_STAGE_RING;
        c->stage_next_deep = (idx + 1) % NM_STAGE_RING;
    } else {
        idx = c->stage_next;
        if (held(idx)) idx ^= 1;
        c->stage_next = idx ^ 1;
        for (int tries = 0; tries < NM_STAGE_RING && held(idx); ++tries) idx = (idx + 1) % NM_STAGE_RING;     // (two flights may hold both)
    }
    if (held(idx)) return fail(NM_ESTATE, "staging ring: every pair is held by an uncollected batch");
    lk.unlock();
    nm_ctx::Stage &st = c->stage[idx];
    if (!st.busy) HIP_TRY(hipEventCreateWithFlags(&st.busy, hipEventDisableTiming));
    if (st.pending) {
        HIP_TRY(hipEventSynchronize(st.marker));
        st.pending = false;
    }
    bytes += 32;                                           // stage_in / stage_out move whole 16-byte words
    if (bytes > st.bytes) {
        const size_t nb = std::max(bytes, st.bytes * 2);
        if (st.d) (void)nmdetail::dev_free(st.d);
        if (st.h) (void)hipHostFree(st.h);
        st.d = st.h = nullptr;
        st.bytes = 0;
        HIP_TRY(nmdetail::dev_malloc(&st.d, nb));
        HIP_TRY(hipHostMalloc(&st.h, nb, hipHostMallocDefault));
        st.bytes = nb;
    }
    c->d_stage = st.d;
    c->h_stage = st.h;
    c->cur_stage = &st;
    return NM_OK;
}

int release_stage(nm_ctx *c, hipStream_t s) {   // call after the last device work that reads the acquired pair was enqueued
    HIP_TRY(hipEventRecord(c->cur_stage->busy, s ? s : c->stream));
    c->cur_stage->marker = c->cur_stage->busy;
    c->cur_stage->pending = true;
    return NM_OK;
}

// The same for a pair whose last reader is a dispatch that carries `stop` as its stop event: the pair remembers that event and no
// packet is queued.  Only for an event nothing records again while the pair may be pending: a pool event of nm_timing_reset(1),
// which stays its launch's own until the next nm_timing_reset — and that drains every such pair (see there).
void release_stage_bound(nm_ctx *c, hipEvent_t stop) {
    c->cur_stage->marker = stop;
    c->cur_stage->pending = true;
}

constexpr size_t EV_POOL_MAX = 65536;

static hipError_t ev_pool_grow(nm_ctx *c) {             // one more event pair for the timing pool (the callers keep it below EV_POOL_MAX)
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e == hipSuccess) c->ev_pool.emplace_back(a, b);
    return e;
}

void busy_begin(nm_ctx *c) {
    if (!c->ev_collect_all) return;
    if (c->ev_used == c->ev_pool.size() && (c->ev_pool.size() >= EV_POOL_MAX || ev_pool_grow(c) != hipSuccess)) return;
    (void)hipEventRecord(c->ev_pool[c->ev_used].first, c->stream);
    c->busy_open = true;
}

void busy_end(nm_ctx *c) {
    if (!c->ev_collect_all || !c->busy_open) return;
    (void)hipEventRecord(c->ev_pool[c->ev_used].second, c->stream);
    c->ev_used += 1;
    c->busy_open = false;
}

int join_lanes(nm_ctx *c) {
    if (c->lane_stream && c->lane_pending) {
        HIP_TRY(hipStreamSynchronize(c->lane_stream));
        c->lane_pending = false;
    }
    return NM_OK;
}

}  // namespace nmdetail

namespace {


// Launch shape of a batch: which kernel variant its plan (nmscore_plan.h: plan_shape) asks for.
struct LaunchShape {
    int wide;                 // 0: offsets in [-32, 31], 1: [-64, 63], 2: [-96, 95]
    bool compact, lit, light; // light: the streaming (CF) variants
    bool fuse;                // two slots in one workgroup column
    bool per_contig;
    bool classes;             // narrow compact non-literal heavy batch: the class-plane variants and their program layout
    bool park;                // ... the one that parks the state words in LDS (never per-contig)
};

template <class K>
void launch_variant(const ScoreArgs &a, uint32_t gx, uint32_t gy, hipStream_t s, hipEvent_t stop) {
    // stop: an event bound to the dispatch (complete when the kernel is, its time the kernel's end) instead of one recorded behind it
    if (stop) hipExtLaunchKernelGGL((score_kernel<K>), dim3(gx, gy), dim3(256), 0, s, nullptr, stop, 0, a);
    else hipLaunchKernelGGL((score_kernel<K>), dim3(gx, gy), dim3(256), 0, s, a);
}

template <int G, bool COMPACT, bool LIT>
void launch_by_load(const ScoreArgs &a, uint32_t gx, uint32_t gy, const LaunchShape &sh, hipStream_t s, hipEvent_t stop = nullptr) {
    if (!sh.light) launch_variant<Variant<G, G, COMPACT, 1, LIT, false>>(a, gx, gy, s, stop);
    else if (sh.fuse && LIT) launch_variant<Variant<G, G, COMPACT, 2, LIT, true>>(a, gx, gy, s, stop);   // (fusing two slots on the 8-plane tile needs 128 VGPRs)
    else launch_variant<Variant<G, G, COMPACT, 1, LIT, true>>(a, gx, gy, s, stop);
}

void launch_score(const ScoreArgs &a, uint32_t gx, uint32_t gy, const LaunchShape &sh, hipStream_t s, hipEvent_t stop = nullptr) {
    if (sh.per_contig) {      // (candidate, contig) counters: the plain one-slot-per-column kernels with the other reduction key
        if (sh.wide == 2 && sh.compact) launch_variant<Variant<3, 3, true, 1, false, false, true>>(a, gx, gy, s, stop);
        else if (sh.wide == 2) launch_variant<Variant<3, 3, false, 1, false, false, true>>(a, gx, gy, s, stop);
        else if (!sh.wide && sh.compact && sh.classes) launch_score_classes(a, gx, gy, true, false, s, stop);
        else if (!sh.wide && sh.compact) launch_variant<Variant<1, 1, true, 1, false, false, true>>(a, gx, gy, s, stop);
        else if (!sh.wide) launch_variant<Variant<1, 1, false, 1, false, false, true>>(a, gx, gy, s, stop);
        else if (sh.compact) launch_variant<Variant<2, 2, true, 1, false, false, true>>(a, gx, gy, s, stop);
        else launch_variant<Variant<2, 2, false, 1, false, false, true>>(a, gx, gy, s, stop);
        return;
    }
    if (sh.wide == 2) {       // motifs that reach more than 63 positions from the modified base (search frames above 127)
        if (sh.compact) launch_by_load<3, true, false>(a, gx, gy, sh, s, stop);
        else launch_by_load<3, false, false>(a, gx, gy, sh, s, stop);
    } else if (!sh.wide && sh.compact) {
        if (sh.classes) launch_score_classes(a, gx, gy, false, sh.park, s, stop);
        else if (sh.lit) launch_by_load<1, true, true>(a, gx, gy, sh, s, stop);
        else launch_by_load<1, true, false>(a, gx, gy, sh, s, stop);
    } else if (!sh.wide) launch_by_load<1, false, false>(a, gx, gy, sh, s, stop);
    else if (sh.compact) launch_by_load<2, true, false>(a, gx, gy, sh, s, stop);
    else launch_by_load<2, false, false>(a, gx, gy, sh, s, stop);
}

// What the enqueueing steps of one scoring call share: its plan, where it runs and what it writes.
struct ScoreRun {
    const ScoreRequest &rq;
    const ScorePlan &p;
    hipStream_t sst, pst;               // the scoring stream, and the one the tables travel and are compiled on
    bool laned;
    uint8_t *hs, *ds;                   // the staging pair
    uint32_t *d_prog;
    unsigned long long *out;
    hipEvent_t e0, e1;
    bool timed_launch;
    uint32_t enq;                       // NM_ENQ_*: the parts of the short enqueue this call takes (score_enqueue_form)
};

// The clear of a caller's count table as a dispatch of the library's own: the stream, the position and the bytes of the
// hipMemsetAsync it stands for (the clear stays ordered on the scoring stream against whatever the caller queued on
// the table), and a dispatch carries the timing pair's first event as its stop event.
__global__ __launch_bounds__(256) void clear_counts_kernel(unsigned long long *__restrict__ out, uint64_t n_words) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_words; k += stride) out[k] = 0ull;
}

// Which enqueue a call takes (include/nmscan.h: NM_ENQ_*).  The short one is for a batch whose counts stay on the device and that
// nobody waits for — d_out given, no host counts, not deferred, no spec source: it prepares on the copy stream and is always timed.
// allowed: NM_SCORE_ENQUEUE, read at every call (same-process A/B, tests/test_gpu_score_enqueue.py), unset = all; 0 = the enqueue as
// it was: hipMemsetAsync and three recorded events.
uint32_t score_enqueue_form(const ScoreRequest &rq, const ScorePlan &p, uint32_t allowed) {
    if (!rq.d_out || rq.h_out || rq.defer || rq.spec || p.via_stage || p.by_kernels || p.inline_prep) return 0;
    return allowed & NM_ENQ_BOUND_EVENTS;
}

// Everything the scoring launch waits for, in the order the measured step time rests on: tables in, the timing pair, the
// programs (compiled here, or written by the spec source between its own clear and the scoring), the hand-over from the
// copy stream, the clear of the count table.
int score_prepare(nm_ctx *c, ScoreRun &r, uint32_t c_slots) {       // c_slots: bit s = mod slot s has canonical base C
    const ScorePlan &p = r.p;
    // a batch somebody waits for: tables in and outputs cleared by ONE kernel on its own stream (nmscan_internal.h: stage_in)
    if (p.by_kernels) {
        const int rc = stage_in(r.pst, r.hs, r.ds, p.total, r.out, p.clear_bytes);
        if (rc) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(r.ds, r.hs, p.total, hipMemcpyHostToDevice, r.pst));
    }
    r.e0 = c->ev0;
    r.e1 = c->ev1;
    r.timed_launch = c->ev_collect || !r.rq.defer;          // (a deferred batch of the search is not asked for its kernel time)
    if (c->ev_collect) {
        if (c->ev_used == c->ev_pool.size()) {
            if (c->ev_pool.size() >= EV_POOL_MAX) return fail(NM_ESTATE, "timing pool exhausted: call nm_timing_reset");
            HIP_TRY(ev_pool_grow(c));
        }
        r.e0 = c->ev_pool[c->ev_used].first;
        r.e1 = c->ev_pool[c->ev_used].second;
        c->ev_used += 1;
    }
    CandRec *const d_rec = reinterpret_cast<CandRec *>(r.ds);
    uint4 *const d_range = reinterpret_cast<uint4 *>(r.ds + p.off_range);
    const int fold_modpos = p.all_compact ? 1 : 0;
    switch (p.compile) {
    case PLAN_COMPILE_NONE: break;                       // nothing resident for this batch
    case PLAN_COMPILE_SPEC: {
        // counts and the writer's extra output: one clear; the writer (window kernel + children + their programs); timed with the scoring
        const SpecSource *spec = r.rq.spec;
        if (!p.by_kernels) HIP_TRY(hipMemsetAsync(r.ds + p.off_counts, 0, p.clear_bytes, r.pst));
        if (r.timed_launch) HIP_TRY(hipEventRecord(r.e0, r.pst));
        const SpecCompile cc{d_rec, reinterpret_cast<const uint32_t *>(r.ds + p.off_posof), r.ds + p.off_masks, d_range, r.d_prog, p.pdw, p.n_prog,
                             (int)p.np, p.any_wide, fold_modpos, p.cf ? 1 : 0};
        const int rc = spec->launch(r.pst, r.ds + p.off_xin, r.ds + p.off_xout, cc);
        if (rc) return rc;
        *spec->h_extra_out = r.hs + p.off_xout;
        break;
    }
    case PLAN_COMPILE_FUSED: {
        const size_t lds_bytes = (size_t)p.n_prog * p.pdw * 4 <= 48 * 1024 ? (size_t)p.n_prog * p.pdw * 4 : 0;
        hipLaunchKernelGGL(compile_common_kernel, dim3(1), dim3(1024), lds_bytes, r.pst, p.n_prog, d_rec, r.ds + p.off_masks, r.d_prog, p.any_wide, (int)p.np,
                           fold_modpos, p.n_entries, d_range, p.pdw, 8u, (uint32_t)(lds_bytes / 4));
        HIP_TRY(hipGetLastError());
        break;
    }
    case PLAN_COMPILE_ONLY:
    case PLAN_COMPILE_THEN_COMMON:
        hipLaunchKernelGGL(compile_kernel, dim3((p.n_prog + 255) / 256), dim3(256), 0, r.pst, p.n_prog, d_rec, r.ds + p.off_masks, r.d_prog, p.any_wide,
                           (int)p.np, fold_modpos, p.classes ? (p.cls_head ? 1 : 2) | p.cls_tail << 2 : 0, c_slots);
        HIP_TRY(hipGetLastError());
        if (p.compile == PLAN_COMPILE_THEN_COMMON) {
            hipLaunchKernelGGL(common_kernel, dim3((p.n_entries + 63) / 64), dim3(64), 0, r.pst, p.n_entries, d_range, r.d_prog, p.pdw, p.n_prog, 8u);
            HIP_TRY(hipGetLastError());
        }
        break;
    }
    if (!p.inline_prep) {
        HIP_TRY(hipEventRecord(c->copy_done, c->copy_stream));
        // strict order: the host waits for the compiled programs (tens of microseconds, the previous batch is still being
        // scored) and the scoring queue carries no cross-stream barrier packet — 5-6 us less between two launches; with two
        // lanes the host must run ahead instead, so there the stream waits
        if (r.laned || c->opt_stream_wait) HIP_TRY(hipStreamWaitEvent(r.sst, c->copy_done, 0));
        else HIP_TRY(hipEventSynchronize(c->copy_done));
    }
#ifdef NM_SCORE_PROBES
    // probe builds only (NM_CXXFLAGS=-DNM_SCORE_PROBES, tools/gpu_step_gap.sh): NM_SCORE_PROBE=1 leaves the clear out (the counts are garbage)
    static const int score_probe = getenv("NM_SCORE_PROBE") ? atoi(getenv("NM_SCORE_PROBE")) : 0;
#else
    constexpr int score_probe = 0;                       // (the shipped library has no switch that changes what a call computes)
#endif
    if (r.enq & NM_ENQ_BOUND_EVENTS) {
        // (never a spec or by_kernels batch: score_enqueue_form)  the timing pair's first event is complete when the clear is
        if (!(score_probe & 1) && p.clear_bytes) {
            const uint64_t n_words = p.clear_bytes / sizeof(unsigned long long);
            const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024, (n_words + 255) / 256);
            hipExtLaunchKernelGGL(clear_counts_kernel, dim3(blocks), dim3(256), 0, r.sst, nullptr, r.e0, 0, r.out, n_words);
            HIP_TRY(hipGetLastError());
        } else HIP_TRY(hipEventRecord(r.e0, r.sst));
        return NM_OK;
    }
    if (p.compile != PLAN_COMPILE_SPEC && !p.by_kernels && !(score_probe & 1)) HIP_TRY(hipMemsetAsync(r.out, 0, p.clear_bytes, r.sst));
    return NM_OK;
}

// Results out (through the pinned half of the pair, by a kernel or a copy engine), the pair released, the call's bookkeeping, and
// what the caller gets now: a note for nm_score_batch_end, the counts, or nothing (device counts).
int score_collect(nm_ctx *c, const ScoreRun &r, nm_ctx::Waiting &wait_slot) {
    const ScorePlan &p = r.p;
    if (p.via_stage && p.by_kernels) {
        const int rc = stage_out(r.sst, r.out, r.hs + p.off_counts, p.clear_bytes);
        if (rc) return rc;
    } else if (p.via_stage) HIP_TRY(hipMemcpyAsync(r.hs + p.off_counts, r.out, p.clear_bytes, hipMemcpyDeviceToHost, r.sst));
    // The pair's release marker.  Launches collected (nm_timing_reset(1)): e1 is this launch's own pool event, bound to the kernel that
    // reads the pair last — the pair remembers it and nothing is recorded.  Otherwise e1 is the ctx's one ev1, bound again by the next
    // call (a waiter would wait for the newest launch, not for this one): `busy` is recorded as before.
    if ((r.enq & NM_ENQ_BOUND_EVENTS) && c->ev_collect) nmdetail::release_stage_bound(c, r.e1);
    else {
        const int rc = release_stage(c, r.sst);
        if (rc) return rc;
    }
    c->last_enqueue = r.enq;
    c->cur_stage->last_out = r.rq.d_out;
    c->cur_stage->last_stream = r.sst;
    c->last_score_stream = r.sst;
    c->timed = !c->ev_collect && r.timed_launch;
    c->launches += 1;
    c->last_wgs = p.last_wgs;
    c->last_compact = p.all_compact ? p.n_prog : 0;
    c->last_general = p.all_compact ? 0 : p.n_prog;
    c->last_parked = p.n_prog && p.park;
    if (r.rq.defer) {
        nmdetail::wait_set(c, wait_slot, nm_ctx::Waiting{r.hs + p.off_counts, p.out_bytes, c->cur_stage, true});
    } else if (p.via_stage) {
        HIP_TRY(hipEventSynchronize(c->cur_stage->busy));
        memcpy(r.rq.h_out, r.hs + p.off_counts, p.out_bytes);
    } else if (r.rq.h_out) {
        HIP_TRY(hipMemcpyAsync(r.rq.h_out, r.out, p.out_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return NM_OK;
}

PlanFacts plan_facts(const nm_ctx *c) {
    PlanFacts f;
    f.n_bins = c->n_bins;
    f.bin_nchunks = c->bin_nchunks.data();
    f.bin_chunk0 = c->bin_chunk0.data();
    f.bin_ncontigs = c->bin_ncontigs.data();
    static_assert(NM_MAX_MOD_SLOTS <= 32, "one bit per mod slot");
    for (int sl = 0; sl < NM_MAX_MOD_SLOTS; ++sl) {
        f.slot_present |= (c->slots[sl].present ? 1u : 0u) << sl;
        f.slot_is_c |= (c->slots[sl].canonical == 'C' ? 1u : 0u) << sl;
    }
    f.n_segments = c->n_segments;
    for (int w = 0; w < 2; ++w) {
        f.list_start[w] = c->list_start[w].data();
        f.list_len[w] = c->list_len[w].data();
        f.list_segments[w] = c->n_list_segments[w];
    }
    f.seg_chunks = c->seg_chunks;
    f.n_cus = c->n_cus;
    f.opt_no_lit = c->opt_no_lit;
    f.opt_no_cf = c->opt_no_cf;
    f.opt_no_inline = c->opt_no_inline;
    f.opt_fine = c->opt_fine;
    f.opt_split = c->opt_split;
    return f;
}

// One scoring call: the batch is planned in the pure steps of nmscore_plan.h, then enqueued here — every HIP call of the scoring
// path is in this function, score_prepare or score_collect, in the order and on the streams the measured step time rests on.
int score_impl(nm_ctx *c, const ScoreRequest &rq) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    nm_ctx::Waiting &wait_slot = rq.spec ? c->spec_wait[rq.flight] : c->score_wait[rq.flight];
    if (rq.defer) {
        if (wait_slot.open) return fail(NM_ESTATE, "nm_score_batch_begin: the previous batch has not been collected (nm_score_batch_end)");
        nmdetail::wait_set(c, wait_slot, nm_ctx::Waiting{nullptr, 0, nullptr, true});
    }
    if (rq.n_cand == 0) return NM_OK;
    HIP_TRY(hipSetDevice(c->device));
    // ---- classify, shape, layout
    const PlanFacts f = plan_facts(c);
    c->bucket.assign((size_t)NM_MAX_MOD_SLOTS * f.n_bins + 1, 0);          // counting sort by (slot, bin)
    c->bin_active.assign(f.n_bins, 0);
    ScorePlan p;
    if (plan_classify(p, rq, f, c->bucket.data(), c->bin_active.data())) return fail(p.status, "%s", p.err);
    plan_shape(p, rq, f);
    plan_layout(p, rq);
    int rc = ensure_stage(c, p.via_stage ? p.stage_end : p.total, 1);
    if (rc) return rc;
    // ---- scoring lane of this call (nm_set_score_lanes): asynchronous device-output batches take the lane of their staging
    // pair — a pair, its half of the program table and its stream are reused together; every other call runs on the
    // ctx stream after the second lane has drained (a spec batch: on the stream it was given, the lanes left alone)
    ScoreRun r{rq, p};
    r.sst = rq.spec ? static_cast<hipStream_t>(rq.stream) : c->stream;
    r.laned = c->score_lanes == 2 && rq.d_out && !rq.h_out && !rq.defer;
    if (!r.laned && !rq.spec) {
        rc = join_lanes(c);
        if (rc) return rc;
    } else if (r.laned && ((c->cur_stage - c->stage) & 1)) {
        r.sst = c->lane_stream;
        c->lane_pending = true;
    }
    if (r.laned) {
        // two launches that write the same count table are ordered (memset, kernel) only within one stream: when an
        // earlier launch in flight wrote d_out from the other lane, this lane waits for it (its staging pair's event)
        for (auto &st : c->stage)
            if (&st != c->cur_stage && st.pending && st.last_out == rq.d_out && st.last_stream && st.last_stream != r.sst)
                HIP_TRY(hipStreamWaitEvent(r.sst, st.marker, 0));
    }
    // staged tables travel and are compiled on the copy stream; the scoring stream waits for the compiled programs.  A call
    // that returns host counts prepares on the scoring stream itself (plan_shape: inline_prep)
    r.pst = p.inline_prep ? r.sst : c->copy_stream;
    {
        const char *enq_env = getenv("NM_SCORE_ENQUEUE");
        r.enq = score_enqueue_form(rq, p, enq_env ? (uint32_t)atoi(enq_env) : ~0u);
    }
    // ---- fill
    r.hs = static_cast<uint8_t *>(c->h_stage);
    r.ds = static_cast<uint8_t *>(c->d_stage);
    plan_fill(p, rq, f, c->bucket.data(), c->bin_active.data(), r.hs);
    if (rq.spec && rq.spec->extra_in) rq.spec->fill_host(r.hs + p.off_xin);
    // ---- device-side program buffer: one part per staging pair, so that compiling the next batches (on the copy stream)
    // overlaps the scoring kernel of batch k; reuse of a part is gated like its staging pair (ensure_stage)
    static_assert(nmdetail::CLS_PROG_DW == 32, "a class program takes the room of a narrow 8-plane one");
    if (c->prog_cap_dw < p.prog_dw) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipStreamSynchronize(c->copy_stream));
        HIP_TRY(nmdetail::sync_flight_streams(c));
        rc = join_lanes(c);
        if (rc) return rc;
        if (c->d_programs) (void)nmdetail::dev_free(c->d_programs);
        c->d_programs = nullptr;
        c->prog_cap_dw = 0;
        HIP_TRY(nmdetail::dev_malloc(&c->d_programs, p.prog_dw * 2 * 4 * NM_STAGE_RING));
        c->prog_cap_dw = p.prog_dw * 2;
    }
    r.d_prog = c->d_programs + (size_t)(c->cur_stage - c->stage) * c->prog_cap_dw;
    // ---- output counters: the caller's table, the batch's own pair (spec), or the ctx's table
    r.out = rq.spec ? reinterpret_cast<unsigned long long *>(r.ds + p.off_counts) : rq.d_out;
    if (!r.out) {
        if (c->counts_cap < p.out_rows) {
            if (c->d_counts) (void)nmdetail::dev_free(c->d_counts);
            c->d_counts = nullptr;
            c->counts_cap = 0;
            HIP_TRY(nmdetail::dev_malloc(&c->d_counts, (size_t)p.out_rows * 2 * sizeof(unsigned long long) * 2));
            c->counts_cap = (size_t)p.out_rows * 2;
        }
        r.out = c->d_counts;
    }
    // ---- tables in, compile, clear
    rc = score_prepare(c, r, f.slot_is_c);
    if (rc) return rc;
    // ---- launch
    plan_geometry(p, f);
    ScoreArgs a{};
    a.seq = Planes{c->dH, c->dL, c->dV, c->d_needs_v};
    for (int s = 0; s < NM_MAX_MOD_SLOTS; ++s) {
        const ModSlot &ms = c->slots[s];
        a.st[s] = StatePlanes{ms.planes[0], ms.planes[1], ms.planes[2], ms.planes[3], ms.planes[4], ms.planes[5]};
        a.slot_is_c[s] = ms.canonical == 'C';
    }
    a.segments = p.own_segments ? reinterpret_cast<const uint4 *>(r.ds + p.off_segs) : p.use_list ? c->d_list_segments[p.pack] : c->d_segments;
    a.work_list = c->d_work_list[p.pack];
    a.strip_rows = c->d_strip_rows;
    a.n_segments = p.n_segments;
    a.n_bins = c->n_bins;
    a.programs = r.d_prog;
    a.orig_index = reinterpret_cast<uint32_t *>(r.ds + p.off_orig);
    a.cand_range = reinterpret_cast<uint4 *>(r.ds + p.off_range);
    a.out = r.out;
    a.chunk_rank = c->d_chunk_rank;
    a.row_base = reinterpret_cast<const uint64_t *>(r.ds + p.off_rows);
    for (uint32_t i = 0; i < p.n_active; ++i) a.active_slot[i] = p.active[i];
    a.split_log2 = p.split_log2;
    a.pieces_per_run = p.pieces_per_run;
    a.fine_log2 = p.fine_log2;
    a.j_big = p.j_big;
    const LaunchShape shape{p.any_wide, p.all_compact, p.lit, p.cf, p.fuse, p.per_contig, p.classes, p.park};
    if (r.enq & NM_ENQ_BOUND_EVENTS) {
        // two dispatches, no packet besides: e0 came with the clear (score_prepare), e1 comes with the scoring kernel — the measured
        // time is still the end of the clear to the end of the kernel
        if (p.n_prog) launch_score(a, p.gx, p.gy, shape, r.sst, r.e1);
        else HIP_TRY(hipEventRecord(r.e1, r.sst));             // (nothing resident for this batch: the zeroed table is the answer)
        HIP_TRY(hipGetLastError());
        return score_collect(c, r, wait_slot);
    }
    if (r.timed_launch && p.compile != PLAN_COMPILE_SPEC) HIP_TRY(hipEventRecord(r.e0, r.sst));
    if (p.n_prog) launch_score(a, p.gx, p.gy, shape, r.sst);   // else nothing resident for this batch: the zeroed table is the answer
    HIP_TRY(hipGetLastError());
    if (r.timed_launch) HIP_TRY(hipEventRecord(r.e1, r.sst));
    // ---- results out or deferral, bookkeeping
    return score_collect(c, r, wait_slot);
}

}  // namespace

// error sink for the other translation units of the library (nmbed.cpp)
int nm_set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" {

int nm_abi_version(void) { return 1; }

int nm_set_device_allocator(nm_alloc_fn alloc, nm_free_fn free_fn, void *user) {
    if ((alloc == nullptr) != (free_fn == nullptr)) return fail(NM_EINVAL, "give both functions or neither");
    // a block must go back to the allocator it came from: with a ctx alive its planes, staging buffers and tables would
    // be released through the other pair (hipFree on a pool sub-block, the pool's free on a hipMalloc pointer)
    if (nmdetail::g_live_ctx > 0 && (alloc != nmdetail::g_alloc || free_fn != nmdetail::g_free || user != nmdetail::g_alloc_user))
        return fail(NM_ESTATE, "nm_set_device_allocator with %d nm_ctx alive: destroy them first", nmdetail::g_live_ctx);
    nmdetail::g_alloc = alloc;
    nmdetail::g_free = free_fn;
    nmdetail::g_alloc_user = user;
    return NM_OK;
}

const char *nm_last_error(void) { return g_err.c_str(); }

static int ctx_init(nm_ctx *c) {
    c->opt_no_lit = getenv("NM_NO_LIT") != nullptr;
    c->opt_no_cf = getenv("NM_NO_CF") != nullptr;
    c->opt_no_inline = getenv("NM_NO_INLINE_PREP") != nullptr;
    c->opt_stream_wait = getenv("NM_STREAM_WAIT") != nullptr;      // A/B switch: never wait for the compile on the host
    if (const char *e = getenv("NM_FINE")) c->opt_fine = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("NM_SPLIT")) c->opt_split = std::max(0, std::min(2, atoi(e)));
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && cus > 0) c->n_cus = (uint32_t)cus;
    }
    if (const char *e = getenv("NM_SEG_CHUNKS")) c->seg_chunks = (uint32_t)std::max(4, atoi(e));
    HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    // the second scoring lane is made here, next to the first: the runtime deals its hardware queues to streams in
    // creation order, and two lanes that share a queue do not overlap (profiles/r2/lanes_queue_ab.txt)
    HIP_TRY(hipStreamCreateWithFlags(&c->lane_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->copy_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    HIP_TRY(nmdetail::dev_malloc(&c->d_err, sizeof(unsigned int)));
    HIP_TRY(nmdetail::dev_malloc(&c->d_other, sizeof(unsigned long long)));
    return NM_OK;
}

int nm_ctx_create(int device, nm_ctx **out) {
    if (!out) return fail(NM_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(NM_EINVAL, "device %d not in 0..%d", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    nm_ctx *c = new (std::nothrow) nm_ctx();
    if (!c) return fail(NM_ENOMEM, "out of host memory");
    c->device = device;
    c->stream = nullptr;
    nmdetail::g_live_ctx += 1;
    const int rc = ctx_init(c);
    if (rc != NM_OK) {                 // nm_ctx_destroy releases whatever was created (the error text is already set)
        const std::string keep = g_err;
        (void)nm_ctx_destroy(c);
        g_err = keep;
        return rc;
    }
    *out = c;
    return NM_OK;
}

static void free_assembly(nm_ctx *c) {
    drop_ingest_rows(c);
    nmdetail::free_readstats(c);
    void *ptrs[] = {c->dH /* owns L and V too */, c->d_needs_v, c->d_contig_chunk, c->d_contig_len, c->d_segments, c->d_chunk_rank,
                    c->d_work_list[0] /* owns both lists, the strips and the list segment tables */};
    c->d_chunk_rank = nullptr;
    for (int w = 0; w < 2; ++w) {
        c->d_work_list[w] = nullptr;
        c->d_list_segments[w] = nullptr;
        c->n_list_segments[w] = 0;
        c->list_start[w].clear();
        c->list_len[w].clear();
    }
    c->d_strip_rows = nullptr;
    for (void *p : ptrs)
        if (p) (void)nmdetail::dev_free(p);
    c->dH = c->dL = c->dV = nullptr;
    c->d_needs_v = nullptr;
    c->d_contig_chunk = nullptr;
    c->d_contig_len = nullptr;
    c->d_segments = nullptr;
    for (int b = 0; b < 4; ++b) {
        if (c->d_rank[b]) (void)nmdetail::dev_free(c->d_rank[b]);
        if (c->d_base_total[b]) (void)nmdetail::dev_free(c->d_base_total[b]);
        c->d_rank[b] = nullptr;
        c->d_base_total[b] = nullptr;
    }
    for (auto &s : c->slots) {
        free_slot_planes(s);
        s.present = false;
        s.n_rows = 0;
        drop_slot_ranks(s);
    }
}

int nm_ctx_destroy(nm_ctx *c) {
    if (!c) return NM_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);      // a registered pool's free does not wait like hipFree
    if (c->lane_stream) (void)hipStreamSynchronize(c->lane_stream);
    c->lane_pending = false;
    (void)nm_comm_destroy(c);
    free_assembly(c);
    for (auto &st : c->stage) {
        if (st.d) (void)nmdetail::dev_free(st.d);
        if (st.h) (void)hipHostFree(st.h);
        if (st.busy) (void)hipEventDestroy(st.busy);
    }
    if (c->d_counts) (void)nmdetail::dev_free(c->d_counts);
    if (c->d_programs) (void)nmdetail::dev_free(c->d_programs);
    if (c->d_spec_bg) (void)nmdetail::dev_free(c->d_spec_bg);
    for (int f = 0; f < NM_FLIGHTS; ++f) {
        if (c->d_spec_counts[f]) (void)nmdetail::dev_free(c->d_spec_counts[f]);
        if (c->d_flight_counts[f]) (void)nmdetail::dev_free(c->d_flight_counts[f]);
    }
    for (hipStream_t s : c->flight_stream) if (s) (void)hipStreamDestroy(s);
    if (c->d_win_planes) (void)nmdetail::dev_free(c->d_win_planes);
    if (c->d_win_alive) (void)nmdetail::dev_free(c->d_win_alive);
    if (c->d_win_tasks) (void)nmdetail::dev_free(c->d_win_tasks);
    if (c->d_err) (void)nmdetail::dev_free(c->d_err);
    if (c->d_other) (void)nmdetail::dev_free(c->d_other);
    for (auto &pr : c->ev_pool) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->copy_done) (void)hipEventDestroy(c->copy_done);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->lane_stream) (void)hipStreamDestroy(c->lane_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    nmdetail::g_live_ctx -= 1;
    return NM_OK;
}

int nm_set_stream(nm_ctx *c, void *hip_stream) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = join_lanes(c);
    if (rc) return rc;
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    c->last_score_stream = nullptr;
    c->timed = false;
    return NM_OK;
}

int nm_set_score_lanes(nm_ctx *c, int lanes) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (lanes != 1 && lanes != 2) return fail(NM_EINVAL, "lanes must be 1 or 2, got %d", lanes);
    HIP_TRY(hipSetDevice(c->device));
    int rc = join_lanes(c);
    if (rc) return rc;
    if (lanes == 2 && !c->lane_stream) HIP_TRY(hipStreamCreateWithFlags(&c->lane_stream, hipStreamNonBlocking));
    c->score_lanes = lanes;
    return NM_OK;
}

int nm_sync(nm_ctx *c) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return join_lanes(c);
}

static int upload_contigs_impl(nm_ctx *c, uint32_t n_contigs, const uint64_t *offsets, const uint32_t *bin_id,
                               uint32_t n_bins, const uint8_t *seq_ascii, bool on_device, const uint64_t *src_off = nullptr) {
    // src_off (device sources only): where each contig's bytes start in seq_ascii; NULL = back to back, at offsets[i]
    // n_contigs == 0 is a valid shard: a rank of a multi-GPU run that received no contig (more GPUs than pieces) holds
    // the bins' numbering and two pad chunks, scores every candidate to zero and still joins every collective
    if (!c || !offsets || (n_contigs && (!bin_id || !seq_ascii))) return fail(NM_EINVAL, "NULL argument");
    if (n_bins == 0) return fail(NM_EINVAL, "need at least one bin");
    if (offsets[0] != 0) return fail(NM_EINVAL, "offsets[0] must be 0");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    {
        const int rcj = join_lanes(c);
        if (rcj) return rcj;
    }
    free_assembly(c);
    // any failure below leaves the ctx WITHOUT an assembly (dH == nullptr, so scoring refuses) and frees the temporaries
    struct Rollback {
        nm_ctx *c;
        void *tmp[3] = {nullptr, nullptr, nullptr};
        bool keep = false;
        ~Rollback() {
            (void)hipStreamSynchronize(c->stream);          // nothing may still read the temporaries
            for (void *p : tmp)
                if (p) (void)nmdetail::dev_free(p);
            if (!keep) free_assembly(c);
        }
    } guard{c};
    c->n_contigs = n_contigs;
    c->n_bins = n_bins;
    c->contig_len.assign(n_contigs, 0);
    c->contig_bin.assign(bin_id, bin_id + (bin_id ? n_contigs : 0));
    c->contig_chunk.assign(n_contigs, 0);
    c->contig_nchunks.assign(n_contigs, 0);
    c->total_bp = offsets[n_contigs];
    for (uint32_t i = 0; i < n_contigs; ++i) {
        if (offsets[i + 1] <= offsets[i]) return fail(NM_EINVAL, "contig %u is empty (seq.py:70 asserts non-empty)", i);
        if (bin_id[i] >= n_bins) return fail(NM_EINVAL, "contig %u: bin %u >= n_bins %u", i, bin_id[i], n_bins);
        c->contig_len[i] = offsets[i + 1] - offsets[i];
        if (c->contig_len[i] >= 0xFFFFFFFFull - CHUNK_BP) return fail(NM_ERANGE, "contig %u longer than 4 Gbp", i);
    }
    // group contigs by bin; chunk 0 and the last chunk are zero pads for the halo reads
    std::vector<uint32_t> order(n_contigs);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return bin_id[x] < bin_id[y]; });
    c->bin_chunk0.assign(n_bins, 0);
    c->bin_nchunks.assign(n_bins, 0);
    c->bin_ncontigs.assign(n_bins, 0);
    c->contig_rank.assign(n_contigs, 0);
    uint64_t next = 1;
    std::vector<uint32_t> chunk_contig(1, 0xFFFFFFFFu);
    for (uint32_t oi = 0; oi < n_contigs; ++oi) {
        const uint32_t i = order[oi];
        const uint64_t nch = (c->contig_len[i] + GAP_BP + CHUNK_BP - 1) / CHUNK_BP;
        if (next + nch + 1 >= 0xFFFFFFFFull / CHUNK_WORDS * 8) return fail(NM_ERANGE, "assembly too large for one device context");
        c->contig_chunk[i] = (uint32_t)next;
        c->contig_nchunks[i] = (uint32_t)nch;
        const uint32_t b = bin_id[i];
        c->contig_rank[i] = c->bin_ncontigs[b]++;              // position of the contig inside its bin (upload order)
        if (c->bin_nchunks[b] == 0) c->bin_chunk0[b] = (uint32_t)next;
        c->bin_nchunks[b] += (uint32_t)nch;
        chunk_contig.insert(chunk_contig.end(), nch, i);
        next += nch;
    }
    chunk_contig.push_back(0xFFFFFFFFu);
    c->n_chunks = (uint32_t)(next + 1);
    const size_t words = plane_words(c);
    HIP_TRY(nmdetail::dev_malloc(&c->dH, words * 4 * 3));          // one block for H, L, V (see alloc_slot_planes)
    c->dL = c->dH + words;
    c->dV = c->dL + words;
    HIP_TRY(nmdetail::dev_malloc(&c->d_needs_v, c->n_chunks));
    HIP_TRY(hipMemsetAsync(c->dH, 0, words * 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->dL, 0, words * 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->dV, 0, words * 4, c->stream));
    HIP_TRY(nmdetail::dev_malloc(&c->d_contig_chunk, (size_t)std::max(n_contigs, 1u) * 4));
    HIP_TRY(nmdetail::dev_malloc(&c->d_contig_len, (size_t)std::max(n_contigs, 1u) * 8));
    HIP_TRY(hipMemcpyAsync(c->d_contig_chunk, c->contig_chunk.data(), (size_t)n_contigs * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_contig_len, c->contig_len.data(), (size_t)n_contigs * 8, hipMemcpyHostToDevice, c->stream));
    // temporaries for the pack pass
    uint8_t *d_ascii = nullptr;
    uint64_t *d_off = nullptr;
    uint32_t *d_chunk_contig = nullptr;
    if (on_device) d_ascii = const_cast<uint8_t *>(seq_ascii);
    else {
        HIP_TRY(nmdetail::dev_malloc(&d_ascii, std::max<uint64_t>(c->total_bp, 1)));
        guard.tmp[0] = d_ascii;
    }
    HIP_TRY(nmdetail::dev_malloc(&d_off, (size_t)(n_contigs + 1) * 8));
    guard.tmp[1] = d_off;
    HIP_TRY(nmdetail::dev_malloc(&d_chunk_contig, (size_t)c->n_chunks * 4));
    guard.tmp[2] = d_chunk_contig;
    if (!on_device && c->total_bp) HIP_TRY(hipMemcpyAsync(d_ascii, seq_ascii, c->total_bp, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_off, src_off ? src_off : offsets, (size_t)(n_contigs + (src_off ? 0 : 1)) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_chunk_contig, chunk_contig.data(), (size_t)c->n_chunks * 4, hipMemcpyHostToDevice, c->stream));
    {   // per chunk: rank of its contig within its bin (the row of the per-contig counters)
        std::vector<uint32_t> chunk_rank(c->n_chunks, 0);
        for (uint32_t ch = 0; ch < c->n_chunks; ++ch)
            if (chunk_contig[ch] != 0xFFFFFFFFu) chunk_rank[ch] = c->contig_rank[chunk_contig[ch]];
        HIP_TRY(nmdetail::dev_malloc(&c->d_chunk_rank, (size_t)c->n_chunks * 4));
        HIP_TRY(hipMemcpy(c->d_chunk_rank, chunk_rank.data(), (size_t)c->n_chunks * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemsetAsync(c->d_other, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(pack_kernel, dim3(c->n_chunks), dim3(256), 0, c->stream, d_ascii, d_off, c->d_contig_len, d_chunk_contig,
                       c->d_contig_chunk, c->dH, c->dL, c->dV, c->d_other);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(needs_v_kernel, dim3(c->n_chunks), dim3(CHUNK_WORDS), 0, c->stream, c->dV, c->d_needs_v, c->n_chunks);
    HIP_TRY(hipGetLastError());
    // static segment table: every bin's chunk range cut into pieces of SEG_CHUNKS
    std::vector<uint4> segs;
    for (uint32_t b = 0; b < n_bins; ++b)
        for (uint32_t k = 0; k < c->bin_nchunks[b]; k += c->seg_chunks)
            segs.push_back(make_uint4(c->bin_chunk0[b] + k, std::min<uint32_t>(c->seg_chunks, c->bin_nchunks[b] - k), b, 0));
    c->n_segments = (uint32_t)segs.size();
    HIP_TRY(nmdetail::dev_malloc(&c->d_segments, std::max<size_t>(segs.size(), 1) * sizeof(uint4)));
    if (!segs.empty()) HIP_TRY(hipMemcpyAsync(c->d_segments, segs.data(), segs.size() * sizeof(uint4), hipMemcpyHostToDevice, c->stream));
    unsigned long long other = 0;
    HIP_TRY(hipMemcpyAsync(&other, c->d_other, sizeof other, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->other_letters = other;
    {   // the work lists of the heavy kernels, plain and with the contigs' tails packed (nmscore_worklist.h), in one block:
        // plain list | packed list | strips of the packed rows | (16-byte aligned) segments of the plain list | of the packed list
        std::vector<uint8_t> needs_v(c->n_chunks);
        HIP_TRY(hipMemcpy(needs_v.data(), c->d_needs_v, c->n_chunks, hipMemcpyDeviceToHost));
        WorkList wl[2];
        for (int w = 0; w < 2; ++w)
            build_work_list(wl[w], w == 1, n_bins, n_contigs, order.data(), c->contig_bin.data(), c->contig_len.data(), c->contig_chunk.data(), needs_v.data(),
                            c->n_chunks, c->seg_chunks);
        const size_t o_list[2] = {0, wl[0].entries.size()}, o_strips = o_list[1] + wl[1].entries.size();
        const size_t o_segs0 = (o_strips + wl[1].strip_rows.size() + 3) & ~(size_t)3, o_segs1 = o_segs0 + wl[0].segs.size() * 4;
        const size_t o_segs[2] = {o_segs0, o_segs1}, total = o_segs1 + wl[1].segs.size() * 4;
        std::vector<uint32_t> blob(std::max<size_t>(total, 4), 0);
        for (int w = 0; w < 2; ++w) {
            std::copy(wl[w].entries.begin(), wl[w].entries.end(), blob.begin() + o_list[w]);
            if (!wl[w].segs.empty()) memcpy(blob.data() + o_segs[w], wl[w].segs.data(), wl[w].segs.size() * sizeof(PlanU4));
        }
        std::copy(wl[1].strip_rows.begin(), wl[1].strip_rows.end(), blob.begin() + o_strips);
        HIP_TRY(nmdetail::dev_malloc(&c->d_work_list[0], blob.size() * 4));
        HIP_TRY(hipMemcpy(c->d_work_list[0], blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
        c->d_work_list[1] = c->d_work_list[0] + o_list[1];
        c->d_strip_rows = c->d_work_list[0] + o_strips;
        for (int w = 0; w < 2; ++w) {
            c->d_list_segments[w] = reinterpret_cast<uint4 *>(c->d_work_list[0] + o_segs[w]);
            c->n_list_segments[w] = (uint32_t)wl[w].segs.size();
            c->list_start[w] = std::move(wl[w].bin_start);
            c->list_len[w] = std::move(wl[w].bin_len);
        }
    }
    guard.keep = true;
    return NM_OK;
}

static int upload_pileup_impl(nm_ctx *c, uint32_t mod_slot, uint8_t canonical_base, double low, double high,
                              uint64_t n_rows, const uint32_t *contig_id, const uint32_t *position,
                              const uint8_t *strand, const double *fraction_mod, int append, bool on_device) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs must come first");
    if (mod_slot >= NM_MAX_MOD_SLOTS) return fail(NM_EINVAL, "mod_slot %u >= %d", mod_slot, NM_MAX_MOD_SLOTS);
    if (canonical_base != 'A' && canonical_base != 'C') return fail(NM_EINVAL, "canonical base must be 'A' or 'C'");
    if (!(high > low)) return fail(NM_EINVAL, "high threshold must exceed low (find_motifs_bin.py:117-118)");
    if (n_rows && (!contig_id || !position || !strand || !fraction_mod)) return fail(NM_EINVAL, "NULL column");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));      // an asynchronous scoring launch may still read the planes replaced below
    {
        const int rcj = join_lanes(c);
        if (rcj) return rcj;
    }
    ModSlot &ms = c->slots[mod_slot];
    drop_slot_ranks(ms);
    const size_t words = plane_words(c);
    if (!ms.present || !append) {
        HIP_TRY(alloc_slot_planes(ms, words));
        HIP_TRY(hipMemsetAsync(ms.planes[0], 0, words * 4 * 6, c->stream));
        ms.n_rows = 0;
    } else if (ms.canonical != canonical_base || ms.low != low || ms.high != high) {
        return fail(NM_EINVAL, "append with different canonical base / thresholds than the slot holds");
    }
    ms.present = true;
    ms.canonical = canonical_base;
    ms.low = low;
    ms.high = high;
    if (n_rows == 0) return NM_OK;
    HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(unsigned int), c->stream));
    const uint32_t can_h = 0, can_l = canonical_base == 'C' ? 1u : 0u;   // A = 00, C = 01
    // host columns stream through the pinned staging ring in slabs; device columns are consumed in place
    const uint64_t slab = on_device ? n_rows : (8ull << 20);  // rows per slab (17 B each)
    for (uint64_t r0 = 0; r0 < n_rows; r0 += slab) {
        const uint64_t n = std::min(slab, n_rows - r0);
        const uint32_t *d_cid = contig_id + r0, *d_pos = position + r0;
        const uint8_t *d_str = strand + r0;
        const double *d_frac = fraction_mod + r0;
        int rc = NM_OK;
        if (!on_device) {
            const size_t o_pos = n * 4, o_frac = ((o_pos + n * 4) + 7) & ~(size_t)7, o_str = o_frac + n * 8;
            rc = ensure_stage(c, o_str + n);
            if (rc) return rc;
            uint8_t *hs = static_cast<uint8_t *>(c->h_stage), *ds = static_cast<uint8_t *>(c->d_stage);
            memcpy(hs, contig_id + r0, n * 4);
            memcpy(hs + o_pos, position + r0, n * 4);
            memcpy(hs + o_frac, fraction_mod + r0, n * 8);
            memcpy(hs + o_str, strand + r0, n);
            HIP_TRY(hipMemcpyAsync(ds, hs, o_str + n, hipMemcpyHostToDevice, c->stream));
            d_cid = reinterpret_cast<uint32_t *>(ds);
            d_pos = reinterpret_cast<uint32_t *>(ds + o_pos);
            d_str = ds + o_str;
            d_frac = reinterpret_cast<double *>(ds + o_frac);
        }
        hipLaunchKernelGGL(state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, d_cid, d_pos,
                           d_str, d_frac, low, high, c->d_contig_chunk, c->d_contig_len, c->n_contigs, can_h, can_l,
                           c->dH, c->dL, c->dV, ms.planes[0], ms.planes[1], ms.planes[2], ms.planes[3], ms.planes[4],
                           ms.planes[5], c->d_err);
        HIP_TRY(hipGetLastError());
        if (!on_device) {
            rc = release_stage(c);
            if (rc) return rc;
        }
    }
    unsigned int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, c->d_err, sizeof err, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (err) {
        // the planes already carry part of the bad rows: the slot goes back to "no pileup" (scoring then refuses it with
        // NM_ESTATE) instead of staying half-written; an append loses what the slot held before, which is corrupt too
        ms.present = false;
        ms.n_rows = 0;
    } else {
        ms.n_rows += n_rows;
    }
    if (err & 1u) return fail(NM_EINVAL, "pileup row with contig_id / position outside the uploaded assembly");
    if (err & 2u) return fail(NM_EINVAL, "pileup strand must be '+' or '-'");
    if (err & 4u) return fail(NM_EINVAL, "duplicate (contig, position, strand) rows: the reference's np.isin(assume_unique=True) requires unique positions (find_motifs_bin.py:1258)");
    return NM_OK;
}

int nm_upload_contigs(nm_ctx *c, uint32_t n_contigs, const uint64_t *offsets, const uint32_t *bin_id, uint32_t n_bins,
                      const uint8_t *seq_ascii) {
    return upload_contigs_impl(c, n_contigs, offsets, bin_id, n_bins, seq_ascii, false);
}

int nm_upload_contigs_device(nm_ctx *c, uint32_t n_contigs, const uint64_t *offsets, const uint32_t *bin_id,
                             uint32_t n_bins, const uint8_t *d_seq_ascii) {
    return upload_contigs_impl(c, n_contigs, offsets, bin_id, n_bins, d_seq_ascii, true);
}

}  // extern "C"

// the count table of a deferred batch of a flight: grown on demand behind the stream that may still write the old one
static int flight_table(nm_ctx *c, unsigned long long **table, size_t *cap, size_t rows, hipStream_t st) {
    if (*cap >= rows) return NM_OK;
    HIP_TRY(hipStreamSynchronize(st));
    if (*table) (void)nmdetail::dev_free(*table);
    *table = nullptr;
    *cap = 0;
    HIP_TRY(nmdetail::dev_malloc(table, rows * 2 * sizeof(unsigned long long) * 2));
    *cap = rows * 2;
    return NM_OK;
}

// the candidate arrays every entry point passes on
static ScoreRequest score_request(uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len = nullptr,
                                  const uint8_t *cand_modpos = nullptr, const uint32_t *cand_mask_offset = nullptr, const uint8_t *cand_masks = nullptr) {
    ScoreRequest rq;
    rq.n_cand = n_cand;
    rq.bin = cand_bin;
    rq.slot = cand_mod_slot;
    rq.len = cand_len;
    rq.modpos = cand_modpos;
    rq.mask_off = cand_mask_offset;
    rq.masks = cand_masks;
    return rq;
}

int nmdetail::score_batch_spec_begin(nm_ctx *c, int flight, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const SpecSource &spec,
                                     hipStream_t st) {
    if (n_cand && (!cand_bin || !cand_mod_slot)) return fail(NM_EINVAL, "NULL argument");
    ScoreRequest rq = score_request(n_cand, cand_bin, cand_mod_slot);
    rq.defer = true;
    rq.spec = &spec;
    rq.spec_mask_stride = spec.mask_stride;
    rq.spec_extra_in = spec.extra_in;
    rq.spec_extra_out = spec.extra_out;
    rq.stream = st;
    rq.flight = flight;
    const int rc = score_impl(c, rq);
    if (rc) nmdetail::wait_close(c, c->spec_wait[flight]);
    return rc;
}

int nmdetail::score_batch_flight_begin(nm_ctx *c, int flight, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                                       const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks) {
    if (!c || flight < 0 || flight >= NM_FLIGHTS) return fail(NM_EINVAL, "bad flight");
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks)) return fail(NM_EINVAL, "NULL argument");
    if (c->score_wait[flight].open) return fail(NM_ESTATE, "score batch: the previous batch of the flight has not been collected");
    int rc = flight_table(c, &c->d_flight_counts[flight], &c->flight_counts_cap[flight], n_cand, c->stream);
    if (rc) return rc;
    ScoreRequest rq = score_request(n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks);
    rq.d_out = c->d_flight_counts[flight];
    rq.defer = true;
    rq.flight = flight;
    rc = score_impl(c, rq);
    if (rc) nmdetail::wait_close(c, c->score_wait[flight]);
    return rc;
}

// the collecting half of a deferred batch; not_begun: what the entry point says when there is none
static int score_batch_end(nm_ctx *c, int flight, int64_t *out_counts, const char *not_begun) {
    if (!c->score_wait[flight].open) return fail(NM_ESTATE, "%s", not_begun);
    const nm_ctx::Waiting w = c->score_wait[flight];
    nmdetail::WaitCloser closer{c, &c->score_wait[flight], nullptr};          // (the pair stays held until the counts are copied out)
    if (w.bytes == 0) return NM_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(w.stage->busy));
    if (out_counts) memcpy(out_counts, w.h, w.bytes);           // NULL: the batch is dropped
    return NM_OK;
}

int nmdetail::score_batch_flight_end(nm_ctx *c, int flight, int64_t *out_counts) {
    if (!c || flight < 0 || flight >= NM_FLIGHTS) return fail(NM_EINVAL, "bad flight");
    return score_batch_end(c, flight, out_counts, "score batch end without begin");
}

// nmfasta.hip: the contigs picked out of a device-resident packed sequence (any subset, any order, a record more than once)
int nmdetail::upload_contigs_gather(nm_ctx *c, uint32_t n_contigs, const uint64_t *offsets, const uint64_t *src_off, const uint32_t *bin_id,
                                    uint32_t n_bins, const uint8_t *d_seq_ascii) {
    return upload_contigs_impl(c, n_contigs, offsets, bin_id, n_bins, d_seq_ascii, true, src_off);
}

extern "C" {

int nm_upload_pileup(nm_ctx *c, uint32_t mod_slot, uint8_t canonical_base, double low, double high, uint64_t n_rows,
                     const uint32_t *contig_id, const uint32_t *position, const uint8_t *strand,
                     const double *fraction_mod, int append) {
    return upload_pileup_impl(c, mod_slot, canonical_base, low, high, n_rows, contig_id, position, strand, fraction_mod,
                              append, false);
}

int nm_upload_pileup_device(nm_ctx *c, uint32_t mod_slot, uint8_t canonical_base, double low, double high,
                            uint64_t n_rows, const uint32_t *d_contig_id, const uint32_t *d_position,
                            const uint8_t *d_strand, const double *d_fraction_mod, int append) {
    return upload_pileup_impl(c, mod_slot, canonical_base, low, high, n_rows, d_contig_id, d_position, d_strand,
                              d_fraction_mod, append, true);
}

int nm_score_batch(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot,
                   const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset,
                   const uint8_t *cand_masks, int64_t *out_counts) {
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !out_counts))
        return fail(NM_EINVAL, "NULL argument");
    ScoreRequest rq = score_request(n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks);
    rq.h_out = out_counts;
    return score_impl(c, rq);
}

int nm_score_batch_wide(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint16_t *cand_len,
                        const uint16_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, int64_t *out_counts) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !out_counts)) return fail(NM_EINVAL, "NULL argument");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (n_cand == 0) return NM_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = join_lanes(c);
    if (rc) return rc;
    uint64_t mask_bytes = 0;
    uint32_t max_chunks = 0;
    ScorePlan check;                                                      // (carries the text of a refused motif)
    for (uint32_t k = 0; k < n_cand; ++k) {
        const uint32_t slot = cand_mod_slot[k], bin = cand_bin[k], len = cand_len[k];
        if (slot >= NM_MAX_MOD_SLOTS || !c->slots[slot].present) return fail(NM_ESTATE, "candidate %u uses mod slot %u with no pileup uploaded", k, slot);
        if (bin >= c->n_bins) return fail(NM_EINVAL, "candidate %u: bin %u >= n_bins %u", k, bin, c->n_bins);
        bool literal;
        if (check_motif(check, k, len, cand_modpos[k], cand_masks + cand_mask_offset[k], NM_MAX_WIDE_MOTIF_LEN, &literal)) return fail(check.status, "%s", check.err);
        mask_bytes = std::max<uint64_t>(mask_bytes, (uint64_t)cand_mask_offset[k] + len);
        max_chunks = std::max(max_chunks, c->bin_nchunks[bin]);
    }
    memset(out_counts, 0, (size_t)n_cand * 2 * sizeof(int64_t));
    if (max_chunks == 0) return NM_OK;                                    // none of the bins is resident on this rank
    // (plain synchronous staging: tables in, counts out; this path is not timed by anything)
    std::vector<uint32_t> chunk_contig(c->n_chunks, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < c->n_contigs; ++i)
        for (uint32_t q = 0; q < c->contig_nchunks[i]; ++q) chunk_contig[c->contig_chunk[i] + q] = i;
    const size_t o_bin = 0, o_off = o_bin + (size_t)n_cand * 4, o_len = o_off + (size_t)n_cand * 4, o_mp = o_len + (size_t)n_cand * 2,
                 o_slot = o_mp + (size_t)n_cand * 2, o_masks = (o_slot + n_cand + 15) & ~(size_t)15, o_b0 = (o_masks + mask_bytes + 15) & ~(size_t)15,
                 o_bn = o_b0 + (size_t)c->n_bins * 4, o_cc = o_bn + (size_t)c->n_bins * 4, o_out = (o_cc + (size_t)c->n_chunks * 4 + 15) & ~(size_t)15,
                 total = o_out + (size_t)n_cand * 16;
    std::vector<uint8_t> h(total, 0);
    memcpy(h.data() + o_bin, cand_bin, (size_t)n_cand * 4);
    memcpy(h.data() + o_off, cand_mask_offset, (size_t)n_cand * 4);
    memcpy(h.data() + o_len, cand_len, (size_t)n_cand * 2);
    memcpy(h.data() + o_mp, cand_modpos, (size_t)n_cand * 2);
    memcpy(h.data() + o_slot, cand_mod_slot, n_cand);
    memcpy(h.data() + o_masks, cand_masks, mask_bytes);
    memcpy(h.data() + o_b0, c->bin_chunk0.data(), (size_t)c->n_bins * 4);
    memcpy(h.data() + o_bn, c->bin_nchunks.data(), (size_t)c->n_bins * 4);
    memcpy(h.data() + o_cc, chunk_contig.data(), (size_t)c->n_chunks * 4);
    uint8_t *d = nullptr;
    HIP_TRY(nmdetail::dev_malloc(&d, total));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)nmdetail::dev_free(p); } } guard{d, c};
    HIP_TRY(hipMemcpyAsync(d, h.data(), total, hipMemcpyHostToDevice, c->stream));
    WideArgs a{};
    a.seq = Planes{c->dH, c->dL, c->dV, c->d_needs_v};
    for (int s = 0; s < NM_MAX_MOD_SLOTS; ++s) {
        const ModSlot &ms = c->slots[s];
        a.st[s] = StatePlanes{ms.planes[0], ms.planes[1], ms.planes[2], ms.planes[3], ms.planes[4], ms.planes[5]};
    }
    a.cand_bin = reinterpret_cast<const uint32_t *>(d + o_bin);
    a.cand_mask_off = reinterpret_cast<const uint32_t *>(d + o_off);
    a.cand_len = reinterpret_cast<const uint16_t *>(d + o_len);
    a.cand_modpos = reinterpret_cast<const uint16_t *>(d + o_mp);
    a.cand_slot = d + o_slot;
    a.masks = d + o_masks;
    a.bin_chunk0 = reinterpret_cast<const uint32_t *>(d + o_b0);
    a.bin_nchunks = reinterpret_cast<const uint32_t *>(d + o_bn);
    a.chunk_contig = reinterpret_cast<const uint32_t *>(d + o_cc);
    a.contig_chunk = c->d_contig_chunk;
    a.contig_len = c->d_contig_len;
    a.out = reinterpret_cast<unsigned long long *>(d + o_out);
    a.n_words = (long long)plane_words(c);
    hipLaunchKernelGGL(score_wide_kernel, dim3(max_chunks, n_cand), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_counts, d + o_out, (size_t)n_cand * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}

int nm_score_batch_begin(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot,
                         const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset,
                         const uint8_t *cand_masks) {
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks))
        return fail(NM_EINVAL, "NULL argument");
    if (c && c->score_wait[0].open) return fail(NM_ESTATE, "nm_score_batch_begin: the previous batch has not been collected (nm_score_batch_end)");
    ScoreRequest rq = score_request(n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks);
    rq.defer = true;
    const int rc = score_impl(c, rq);
    if (rc && c) c->score_wait[0].open = false;      // (a batch that failed half way is not open)
    return rc;
}

int nm_score_batch_end(nm_ctx *c, int64_t *out_counts) {                 // the flight-0 case of score_batch_flight_end
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    return score_batch_end(c, 0, out_counts, "nm_score_batch_end without nm_score_batch_begin");
}

int nm_score_batch_device(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot,
                          const uint8_t *cand_len, const uint8_t *cand_modpos, const uint32_t *cand_mask_offset,
                          const uint8_t *cand_masks, int64_t *d_out_counts) {
    if (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !d_out_counts))
        return fail(NM_EINVAL, "NULL argument");
    ScoreRequest rq = score_request(n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks);
    rq.d_out = reinterpret_cast<unsigned long long *>(d_out_counts);
    return score_impl(c, rq);
}

int nm_score_batch_per_contig(nm_ctx *c, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                              const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks,
                              const uint64_t *row_offset, int64_t *out_counts) {
    if (!row_offset || (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !out_counts)))
        return fail(NM_EINVAL, "NULL argument");
    if (row_offset[0] != 0) return fail(NM_EINVAL, "row_offset[0] must be 0");
    ScoreRequest rq = score_request(n_cand, cand_bin, cand_mod_slot, cand_len, cand_modpos, cand_mask_offset, cand_masks);
    rq.h_out = out_counts;
    rq.row_offset = row_offset;
    return score_impl(c, rq);
}

int nm_bin_contigs(nm_ctx *c, uint32_t bin, uint32_t *contig_ids, uint32_t capacity, uint32_t *n_contigs) {
    if (!c || !n_contigs) return fail(NM_EINVAL, "NULL argument");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (bin >= c->n_bins) return fail(NM_EINVAL, "bin %u >= n_bins %u", bin, c->n_bins);
    *n_contigs = c->bin_ncontigs[bin];
    if (contig_ids)
        for (uint32_t i = 0; i < c->n_contigs; ++i)
            if (c->contig_bin[i] == bin && c->contig_rank[i] < capacity) contig_ids[c->contig_rank[i]] = i;
    return NM_OK;
}

int nm_hit_positions(nm_ctx *c, uint32_t contig_id, uint32_t mod_slot, uint8_t len, uint8_t modpos, const uint8_t *masks,
                     int which, int64_t *out, uint64_t capacity, uint64_t *n_out) {
    if (!c || !masks || !n_out) return fail(NM_EINVAL, "NULL argument");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (contig_id >= c->n_contigs) return fail(NM_EINVAL, "contig_id %u >= %u", contig_id, c->n_contigs);
    if (mod_slot >= NM_MAX_MOD_SLOTS || !c->slots[mod_slot].present) return fail(NM_ESTATE, "mod slot %u has no pileup", mod_slot);
    if (which < 0 || which > 3) return fail(NM_EINVAL, "which must be 0..3");
    HIP_TRY(hipSetDevice(c->device));
    uint32_t full[PROG6_DW], prog[PROG6_DW];
    int reach = 0;
    int rc = compile_program(masks, len, modpos, full, &reach);
    if (rc) return rc;
    slice_program(full, reach + 1, prog);
    const uint32_t nch = c->contig_nchunks[contig_id];
    const size_t out_words = (size_t)nch * CHUNK_WORDS;
    // scratch: site masks of the contig | set bits per chunk | their exclusive prefix (+ total)
    const size_t o_cnt = PROG6_DW * 4 + out_words * 4, o_off = (o_cnt + (size_t)nch * 4 + 7) & ~(size_t)7;
    rc = ensure_stage(c, o_off + ((size_t)nch + 1) * 8);
    if (rc) return rc;
    memcpy(c->h_stage, prog, sizeof prog);
    HIP_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, sizeof prog, hipMemcpyHostToDevice, c->stream));
    uint8_t *ds = static_cast<uint8_t *>(c->d_stage);
    uint32_t *d_prog = reinterpret_cast<uint32_t *>(ds);
    uint32_t *d_masks = d_prog + PROG6_DW;
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(ds + o_cnt);
    unsigned long long *d_off = reinterpret_cast<unsigned long long *>(ds + o_off);
    const ModSlot &ms = c->slots[mod_slot];
    Planes seq{c->dH, c->dL, c->dV, c->d_needs_v};
    StatePlanes st{ms.planes[0], ms.planes[1], ms.planes[2], ms.planes[3], ms.planes[4], ms.planes[5]};
    dim3 grid((nch + 3) / 4);
    if (reach == 2) hipLaunchKernelGGL((hits_kernel<3, 3>), grid, dim3(256), 0, c->stream, seq, st, c->contig_chunk[contig_id], nch, d_prog, which, d_masks);
    else if (reach == 1) hipLaunchKernelGGL((hits_kernel<2, 2>), grid, dim3(256), 0, c->stream, seq, st, c->contig_chunk[contig_id], nch, d_prog, which, d_masks);
    else hipLaunchKernelGGL((hits_kernel<1, 1>), grid, dim3(256), 0, c->stream, seq, st, c->contig_chunk[contig_id], nch, d_prog, which, d_masks);
    HIP_TRY(hipGetLastError());
    // compaction on the device (popcount prefix + scatter): only the hit indices cross PCIe, not the contig's masks
    hipLaunchKernelGGL(hits_count_kernel, dim3(nch), dim3(256), 0, c->stream, d_masks, d_cnt);
    hipLaunchKernelGGL(hits_scan_kernel, dim3(1), dim3(256), 0, c->stream, d_cnt, nch, d_off);
    HIP_TRY(hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_off + nch, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t n = total, n_write = out ? std::min<uint64_t>(n, capacity) : 0;
    if (n_write) {
        long long *d_pos = nullptr;
        HIP_TRY(nmdetail::dev_malloc(&d_pos, n_write * 8));
        hipLaunchKernelGGL(hits_scatter_kernel, dim3(nch), dim3(256), 0, c->stream, d_masks, d_off, d_pos, (unsigned long long)n_write);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out, d_pos, n_write * 8, hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        (void)nmdetail::dev_free(d_pos);
        if (e != hipSuccess || e2 != hipSuccess) return fail(NM_EHIP, "hit compaction failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    }
    rc = release_stage(c);
    if (rc) return rc;
    *n_out = n;
    return NM_OK;
}

int nm_parse_motifs(uint32_t n, const char *text, const uint32_t *text_offset, const int32_t *mod_position,
                    uint8_t *out_len, uint8_t *out_modpos, uint32_t *out_mask_offset, uint8_t *out_masks,
                    uint64_t masks_capacity, uint64_t *masks_used) {
    if (n && (!text || !text_offset || !mod_position || !out_len || !out_modpos || !out_mask_offset || !out_masks || !masks_used))
        return fail(NM_EINVAL, "NULL argument");
    uint64_t used = 0;
    uint8_t tmp[4096];
    for (uint32_t k = 0; k < n; ++k) {
        const char *s = text + text_offset[k];
        const uint32_t slen = text_offset[k + 1] - text_offset[k];
        uint32_t nt = 0;
        for (uint32_t i = 0; i < slen;) {
            uint8_t m = 0;
            const char ch = s[i];
            if (ch == '[') {
                uint32_t j = i + 1;
                while (j < slen && s[j] != ']') {
                    const char b = s[j++];
                    m |= b == 'A' ? NM_BASE_A : b == 'C' ? NM_BASE_C : b == 'G' ? NM_BASE_G : b == 'T' ? NM_BASE_T : 0x80;
                }
                if (j >= slen) return fail(NM_EINVAL, "motif %u: unmatched '[' (motif.py:239)", k);
                if (m == 0 || (m & 0x80)) return fail(NM_EINVAL, "motif %u: a bracket may only list A, C, G, T", k);
                i = j + 1;
            } else {
                m = ch == 'A' ? NM_BASE_A : ch == 'C' ? NM_BASE_C : ch == 'G' ? NM_BASE_G : ch == 'T' ? NM_BASE_T
                    : ch == '.' ? 15 : 0;
                if (m == 0)
                    return fail(NM_EINVAL, "motif %u: character '%c' is not A/C/G/T/./[..] — the reference scans motifs as "
                                           "regular expressions (utils.py:61), other letters would be literals", k, ch);
                i += 1;
            }
            if (nt >= sizeof tmp) return fail(NM_ERANGE, "motif %u longer than %zu positions", k, sizeof tmp);
            tmp[nt++] = m;
        }
        uint32_t lo = 0, hi = nt;
        while (lo < nt && tmp[lo] == 15) ++lo;
        if (lo == nt) { lo = 0; }                      // all dots: left as is (motif.py:218-219), rejected at scoring
        else while (hi > lo && tmp[hi - 1] == 15) --hi;
        const uint32_t len = hi - lo;
        const int64_t mp = (int64_t)mod_position[k] - (int64_t)lo;
        if (len > NM_MAX_MOTIF_LEN) return fail(NM_ERANGE, "motif %u: stripped length %u > %d", k, len, NM_MAX_MOTIF_LEN);
        if (mp < 0 || mp >= (int64_t)len) return fail(NM_EINVAL, "motif %u: mod_position %d outside the stripped motif", k, mod_position[k]);
        if (used + len > masks_capacity) return fail(NM_ERANGE, "masks buffer too small");
        memcpy(out_masks + used, tmp + lo, len);
        out_len[k] = (uint8_t)len;
        out_modpos[k] = (uint8_t)mp;
        out_mask_offset[k] = (uint32_t)used;
        used += len;
    }
    *masks_used = used;
    return NM_OK;
}

int nm_stats(nm_ctx *c, uint64_t what[8]) {
    if (!c || !what) return fail(NM_EINVAL, "NULL argument");
    what[0] = c->total_bp;
    what[1] = (uint64_t)c->n_chunks * CHUNK_BP;
    what[2] = (uint64_t)plane_words(c) * 4 * 3;
    what[3] = (uint64_t)plane_words(c) * 4 * 2;
    what[4] = c->launches;
    what[5] = c->last_wgs;
    what[6] = c->last_compact;
    what[7] = c->last_general;
    return NM_OK;
}

int nm_last_score_parked(nm_ctx *c, int *parked) {
    if (!c || !parked) return fail(NM_EINVAL, "NULL argument");
    *parked = c->last_parked ? 1 : 0;
    return NM_OK;
}

int nm_last_score_enqueue(nm_ctx *c, uint32_t *flags) {
    if (!c || !flags) return fail(NM_EINVAL, "NULL argument");
    *flags = c->last_enqueue;
    return NM_OK;
}

int nm_timing_reset(nm_ctx *c, int enable) {
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    {
        const int rcj = join_lanes(c);          // the event pairs are reused: nothing may still be about to record them
        if (rcj) return rcj;
    }
    // A staging pair may remember a pool event as its release marker (score_collect).  The events are handed out again from here on,
    // so every such pair is drained here: both scoring streams have just been synchronised, the dispatch the event was bound to has
    // finished, and the pair is free — a later waiter must not find the event bound to a newer launch.
    for (auto &st : c->stage)
        if (st.pending && st.marker != st.busy) {
            st.pending = false;
            st.marker = st.busy;
        }
    c->ev_used = 0;
    c->ev_collect = enable != 0;
    c->ev_collect_all = enable == 2;
    c->busy_open = false;
    c->timed = false;
    return NM_OK;
}

int nm_timing_total_ms(nm_ctx *c, double *total_ms, uint64_t *n_launches) {
    if (!c || !total_ms || !n_launches) return fail(NM_EINVAL, "NULL argument");
    double tot = 0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        float ms = 0;
        HIP_TRY(hipEventSynchronize(c->ev_pool[i].second));
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_pool[i].first, c->ev_pool[i].second));
        tot += ms;
    }
    *total_ms = tot;
    *n_launches = c->ev_used;
    return NM_OK;
}

int nm_last_kernel_ms(nm_ctx *c, float *ms) {
    if (!c || !ms) return fail(NM_EINVAL, "NULL argument");
    if (!c->timed) return fail(NM_ESTATE, "no scoring launch recorded on this stream");
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NM_OK;
}

}  // extern "C"
