// Methylation of every k-mer context of a bin: for every A (or C) of a bin and every site of its complement on '-', the letters at the
// F counted offsets of a SHAPE around it are the row of a table [4^F][mod, nomod, nocall].  The other export units start from a motif;
// this one has none: no constraint program, no find_occurrences, and the reduction is a histogram keyed by the sequence itself.  What
// it shares with them are the resident planes, the chunk layout, RawChunk's loads, shifted<> and States (nmexport.h).
//   work item  = (request, run of R consecutive chunks of the request's bin): one workgroup of four waves, the waves take the run's
//                chunks in turn; the next chunk's loads are issued before the current one is walked (RawChunk::load waits for its
//                needs_v byte, though, and with it for the loads issued before: profiles/r20/motif_kmers.md, open).
//   digits     the public digit of a position is 2 H + (H ^ L) (A 0, C 1, G 2, T 3; the stored code is A 00, C 01, G 11, T 10) and
//                complementing is ~digit.  Per offset one v_alignbit of the H and the H ^ L words gives the two digit planes of a
//                lane's word: '+' sites shift by +o, '-' sites by -o and flip the assembled row.  Validity is the AND of the
//                shifted V words (only a boundary chunk has any): the GAP_BP invalid positions after a contig and an N make a
//                window incomplete without a special case.
//   histogram  the lane walks the set bits of its complete-site words, assembles the row from the digit planes and adds one to
//                [row][state]: in the workgroup's LDS table (F <= NM_KMER_LDS_FLANKS; zeroed once per work item, its non-zero cells
//                flushed with 64-bit atomics at the end of the run) or straight into the request's table (64-bit atomics).
//   totals     six counters per lane over the run (complete or not), summed over the wave once, one atomic per non-zero counter.
// A call is one launch plus the zeroing, whatever n_req is.  NM_KMER_GLOBAL_ATOMICS=1 forces the global path at any F and
// NM_KMER_RUN_CHUNKS=<1..4096> sets R; both are read per call (A/B runs; small test inputs cross run borders with them).
#include "nmexport.h"

using namespace nmdetail;

namespace {

constexpr int KMER_LDS_FLANKS = 6;                       // 4^6 x 3 uint32 = 48 KB: three workgroups per CU
constexpr uint32_t KMER_DEFAULT_RUN = 16, KMER_MAX_RUN = 4096;
// an LDS cell is a uint32: a run holds at most R x 8192 positions x 2 strands sites
static_assert((uint64_t)KMER_MAX_RUN * CHUNK_BP * 2 < (1ull << 32), "an LDS cell must hold every site of a run");

using KK = Variant<1, 1, false, 1, true, false>;

struct KmerReq {                                         // 48 bytes
    uint32_t chunk0, n_chunks, flip, pad;                // flip: all ones for canonical base C (L is flipped: C reads as A, G as T)
    unsigned long long planes[4];                        // MP UP MM UM of the slot
};
typedef const KmerReq __attribute__((address_space(4))) *creqp;

struct KmerArgs {
    Planes seq;
    const KmerReq *req;
    const uint32_t *run0;                                // [n_req + 1] prefix of the requests' run counts
    const uint32_t *shape;                               // [F] the offsets, ascending, as int32
    uint32_t n_req, run_chunks;
    unsigned long long *totals;                          // [n_req][2][3]
    unsigned long long *table;                           // [n_req][4^F][3]
};

// The sites of one chunk: totals into tot, complete sites into the histogram (LDS: tab, else rows).
template <int F, bool LDS>
__device__ __forceinline__ void kmer_chunk(const RawChunk<KK> &raw, uint32_t flip, const int (&sh)[F ? F : 1], uint32_t (&tot)[6], uint32_t *tab,
                                           unsigned long long *rows) {
    uint32_t x[T_WORDS + 2];
#pragma unroll
    for (int j = 0; j < T_WORDS + 2; ++j) x[j] = raw.h[j] ^ raw.l[j];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        const uint32_t hh = raw.h[t + 1], ll = raw.l[t + 1] ^ flip, vv = raw.v[t + 1];
        const uint32_t site[2] = {vv & ~hh & ~ll, vv & hh & ~ll};       // the canonical base; its complement: a site on '-'
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const States st(raw.s[0][2 * s][t], raw.s[0][2 * s + 1][t]);
#pragma unroll
            for (int i = 0; i < 3; ++i) tot[3 * s + i] += __popc(site[s] & st.s[i]);
            uint32_t hp[F ? F : 1], xp[F ? F : 1], ok = site[s];
#pragma unroll
            for (int f = 0; f < F; ++f) {
                int o = s ? -sh[f] : sh[f];                             // wave-uniform
                // pinned behind the walk of the previous word: left alone the compiler shifts all eight (word, strand) pairs'
                // planes ahead of the first walk (256 VGPRs at F = 6)
                asm volatile("" : "+s"(o));
                if (o > 0) {
                    hp[f] = shifted<true>(raw.h, t, (uint32_t)o);
                    xp[f] = shifted<true>(x, t, (uint32_t)o);
                    if (raw.need_v) ok &= shifted<true>(raw.v, t, (uint32_t)o);
                } else {
                    hp[f] = shifted<false>(raw.h, t, (uint32_t)(32 + o));
                    xp[f] = shifted<false>(x, t, (uint32_t)(32 + o));
                    if (raw.need_v) ok &= shifted<false>(raw.v, t, (uint32_t)(32 + o));
                }
            }
            const uint32_t m = st.s[0], u = st.s[1];
            while (ok) {
                const uint32_t b = (uint32_t)__builtin_ctz(ok);
                ok &= ok - 1;
                uint32_t row = 0;
#pragma unroll
                for (int f = 0; f < F; ++f) row = (row << 2) | ((hp[f] >> b & 1u) << 1) | (xp[f] >> b & 1u);
                if (s) row ^= (1u << (2 * F)) - 1u;                     // the complement of every digit
                const uint32_t cell = row * 3u + 2u - 2u * (m >> b & 1u) - (u >> b & 1u);
                if (LDS) atomicAdd(tab + cell, 1u);
                else atomicAdd(rows + cell, 1ull);
            }
        }
    }
}

template <int F, bool LDS>
__global__ __launch_bounds__(256) void kmer_kernel(KmerArgs a) {
    constexpr uint32_t CELLS = 3u << (2 * F);
    __shared__ uint32_t tab[LDS ? CELLS : 1];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the request of this work item: the last entry of the prefix that is <= it (scalar loads, scalar control flow)
    const cu32p run0 = (cu32p)a.run0;
    const uint32_t it = blockIdx.x;
    uint32_t lo = 0, hi = a.n_req;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (run0[mid] <= it) lo = mid; else hi = mid;
    }
    const creqp q = (creqp)a.req + lo;
    const uint32_t first = (it - run0[lo]) * a.run_chunks;
    const uint32_t n = min(a.run_chunks, q->n_chunks - first), chunk = q->chunk0 + first, flip = q->flip;
    StatePlanes stp[1];
    stp[0].M = stp[0].U = nullptr;
    stp[0].MP = reinterpret_cast<const uint32_t *>(q->planes[0]);
    stp[0].UP = reinterpret_cast<const uint32_t *>(q->planes[1]);
    stp[0].MM = reinterpret_cast<const uint32_t *>(q->planes[2]);
    stp[0].UM = reinterpret_cast<const uint32_t *>(q->planes[3]);
    int sh[F ? F : 1] = {};
#pragma unroll
    for (int f = 0; f < F; ++f) sh[f] = (int)((cu32p)a.shape)[f];
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < CELLS; i += 256) tab[i] = 0;
        __syncthreads();
    }
    unsigned long long *rows = a.table + (size_t)lo * CELLS;
    uint32_t tot[6] = {0, 0, 0, 0, 0, 0};
    RawChunk<KK> cur;
    if (wave < n) cur.load(a.seq, stp, chunk + wave, lane);
    for (uint32_t c = wave; c < n; c += 4) {                             // wave-uniform
        RawChunk<KK> nxt;
        const bool more = c + 4 < n;
        if (more) nxt.load(a.seq, stp, chunk + c + 4, lane);
        kmer_chunk<F, LDS>(cur, flip, sh, tot, tab, rows);
        if (more) cur = nxt;
    }
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) tot[j] += __shfl_xor(tot[j], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (tot[j]) atomicAdd(a.totals + (size_t)lo * 6 + j, (unsigned long long)tot[j]);
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < CELLS; i += 256) {
            const uint32_t v = tab[i];
            if (v) atomicAdd(rows + i, (unsigned long long)v);
        }
    }
}

typedef void (*KmerKernel)(KmerArgs);
constexpr KmerKernel kmer_global[NM_KMER_MAX_FLANKS + 1] = {kmer_kernel<0, false>, kmer_kernel<1, false>, kmer_kernel<2, false>, kmer_kernel<3, false>,
                                                            kmer_kernel<4, false>, kmer_kernel<5, false>, kmer_kernel<6, false>, kmer_kernel<7, false>,
                                                            kmer_kernel<8, false>, kmer_kernel<9, false>, kmer_kernel<10, false>};
constexpr KmerKernel kmer_lds[KMER_LDS_FLANKS + 1] = {kmer_kernel<0, true>, kmer_kernel<1, true>, kmer_kernel<2, true>, kmer_kernel<3, true>,
                                                      kmer_kernel<4, true>, kmer_kernel<5, true>, kmer_kernel<6, true>};

struct KmerBlock {                                       // the call's device block, freed however the call returns
    nm_ctx *c;
    uint8_t *d = nullptr;
    ~KmerBlock() {
        if (!d) return;
        (void)hipStreamSynchronize(c->stream);
        (void)dev_free(d);
    }
};

}  // namespace

int nm_kmer_methylation(nm_ctx *c, uint32_t n_req, const uint32_t *req_bin, const uint8_t *req_mod_slot, uint32_t n_offsets, const int8_t *offsets,
                        uint64_t *totals, uint64_t *table) {
    if (n_req && (!req_bin || !req_mod_slot || !totals || !table)) return fail(NM_EINVAL, "NULL argument");
    if (n_offsets && !offsets) return fail(NM_EINVAL, "NULL argument: offsets");
    if (n_offsets > NM_KMER_MAX_FLANKS) return fail(NM_EINVAL, "n_offsets %u above NM_KMER_MAX_FLANKS = %d", n_offsets, NM_KMER_MAX_FLANKS);
    for (uint32_t f = 0; f < n_offsets; ++f) {
        const int o = offsets[f];
        if (o == 0) return fail(NM_EINVAL, "offsets[%u] is 0: the modified base itself is not a counted position", f);
        if (o < -NM_KMER_MAX_OFFSET || o > NM_KMER_MAX_OFFSET) return fail(NM_EINVAL, "offsets[%u] = %d outside [-%d, %d]", f, o, NM_KMER_MAX_OFFSET, NM_KMER_MAX_OFFSET);
        if (f && o <= offsets[f - 1]) return fail(NM_EINVAL, "offsets[%u] = %d is not above offsets[%u] = %d: strictly ascending offsets are expected", f, o, f - 1, (int)offsets[f - 1]);
    }
    if (!c) return fail(NM_EINVAL, "ctx is NULL");
    if (n_req == 0) return NM_OK;
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    const int F = (int)n_offsets;
    const char *env_g = getenv("NM_KMER_GLOBAL_ATOMICS"), *env_r = getenv("NM_KMER_RUN_CHUNKS");
    const bool lds = F <= KMER_LDS_FLANKS && !(env_g && env_g[0] && env_g[0] != '0');
    uint32_t run_chunks = KMER_DEFAULT_RUN;
    if (env_r && env_r[0]) {
        const long v = strtol(env_r, nullptr, 10);
        if (v >= 1 && v <= (long)KMER_MAX_RUN) run_chunks = (uint32_t)v;
    }
    std::vector<KmerReq> req(n_req);
    std::vector<uint32_t> run0(n_req + 1, 0);
    uint64_t items = 0;
    for (uint32_t k = 0; k < n_req; ++k) {
        const uint32_t bin = req_bin[k];
        if (bin >= c->n_bins) return fail(NM_EINVAL, "request %u: req_bin %u >= n_bins %u", k, bin, c->n_bins);
        KmerReq &r = req[k];
        const int rc = slot_state_planes(c, "req_mod_slot", k, req_mod_slot[k], r.planes);
        if (rc) return rc;
        r.chunk0 = c->bin_chunk0[bin];
        r.n_chunks = c->bin_nchunks[bin];
        r.flip = c->slots[req_mod_slot[k]].canonical == 'C' ? 0xFFFFFFFFu : 0u;
        r.pad = 0;
        run0[k] = (uint32_t)items;
        items += (r.n_chunks + run_chunks - 1) / run_chunks;
    }
    // (one workgroup per work item: the grid's own limit is 2^31)
    if (items >= 0x7FFFFFF0ull) return fail(NM_ERANGE, "more than 2^32 (request, run of chunks) work items in one call: send fewer requests");
    run0[n_req] = (uint32_t)items;
    const size_t cells = (size_t)3 << (2 * F);
    int shape[NM_KMER_MAX_FLANKS + 1] = {};
    for (int f = 0; f < F; ++f) shape[f] = offsets[f];
    // ---- one device block: requests | run prefix | shape | totals, table (zeroed)
    const size_t o_run = align16(req.size() * sizeof(KmerReq)), o_shape = o_run + align16(run0.size() * 4), in_bytes = o_shape + align16(sizeof shape);
    const size_t tot_bytes = align16((size_t)n_req * 48), tab_bytes = align16((size_t)n_req * cells * 8);
    HIP_TRY(hipSetDevice(c->device));
    KmerBlock blk{c};
    HIP_TRY(dev_malloc(&blk.d, in_bytes + tot_bytes + tab_bytes));
    std::vector<uint8_t> h(in_bytes, 0);
    memcpy(h.data(), req.data(), req.size() * sizeof(KmerReq));
    memcpy(h.data() + o_run, run0.data(), run0.size() * 4);
    memcpy(h.data() + o_shape, shape, sizeof shape);
    HIP_TRY(hipMemcpyAsync(blk.d, h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                              // (h is pageable memory of this frame)
    HIP_TRY(hipMemsetAsync(blk.d + in_bytes, 0, tot_bytes + tab_bytes, c->stream));
    KmerArgs a;
    a.seq = seq_planes(c);
    a.req = reinterpret_cast<const KmerReq *>(blk.d);
    a.run0 = reinterpret_cast<const uint32_t *>(blk.d + o_run);
    a.shape = reinterpret_cast<const uint32_t *>(blk.d + o_shape);
    a.n_req = n_req;
    a.run_chunks = run_chunks;
    a.totals = reinterpret_cast<unsigned long long *>(blk.d + in_bytes);
    a.table = reinterpret_cast<unsigned long long *>(blk.d + in_bytes + tot_bytes);
    if (items) {                                                           // (every request in a bin without a resident contig: zeros)
        hipLaunchKernelGGL(lds ? kmer_lds[F] : kmer_global[F], dim3((uint32_t)items), dim3(256), 0, c->stream, a);
        HIP_TRY(hipGetLastError());
        c->launches += 1;
    }
    HIP_TRY(hipMemcpyAsync(totals, a.totals, (size_t)n_req * 48, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(table, a.table, (size_t)n_req * cells * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}
