// Motif methylation INSIDE ANNOTATED REGIONS: a user's intervals (prophages, genes, repeat masks) as bit planes in the chunk space of the
// resident assembly, and the sites of every candidate counted and exported against them.  Two halves:
//   the region set   nm_regions: up to NM_REGION_MAX_CLASSES class planes of plane_words(ctx) words and one byte per chunk (which
//                    classes have a bit in the chunk), in a handle of its own as nm_bedcols / nm_fastadev are — the planes are not part
//                    of nm_ctx.  The handle keeps a COPY of the assembly's layout (contig_chunk, contig_len) and its device id: every call
//                    that takes (ctx, regions) compares the layouts, nm_regions_destroy never looks at a context.
//                    regions_raster_kernel: the host cuts an interval into pieces of at most P whole plane words, at multiples of P
//                    words from the contig's first word (a piece does not depend on where the interval starts); one wave per piece,
//                    lanes stride over its words, one atomicOr per word (the two edge masks, all-ones between them) — atomics
//                    everywhere: two intervals may meet inside one word.  The lanes 0.. OR the class bit into the byte of every chunk
//                    the piece touches, with a 32-bit atomic on the aligned word that holds the byte.
//                    regions_covered_kernel: one workgroup per (class, contig), the popcount of the contig's words.
//   the consumer     regions_kernel<G, FILL> on the scaffold of nmexport.h.  An occurrence and its state are nm_motif_sites'; it is
//                    INSIDE class c when the position of its modified base has its bit in plane c.
//          count  find_occurrences, return without an occurrence; one scalar load of the chunk's class byte and a wave-uniform loop over
//                 its set bits only: per class present the lane's T_WORDS words of the plane, one ballot that skips the class when it
//                 shares nothing with the occurrences, else six popcounts folded over the wave two counters to a dword (a wave holds at
//                 most 8192 sites per cell) and 64-bit atomics from lane 0 into the (candidate, contig) row — atomics: a contig of
//                 several chunks takes several work items.  The OUTSIDE cell is occurrences & ~(OR of the classes present).  A chunk
//                 without a class (the common case) costs sites_kernel's count and that one load.
//          fill   a record per occurrence whose state is in state_set and that is inside a class of class_set (or, want_outside,
//                 outside every uploaded class).  Beside nm_motif_sites' three columns it carries one byte more, the mask of ALL
//                 uploaded classes the site is inside: the fill loop and the window half are this unit's own, as in nmpileup.hip.
//                 The eight class words are held at static register indices (an unrolled loop with wave-uniform branches).
#include <cstdlib>

#include "nmexport.h"

using namespace nmdetail;

static_assert(T_WORDS == 4, "a lane's words of a class plane are one 16-byte load");

struct nm_regions {
    int device = 0;
    uint32_t n_classes = 0, n_chunks = 0;
    size_t words = 0;                          // of one plane
    std::vector<uint32_t> contig_chunk;        // the layout the planes were rasterised in
    std::vector<uint64_t> contig_len;
    uint32_t *planes = nullptr;                // [n_classes][words]; owns the allocation: chunk_classes and the layout lie behind the planes
    uint32_t *chunk_classes = nullptr;         // one byte per chunk, four to a word
    uint64_t *d_contig_len = nullptr;          // the layout again, for regions_covered_kernel
    uint32_t *d_contig_chunk = nullptr;
    uint64_t n_pieces = 0;
};

namespace {

constexpr uint32_t PIECE_MAX_WORDS = 2048;     // 65 536 bp

struct Piece {
    uint32_t w0, w1;                           // plane words [w0, w1) of the whole assembly
    uint32_t lo, hi;                           // masks of the words w0 and w1 - 1 (both on a piece of one word)
    uint32_t cls, pad;
};

__global__ __launch_bounds__(256) void regions_raster_kernel(const Piece *__restrict__ pieces, uint32_t n_pieces, uint32_t *__restrict__ planes, size_t words,
                                                             uint32_t *__restrict__ chunk_classes) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n_pieces) return;
    const Piece p = pieces[i];
    uint32_t *plane = planes + (size_t)p.cls * words;
    for (uint32_t w = p.w0 + lane; w < p.w1; w += 64) {
        uint32_t m = 0xFFFFFFFFu;
        if (w == p.w0) m &= p.lo;
        if (w == p.w1 - 1) m &= p.hi;
        atomicOr(plane + w, m);
    }
    const uint32_t c0 = p.w0 / CHUNK_WORDS, c1 = (p.w1 - 1) / CHUNK_WORDS;
    for (uint32_t c = c0 + lane; c <= c1; c += 64) atomicOr(chunk_classes + (c >> 2), (1u << p.cls) << ((c & 3u) * 8u));
}

__global__ __launch_bounds__(256) void regions_covered_kernel(const uint32_t *__restrict__ planes, size_t words, const uint32_t *__restrict__ contig_chunk,
                                                              const uint64_t *__restrict__ contig_len, uint32_t n_contigs,
                                                              unsigned long long *__restrict__ out) {
    __shared__ unsigned long long part[4];
    const uint32_t contig = blockIdx.x, cls = blockIdx.y;
    const uint32_t *p = planes + (size_t)cls * words + (size_t)contig_chunk[contig] * CHUNK_WORDS;
    const uint64_t nw = (contig_len[contig] + 31) / 32;
    unsigned long long n = 0;
    for (uint64_t w = threadIdx.x; w < nw; w += 256) n += __popc(p[w]);
    for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) out[(size_t)cls * n_contigs + contig] = part[0] + part[1] + part[2] + part[3];
}

uint32_t piece_words() {
    const char *e = getenv("NM_REGIONS_PIECE_WORDS");                    // read at every call: the piece borders within reach of a small contig
    if (!e || !*e) return PIECE_MAX_WORDS;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end) return PIECE_MAX_WORDS;
    return (uint32_t)std::min<long>(std::max<long>(v, 1), PIECE_MAX_WORDS);
}

bool same_layout(const nm_ctx *c, const nm_regions *r) {
    return r->n_chunks == c->n_chunks && r->contig_chunk == c->contig_chunk && r->contig_len == c->contig_len;
}

int check_layout(const nm_ctx *c, const nm_regions *r) {
    if (!same_layout(c, r)) return fail(NM_ESTATE, "the region set was made for another assembly than the one resident in ctx");
    return NM_OK;
}

// ------------------------------------------------------------------------------------------------ the consumer
struct RegionsArgs : ExportArgs {
    const uint32_t *cand_row0;               // first row of the candidate in the table
    const unsigned long long *cand_planes;   // [n_cand][4] MP UP MM UM of the candidate's mod slot
    const uint32_t *class_planes;            // plane c at class_planes + c * class_words (one allocation: a dynamic class index stays
    unsigned long long class_words;          //   address arithmetic, an array of pointers in the arguments would be copied to scratch)
    const uint32_t *chunk_classes;           // one byte per chunk: the classes with a bit in it
    uint32_t n_classes;
    uint32_t state_set;                      // NM_SITES_MOD | NM_SITES_NOMOD | NM_SITES_NOCALL
    uint32_t class_set;                      // 8 bits
    uint32_t want_outside;
    uint32_t n_rows;                         // rows of the table
    unsigned long long *table;               // count pass: [n_rows][n_classes + 1][2][3], may be NULL
    uint8_t *out_classes;                    // fill pass: the class mask, beside out_contig / out_pos / out_code
};

__device__ __forceinline__ uint32_t pick3(uint32_t set, const uint32_t (&s)[3]) {
    return ((set & 1u) ? s[0] : 0u) | ((set & 2u) ? s[1] : 0u) | ((set & 4u) ? s[2] : 0u);
}

// the six counts of the occurrences under `m` folded over the wave (two 16-bit counters to a dword: a wave's count is at most 8192) and
// added to cell[0..5] from lane 0
__device__ __forceinline__ void add_cell(unsigned long long *cell, const uint32_t (&f)[T_WORDS][3], const uint32_t (&r)[T_WORDS][3], const uint32_t (&m)[T_WORDS],
                                         int lane) {
    if (!cell) return;                                                    // wave-uniform: a call without a table
    uint32_t c[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] += (uint32_t)__popc(f[t][i] & m[t]) | ((uint32_t)__popc(r[t][i] & m[t]) << 16);
    }
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] += __shfl_xor(c[i], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (c[i] & 0xFFFFu) atomicAdd(cell + i, (unsigned long long)(c[i] & 0xFFFFu));
            if (c[i] >> 16) atomicAdd(cell + 3 + i, (unsigned long long)(c[i] >> 16));
        }
    }
}

template <int G, bool FILL>
__global__ __launch_bounds__(256) void regions_kernel(RegionsArgs a) {
    using K = Variant<G, G, false, 1, false, false>;
    const int lane = threadIdx.x & 63;
    WorkItem w;
    if (!locate_item<FILL>(a, w)) return;
    const uint32_t k = w.owner;
    const StatePlanes stp[1] = {slot_planes(a.cand_planes + (size_t)k * 4)};
    RawChunk<K> raw;
    Tile<K> tile;
    uint32_t af[T_WORDS], ar[T_WORDS];
    find_occurrences<K>(a, w, stp, lane, raw, tile, af, ar);
    uint32_t occ = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) occ |= af[t] | ar[t];
    if (!__any((int)(occ != 0))) return;                                 // wave-uniform: no occurrence in this chunk, its item count stays 0
    uint32_t f[T_WORDS][3], r[T_WORDS][3];
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) split_states(raw.s[0], t, af[t], ar[t], f[t], r[t]);
    // the classes with a bit in this chunk: one scalar load of the word that holds the chunk's byte
    const uint32_t present = __builtin_amdgcn_readfirstlane((((cu32p)a.chunk_classes)[w.chunk >> 2] >> ((w.chunk & 3u) * 8u)) & 0xFFu);
    const uint32_t *mine = a.class_planes + (size_t)w.chunk * CHUNK_WORDS + (size_t)lane * T_WORDS;
    const uint32_t set = a.state_set;
    if (!FILL) {
        const uint32_t row = ((cu32p)a.cand_row0)[k] + ((cu32p)a.chunk_rank)[w.chunk];
        unsigned long long *cells = (a.table && row < a.n_rows) ? a.table + (size_t)row * (a.n_classes + 1) * 6 : nullptr;
        uint32_t any[T_WORDS] = {0, 0, 0, 0}, chosen[T_WORDS] = {0, 0, 0, 0};
        for (uint32_t left = present; left; left &= left - 1) {          // wave-uniform: the classes present only
            const uint32_t c = (uint32_t)__builtin_ctz(left);
            const uint4 v = *reinterpret_cast<const uint4 *>(mine + (size_t)c * a.class_words);
            const uint32_t cw[T_WORDS] = {v.x, v.y, v.z, v.w};
            uint32_t hit = 0;
#pragma unroll
            for (int t = 0; t < T_WORDS; ++t) {
                any[t] |= cw[t];
                if (a.class_set >> c & 1u) chosen[t] |= cw[t];
                hit |= (af[t] | ar[t]) & cw[t];
            }
            if (__ballot(hit != 0) == 0) continue;                       // the class shares nothing with the occurrences of this chunk
            add_cell(cells ? cells + (size_t)c * 6 : nullptr, f, r, cw, lane);
        }
        uint32_t n = 0;
#pragma unroll
        for (int t = 0; t < T_WORDS; ++t) {
            any[t] = ~any[t];                                             // from here: outside every uploaded class
            const uint32_t sel = chosen[t] | (a.want_outside ? any[t] : 0u);
            n += __popc(pick3(set, f[t]) & sel) + __popc(pick3(set, r[t]) & sel);
        }
        add_cell(cells ? cells + (size_t)a.n_classes * 6 : nullptr, f, r, any, lane);
        for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
        if (lane == 0) a.item_cnt[w.item] = n;
        return;
    }
    // the class words at static indices; a class that is absent from the chunk is not loaded
    uint32_t cw[NM_REGION_MAX_CLASSES][T_WORDS];
#pragma unroll
    for (int c = 0; c < NM_REGION_MAX_CLASSES; ++c) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (present >> c & 1u) v = *reinterpret_cast<const uint4 *>(mine + (size_t)c * a.class_words);
        cw[c][0] = v.x; cw[c][1] = v.y; cw[c][2] = v.z; cw[c][3] = v.w;
    }
    uint32_t sf[T_WORDS], sr[T_WORDS], count = 0;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t any = 0, chosen = 0;
#pragma unroll
        for (int c = 0; c < NM_REGION_MAX_CLASSES; ++c) {
            any |= cw[c][t];
            if (a.class_set >> c & 1u) chosen |= cw[c][t];
        }
        const uint32_t sel = chosen | (a.want_outside ? ~any : 0u);
        sf[t] = pick3(set, f[t]) & sel;
        sr[t] = pick3(set, r[t]) & sel;
        count += __popc(sf[t]) + __popc(sr[t]);
    }
    // rank of the lane's first record = prefix of the item + records of the lanes before it (emit_records' first half)
    uint32_t incl = count;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    unsigned long long at = w.off0 + (incl - count) - a.first;          // relative to the window: one unsigned comparison covers both ends
    const uint32_t contig = ((cu32p)a.chunk_contig)[w.chunk];
    const uint32_t pos0 = (w.chunk - ((cu32p)a.contig_chunk)[contig]) * (uint32_t)CHUNK_BP + (uint32_t)lane * (T_WORDS * 32);
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t both = sf[t] | sr[t];
        while (both) {                                                  // ascending position, '+' before '-'
            const uint32_t b = __builtin_ctz(both), bit = 1u << b;
            both &= both - 1;
            uint32_t classes = 0;
#pragma unroll
            for (int c = 0; c < NM_REGION_MAX_CLASSES; ++c) classes |= (cw[c][t] >> b & 1u) << c;
            if (sf[t] & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos0 + t * 32 + b;
                    a.out_code[at] = (uint8_t)((f[t][0] & bit) ? 0u : (f[t][1] & bit) ? 1u : 2u);
                    a.out_classes[at] = (uint8_t)classes;
                }
                ++at;
            }
            if (sr[t] & bit) {
                if (at < a.capacity) {
                    a.out_contig[at] = contig;
                    a.out_pos[at] = pos0 + t * 32 + b;
                    a.out_code[at] = (uint8_t)((uint32_t)NM_SITES_MINUS | ((r[t][0] & bit) ? 0u : (r[t][1] & bit) ? 1u : 2u));
                    a.out_classes[at] = (uint8_t)classes;
                }
                ++at;
            }
        }
    }
}

template <bool FILL>
constexpr ExportKernels<RegionsArgs> regions_kernels = {regions_kernel<1, FILL>, regions_kernel<2, FILL>, regions_kernel<3, FILL>};
using RegionsBatch = ExportBatch<RegionsArgs>;

// the call-level checks of the two entry points behind their NULL checks, then the staging and the count pass
int regions_begin(RegionsBatch &rb, nm_ctx *c, const nm_regions *rg, const Candidates &cd, const uint8_t *cand_mod_slot, const uint64_t *cand_row0,
                  uint32_t state_set, uint32_t class_set, int want_outside, bool with_scan) {
    if (state_set == 0 || (state_set & ~7u)) return fail(NM_EINVAL, "state_set %u: a non-empty combination of NM_SITES_MOD / NOMOD / NOCALL", state_set);
    if (class_set >> rg->n_classes) return fail(NM_EINVAL, "class_set 0x%x names a class at or above n_classes %u", class_set, rg->n_classes);
    if (class_set == 0 && !want_outside) return fail(NM_EINVAL, "class_set is empty and want_outside is 0: nothing is selected");
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (const int rc = check_layout(c, rg)) return rc;
    if (cd.n == 0) return NM_OK;
    Staged st;
    const int rc = stage_candidates(c, cd, cand_mod_slot, cand_row0, false, st, no_check);
    if (rc) return rc;
    RegionsArgs &a = rb.base;
    a.class_planes = rg->planes;
    a.class_words = rg->words;
    a.chunk_classes = rg->chunk_classes;
    a.n_classes = rg->n_classes;
    a.state_set = state_set;
    a.class_set = class_set;
    a.want_outside = want_outside ? 1u : 0u;
    a.n_rows = (uint32_t)st.rows;
    std::vector<ExportTable> reserved;
    if (cand_row0) reserved.push_back({&a.table, (size_t)st.rows * (rg->n_classes + 1) * 48});
    return export_begin(rb, c, cd.n, cd.bin, st.width.data(), st.programs,
                        {{&a.cand_row0, st.row0.data(), st.row0.size() * 4}, {&a.cand_planes, st.planes.data(), st.planes.size() * 8}}, reserved,
                        regions_kernels<false>, with_scan);
}

}  // namespace

int nm_regions_create(nm_ctx *c, uint64_t n_intervals, const uint32_t *contig, const uint64_t *start, const uint64_t *end, const uint8_t *cls,
                      uint32_t n_classes, nm_regions **out) {
    if (!c || !out || (n_intervals && (!contig || !start || !end || !cls))) return fail(NM_EINVAL, "NULL argument");
    *out = nullptr;
    if (n_classes == 0 || n_classes > NM_REGION_MAX_CLASSES)
        return fail(NM_EINVAL, "n_classes %u: 1..NM_REGION_MAX_CLASSES = %d classes", n_classes, NM_REGION_MAX_CLASSES);
    if (!c->dH) return fail(NM_ESTATE, "nm_upload_contigs has not been called");
    if (plane_words(c) > 0xFFFFFFFFull) return fail(NM_ERANGE, "the assembly's planes hold more than 2^32 words");
    const uint32_t P = piece_words();
    std::vector<Piece> pieces;
    for (uint64_t i = 0; i < n_intervals; ++i) {
        const unsigned long long ii = i, s = start[i], e = end[i];
        if (contig[i] >= c->n_contigs) return fail(NM_EINVAL, "interval %llu: contig %u >= n_contigs %u", ii, contig[i], c->n_contigs);
        if (cls[i] >= n_classes) return fail(NM_EINVAL, "interval %llu: class %u >= n_classes %u", ii, (unsigned)cls[i], n_classes);
        if (s >= e) return fail(NM_EINVAL, "interval %llu: start %llu >= end %llu", ii, s, e);
        if (e > c->contig_len[contig[i]])
            return fail(NM_EINVAL, "interval %llu: end %llu past the contig's %llu positions", ii, e, (unsigned long long)c->contig_len[contig[i]]);
        // contig-local words [ws, we], cut at multiples of P words from the contig's first word
        const uint64_t ws = s / 32, we = (e - 1) / 32, base = (uint64_t)c->contig_chunk[contig[i]] * CHUNK_WORDS;
        for (uint64_t q = ws / P; q <= we / P; ++q) {
            const uint64_t a = std::max<uint64_t>(ws, q * P), b = std::min<uint64_t>(we + 1, (q + 1) * P);
            Piece p;
            p.w0 = (uint32_t)(base + a);
            p.w1 = (uint32_t)(base + b);
            p.lo = a == ws ? 0xFFFFFFFFu << (s % 32) : 0xFFFFFFFFu;
            p.hi = b == we + 1 ? 0xFFFFFFFFu >> (31 - (e - 1) % 32) : 0xFFFFFFFFu;
            p.cls = cls[i];
            p.pad = 0;
            pieces.push_back(p);
        }
        if (pieces.size() >= 0xFFFFFFF0ull) return fail(NM_ERANGE, "more than 2^32 pieces in one region set");
    }
    HIP_TRY(hipSetDevice(c->device));
    nm_regions *r = new nm_regions;
    bool waited = false;                                                  // the stream has drained: nothing reads this frame or the handle's vectors any more
    struct Fail {
        nm_regions *r; hipStream_t s; bool &waited; bool keep = false;
        ~Fail() { if (keep) return; if (!waited) (void)hipStreamSynchronize(s); (void)nm_regions_destroy(r); }
    } guard{r, c->stream, waited};
    r->device = c->device;
    r->n_classes = n_classes;
    r->n_chunks = c->n_chunks;
    r->words = plane_words(c);
    r->contig_chunk = c->contig_chunk;
    r->contig_len = c->contig_len;
    r->n_pieces = pieces.size();
    // one block: planes | chunk_classes | contig_len | contig_chunk | the pieces
    const size_t n_contigs = r->contig_len.size();
    const size_t o_cc = align16((size_t)n_classes * r->words * 4), o_len = o_cc + align16(((size_t)r->n_chunks + 3) / 4 * 4);
    const size_t o_chunk = o_len + align16(n_contigs * 8), o_end = o_chunk + align16(n_contigs * 4) + 16;
    uint8_t *d = nullptr;
    HIP_TRY(dev_malloc(&d, o_end));
    r->planes = reinterpret_cast<uint32_t *>(d);
    r->chunk_classes = reinterpret_cast<uint32_t *>(d + o_cc);
    r->d_contig_len = reinterpret_cast<uint64_t *>(d + o_len);
    r->d_contig_chunk = reinterpret_cast<uint32_t *>(d + o_chunk);
    HIP_TRY(hipMemsetAsync(d, 0, o_len, c->stream));
    if (n_contigs) {
        HIP_TRY(hipMemcpyAsync(r->d_contig_len, r->contig_len.data(), n_contigs * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(r->d_contig_chunk, r->contig_chunk.data(), n_contigs * 4, hipMemcpyHostToDevice, c->stream));
    }
    Piece *d_pieces = nullptr;
    struct Free {
        Piece *&p; hipStream_t s; bool &waited;
        ~Free() { if (!p) return; if (!waited) (void)hipStreamSynchronize(s); waited = true; (void)dev_free(p); }
    } pieces_guard{d_pieces, c->stream, waited};
    if (!pieces.empty()) {
        HIP_TRY(dev_malloc(&d_pieces, pieces.size() * sizeof(Piece)));
        HIP_TRY(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(Piece), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(regions_raster_kernel, dim3((uint32_t)((pieces.size() + 3) / 4)), dim3(256), 0, c->stream, d_pieces, (uint32_t)pieces.size(), r->planes,
                           r->words, r->chunk_classes);
        c->launches += 1;
    }
    const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(c->stream);   // one wait: the copies read memory of this frame
    waited = done == hipSuccess;
    HIP_TRY(launched);
    HIP_TRY(done);
    guard.keep = true;
    *out = r;
    return NM_OK;
}

int nm_regions_destroy(nm_regions *r) {
    if (!r) return NM_OK;
    (void)hipSetDevice(r->device);
    if (r->planes) (void)dev_free(r->planes);
    delete r;
    return NM_OK;
}

int nm_regions_shape(const nm_regions *r, uint32_t *n_classes, uint32_t *n_contigs, uint64_t *n_pieces) {
    if (!r) return fail(NM_EINVAL, "NULL argument");
    if (n_classes) *n_classes = r->n_classes;
    if (n_contigs) *n_contigs = (uint32_t)r->contig_len.size();
    if (n_pieces) *n_pieces = r->n_pieces;
    return NM_OK;
}

int nm_regions_covered(const nm_regions *r, uint64_t *bp) {
    if (!r || !bp) return fail(NM_EINVAL, "NULL argument");
    const uint32_t n_contigs = (uint32_t)r->contig_len.size();
    if (n_contigs == 0) return NM_OK;
    HIP_TRY(hipSetDevice(r->device));
    const size_t n = (size_t)r->n_classes * n_contigs;
    unsigned long long *d = nullptr;
    HIP_TRY(dev_malloc(&d, n * 8));
    struct Free { void *p; ~Free() { (void)hipStreamSynchronize(nullptr); (void)dev_free(p); } } guard{d};
    hipLaunchKernelGGL(regions_covered_kernel, dim3(n_contigs, r->n_classes), dim3(256), 0, nullptr, r->planes, r->words, r->d_contig_chunk, r->d_contig_len,
                       n_contigs, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(bp, d, n * 8, hipMemcpyDeviceToHost));
    return NM_OK;
}

int nm_regions_plane(const nm_regions *r, uint32_t cls, uint32_t contig, uint32_t *words) {
    if (!r || !words) return fail(NM_EINVAL, "NULL argument");
    if (cls >= r->n_classes) return fail(NM_EINVAL, "class %u >= n_classes %u", cls, r->n_classes);
    if (contig >= r->contig_len.size()) return fail(NM_EINVAL, "contig %u >= n_contigs %u", contig, (uint32_t)r->contig_len.size());
    const size_t nw = (size_t)((r->contig_len[contig] + 31) / 32);
    if (nw == 0) return NM_OK;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipMemcpy(words, r->planes + (size_t)cls * r->words + (size_t)r->contig_chunk[contig] * CHUNK_WORDS, nw * 4, hipMemcpyDeviceToHost));
    return NM_OK;
}

int nm_regions_chunk_classes(const nm_regions *r, uint32_t contig, uint8_t *classes, uint32_t capacity, uint32_t *n_chunks) {
    if (!r || !n_chunks) return fail(NM_EINVAL, "NULL argument");
    if (contig >= r->contig_len.size()) return fail(NM_EINVAL, "contig %u >= n_contigs %u", contig, (uint32_t)r->contig_len.size());
    const uint32_t n = (uint32_t)((r->contig_len[contig] + CHUNK_BP - 1) / CHUNK_BP);   // the chunks that hold a position of the contig
    *n_chunks = n;
    if (!classes) return NM_OK;
    if (capacity < n) return fail(NM_ERANGE, "capacity %u below the contig's %u chunks", capacity, n);
    if (n == 0) return NM_OK;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipMemcpy(classes, reinterpret_cast<const uint8_t *>(r->chunk_classes) + r->contig_chunk[contig], n, hipMemcpyDeviceToHost));
    return NM_OK;
}

int nm_motif_regions_count(nm_ctx *c, const nm_regions *rg, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                           const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t state_set, uint32_t class_set,
                           int want_outside, const uint64_t *cand_row0, uint64_t *cand_total, int64_t *counts) {
    if (!c || !cand_row0 || (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks || !counts)))
        return fail(NM_EINVAL, "NULL argument");
    if (!rg) return fail(NM_ESTATE, "no region set: nm_regions_create has not been called");
    RegionsBatch rb;
    int rc = regions_begin(rb, c, rg, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, cand_mod_slot, cand_row0, state_set, class_set,
                           want_outside, cand_total != nullptr);
    if (rc || n_cand == 0) return rc;
    const uint64_t rows = rb.base.n_rows;
    if (rows) HIP_TRY(hipMemcpyAsync(counts, rb.base.table, (size_t)rows * (rg->n_classes + 1) * 48, hipMemcpyDeviceToHost, c->stream));
    if (cand_total) {
        std::vector<uint64_t> off(n_cand + 1, 0);
        HIP_TRY(hipMemcpyAsync(off.data(), rb.d_owner_offset, (size_t)(n_cand + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < n_cand; ++k) cand_total[k] = off[k + 1] - off[k];
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return NM_OK;
}

int nm_motif_regions_sites(nm_ctx *c, const nm_regions *rg, uint32_t n_cand, const uint32_t *cand_bin, const uint8_t *cand_mod_slot, const uint8_t *cand_len,
                           const uint8_t *cand_modpos, const uint32_t *cand_mask_offset, const uint8_t *cand_masks, uint32_t state_set, uint32_t class_set,
                           int want_outside, uint64_t first_record, uint64_t capacity, uint32_t *site_contig, uint32_t *site_pos, uint8_t *site_code,
                           uint8_t *site_classes, uint64_t *cand_offset, uint64_t *n_written) {
    if (!c || !cand_offset || !n_written || (capacity && (!site_contig || !site_pos || !site_code || !site_classes)) ||
        (n_cand && (!cand_bin || !cand_mod_slot || !cand_len || !cand_modpos || !cand_mask_offset || !cand_masks)))
        return fail(NM_EINVAL, "NULL argument");
    *n_written = 0;
    if (!rg) return fail(NM_ESTATE, "no region set: nm_regions_create has not been called");
    RegionsBatch rb;
    const int rc = regions_begin(rb, c, rg, {n_cand, cand_bin, {cand_len, cand_modpos, cand_mask_offset, cand_masks}}, cand_mod_slot, nullptr, state_set,
                                 class_set, want_outside, true);
    if (rc) return rc;
    if (n_cand == 0) {
        cand_offset[0] = 0;
        return NM_OK;
    }
    // export_window of nmexport.h with four columns
    HIP_TRY(hipMemcpyAsync(cand_offset, rb.d_owner_offset, (size_t)(n_cand + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = cand_offset[n_cand];
    const uint64_t n = first_record >= total ? 0 : std::min<uint64_t>(capacity, total - first_record);
    if (n == 0) return NM_OK;
    uint8_t *d_out = nullptr;                                             // contig | pos | code | classes of the window's records
    const size_t col = align16((size_t)n * 4), bytes = align16((size_t)n);
    HIP_TRY(dev_malloc(&d_out, 2 * col + 2 * bytes));
    struct Free { uint8_t *p; nm_ctx *c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)dev_free(p); } } guard{d_out, c};
    RegionsArgs a = rb.base;
    a.first = first_record;
    a.capacity = n;
    a.out_contig = reinterpret_cast<uint32_t *>(d_out);
    a.out_pos = reinterpret_cast<uint32_t *>(d_out + col);
    a.out_code = d_out + 2 * col;
    a.out_classes = d_out + 2 * col + bytes;
    if (const int rc2 = rb.launch(regions_kernels<true>, a)) return rc2;
    HIP_TRY(hipMemcpyAsync(site_contig, a.out_contig, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_pos, a.out_pos, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_code, a.out_code, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(site_classes, a.out_classes, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_written = n;
    return NM_OK;
}
