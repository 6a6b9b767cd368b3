// Device side of the read-statistics lookup (included by nmmeth.hip, nmfractions.hip, nmpileup.hip and nmshift.hip, the units that read a site's
// (n_valid_cov, n_modified) by rank): a mod code's presence plane says where kept records sit, the rank table counts the records of
// the contig before every 512-bp block, and the records' values lie in plane (= position) order per strand — nothing is stored per
// base pair.  One wave holds one chunk, a lane T_WORDS = 4 words of it, so a 16-word rank block is four consecutive lanes.
#pragma once
#include "nmscan_device.h"

namespace nmdetail {

struct RsSlot {                              // the lookup tables of one read-statistics slot, per strand, as a kernel takes them
    const uint32_t *rank[2];
    const uint64_t *base[2];
    const uint2 *val[2];
};

// Host, the check a unit hands to stage_candidates: candidate k's read-statistics slot — refused when it holds no pileup, else its tables
// into rs[slot] and the addresses of its presence planes P+ P- into planes[0..1].
inline int stage_readstats_slot(const nm_ctx *c, uint32_t k, uint32_t slot, RsSlot *rs, unsigned long long *planes) {
    if (slot >= NM_MAX_MOD_SLOTS || !c->readstats[slot].present)
        return fail(NM_ESTATE, "candidate %u: read-statistics slot %u holds no pileup (nm_readstats_upload)", k, slot);
    const ReadStats &r = c->readstats[slot];
    planes[0] = (unsigned long long)(uintptr_t)r.planes;
    planes[1] = (unsigned long long)(uintptr_t)(r.planes + plane_words(c));
    rs[slot] = RsSlot{{r.rank[0], r.rank[1]}, {r.base[0], r.base[1]}, {r.val[0], r.val[1]}};
    return NM_OK;
}

// Value index of the first record of this lane's words on one strand: contig base + block rank + the records of the up to three
// lanes before it in its rank block.  pw: the lane's presence words.  Every lane of the wave must call it (lane shuffles).
__device__ __forceinline__ uint64_t first_record_index(const uint32_t (&pw)[T_WORDS], const uint64_t *base, const uint32_t *rank, uint32_t contig,
                                                       uint32_t chunk, int lane) {
    const uint32_t mine = __popc(pw[0]) + __popc(pw[1]) + __popc(pw[2]) + __popc(pw[3]);
    const uint32_t a1 = __shfl_up(mine, 1), a2 = __shfl_up(mine, 2), a3 = __shfl_up(mine, 3);
    const int q = lane & 3;
    const uint32_t before = (q >= 1 ? a1 : 0u) + (q >= 2 ? a2 : 0u) + (q >= 3 ? a3 : 0u);
    const uint32_t blk = chunk * RANK_PER_CHUNK + (uint32_t)(lane >> 2);
    return base[contig] + rank[blk] + before;
}

// f(value) for every bit of `sites` (a subset of the presence words pw) in ascending position; `first`: first_record_index of pw.
template <class F>
__device__ __forceinline__ void for_each_site_value(const uint32_t (&pw)[T_WORDS], const uint32_t (&sites)[T_WORDS], const uint2 *val, uint64_t first, F f) {
    uint64_t idx = first;
#pragma unroll
    for (int t = 0; t < T_WORDS; ++t) {
        uint32_t x = sites[t];
        while (x) {
            const uint32_t b = (uint32_t)__builtin_ctz(x);
            x &= x - 1;
            f(val[idx + __popc(pw[t] & ((1u << b) - 1u))]);
        }
        idx += __popc(pw[t]);
    }
}

}  // namespace nmdetail
