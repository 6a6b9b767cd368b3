// nm_motif_sites_text — the records of nm_motif_sites as the lines of motif-sites.bed, on a few host threads — and
// nm_motif_compare_text, the records of nm_motif_compare_sites as the lines of switched-sites.bed: the same line with the
// transition "a>b" in the state column — and nm_motif_strands_text, the records of nm_motif_strands_sites as the lines of hemi-sites.bed:
// the pair "own-partner" in the state column and the partner's position in a ninth — and nm_motif_pileup_text, the records of
// nm_motif_pileup_sites as the lines of motif-pileup.bed: n_valid_cov in the score column, n_modified and the percentage in the state's place.
// The reference keeps the four position arrays of motif_model_contig(save_motif_positions=True) in memory
// (find_motifs_bin.py:1322-1329) and writes no per-site file; the line format is this project's (README.md).
// Two passes over the span: every thread sizes its share of the records exactly, the shares' offsets are a prefix sum, then every
// thread formats its share in place — the bytes are the same for any number of threads.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/nmscan.h"

int nm_set_error(int code, const char *fmt, ...);

namespace {

inline unsigned digits(uint64_t v) {
    unsigned n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}

inline char *put_u64(char *p, uint64_t v) {
    const unsigned n = digits(v);
    for (unsigned i = n; i-- > 0;) { p[i] = (char)('0' + v % 10); v /= 10; }
    return p + n;
}

// how a record's code reads: its label = text[code & mask] (n labels), its strand bit
struct Labels {
    const char *const *text;
    const unsigned *len;
    unsigned n, mask, minus;
};

const char *const STATE_TEXT[3] = {"mod", "nomod", "nocall"};
const unsigned STATE_LEN[3] = {3, 5, 6};
const Labels SITE_LABELS{STATE_TEXT, STATE_LEN, 3, 3u, NM_SITES_MINUS};
const char *const TRANSITION_TEXT[9] = {"mod>mod", "mod>nomod", "mod>nocall", "nomod>mod", "nomod>nomod", "nomod>nocall", "nocall>mod", "nocall>nomod",
                                        "nocall>nocall"};
const unsigned TRANSITION_LEN[9] = {7, 9, 10, 9, 11, 12, 10, 12, 13};
const Labels TRANSITION_LABELS{TRANSITION_TEXT, TRANSITION_LEN, 9, 15u, NM_COMPARE_MINUS};
const char *const PAIR_TEXT[9] = {"mod-mod", "mod-nomod", "mod-nocall", "nomod-mod", "nomod-nomod", "nomod-nocall", "nocall-mod", "nocall-nomod",
                                  "nocall-nocall"};
const Labels PAIR_LABELS{PAIR_TEXT, TRANSITION_LEN, 9, 15u, NM_STRANDS_MINUS};
const Labels PILEUP_LABELS{nullptr, nullptr, 2, NM_PILEUP_CODE_BARE, NM_PILEUP_MINUS};      // (no label: the values stand in the state's place)

// 100 mod / valid in hundredths, rounded half up in integers (valid > 0)
inline uint64_t percent_hundredths(uint64_t mod, uint64_t valid) { return (20000 * mod + valid) / (2 * valid); }

struct Span {
    const uint32_t *contig, *pos;
    const uint8_t *code;
    uint32_t n_seg;
    const uint64_t *seg_begin, *seg_text_off, *contig_text_off;
    const char *seg_text, *contig_text;
    Labels lab;
    const int32_t *seg_partner;                                          // per run the partner offset d (a ninth column), or NULL
    const uint32_t *valid, *mod;                                         // motif-pileup.bed: a record's n_valid_cov and n_modified, or NULL
    bool bare(uint64_t i) const { return code[i] & lab.mask; }
    // position of the partner of record i of run seg: pos + d on '+', pos - d on '-'
    int64_t partner(uint64_t i, uint32_t seg) const { return (int64_t)pos[i] + ((code[i] & lab.minus) ? -(int64_t)seg_partner[seg] : (int64_t)seg_partner[seg]); }
    // segment that holds record i (the last one whose begin is <= i; empty segments are passed over)
    uint32_t seg_of(uint64_t i) const { return (uint32_t)(std::upper_bound(seg_begin, seg_begin + n_seg + 1, i) - seg_begin) - 1; }
};

// bytes of the records [lo, hi), or their text at `out` (returns its end)
uint64_t size_range(const Span &s, uint64_t lo, uint64_t hi) {
    uint64_t bytes = 0;
    uint32_t seg = lo < hi ? s.seg_of(lo) : 0;
    for (uint64_t i = lo; i < hi; ++i) {
        while (i >= s.seg_begin[seg + 1]) ++seg;
        const uint64_t fixed = (s.seg_text_off[2 * seg + 2] - s.seg_text_off[2 * seg]) + 9;      // name + bin + 7 tabs + "0" + newline
        const uint32_t c = s.contig[i];
        const uint64_t p = s.pos[i];
        bytes += (s.contig_text_off[c + 1] - s.contig_text_off[c]) + digits(p) + digits(p + 1) + 1 + fixed;
        if (s.valid)                                                     // n_valid_cov for the "0", and n_modified \t [percent.dd] for the label
            bytes += digits(s.valid[i]) - 1 + digits(s.mod[i]) + 1 + (s.bare(i) ? 0 : digits(percent_hundredths(s.mod[i], s.valid[i]) / 100) + 3);
        else
            bytes += s.lab.len[s.code[i] & s.lab.mask];
        if (s.seg_partner) bytes += 1 + digits((uint64_t)s.partner(i, seg));
    }
    return bytes;
}

char *write_range(const Span &s, uint64_t lo, uint64_t hi, char *out) {
    uint32_t seg = lo < hi ? s.seg_of(lo) : 0;
    for (uint64_t i = lo; i < hi; ++i) {
        while (i >= s.seg_begin[seg + 1]) ++seg;
        const uint32_t c = s.contig[i];
        const uint64_t p = s.pos[i];
        const uint64_t cl = s.contig_text_off[c + 1] - s.contig_text_off[c];
        memcpy(out, s.contig_text + s.contig_text_off[c], cl);
        out += cl;
        *out++ = '\t';
        out = put_u64(out, p);
        *out++ = '\t';
        out = put_u64(out, p + 1);
        *out++ = '\t';
        const uint64_t nl = s.seg_text_off[2 * seg + 1] - s.seg_text_off[2 * seg];
        memcpy(out, s.seg_text + s.seg_text_off[2 * seg], nl);
        out += nl;
        *out++ = '\t';
        out = put_u64(out, s.valid ? s.valid[i] : 0);
        *out++ = '\t';
        *out++ = (s.code[i] & s.lab.minus) ? '-' : '+';
        *out++ = '\t';
        if (s.valid) {
            out = put_u64(out, s.mod[i]);
            *out++ = '\t';
            if (!s.bare(i)) {
                const uint64_t h = percent_hundredths(s.mod[i], s.valid[i]);
                out = put_u64(out, h / 100);
                *out++ = '.';
                *out++ = (char)('0' + h % 100 / 10);
                *out++ = (char)('0' + h % 10);
            }
        } else {
            const unsigned st = s.code[i] & s.lab.mask;
            memcpy(out, s.lab.text[st], s.lab.len[st]);
            out += s.lab.len[st];
        }
        *out++ = '\t';
        const uint64_t bl = s.seg_text_off[2 * seg + 2] - s.seg_text_off[2 * seg + 1];
        memcpy(out, s.seg_text + s.seg_text_off[2 * seg + 1], bl);
        out += bl;
        if (s.seg_partner) {
            *out++ = '\t';
            out = put_u64(out, (uint64_t)s.partner(i, seg));
        }
        *out++ = '\n';
    }
    return out;
}

int records_text(const Labels &lab, uint64_t n, const uint32_t *site_contig, const uint32_t *site_pos, const uint8_t *site_code, uint32_t n_seg,
                 const uint64_t *seg_begin, const char *seg_text, const uint64_t *seg_text_off, uint32_t n_contigs, const char *contig_text,
                 const uint64_t *contig_text_off, char *out, uint64_t capacity, uint64_t *n_bytes, const int32_t *seg_partner = nullptr,
                 bool with_partner = false, const uint32_t *site_valid = nullptr, const uint32_t *site_mod = nullptr, bool with_values = false) {
    if (!n_bytes) return nm_set_error(NM_EINVAL, "NULL argument");
    *n_bytes = 0;
    if (n == 0) return NM_OK;
    if (!site_contig || !site_pos || !site_code || !seg_begin || !seg_text || !seg_text_off || !contig_text || !contig_text_off || (with_partner && !seg_partner) ||
        (with_values && (!site_valid || !site_mod)))
        return nm_set_error(NM_EINVAL, "NULL argument");
    if (n_seg == 0 || seg_begin[0] != 0 || seg_begin[n_seg] != n) return nm_set_error(NM_EINVAL, "the runs must cover the %llu records exactly", (unsigned long long)n);
    for (uint32_t s = 0; s < n_seg; ++s)
        if (seg_begin[s + 1] < seg_begin[s]) return nm_set_error(NM_EINVAL, "seg_begin is not ascending at run %u", s);
    unsigned n_thr = std::max(1u, std::min(16u, std::thread::hardware_concurrency() / 2));
    if (const char *e = getenv("NM_POST_THREADS")) n_thr = (unsigned)std::max(1, std::min(16, atoi(e)));
    n_thr = (unsigned)std::min<uint64_t>(n_thr, (n + 255) / 256);        // (a thread is not worth starting for less)
    const Span sp{site_contig, site_pos, site_code, n_seg, seg_begin, seg_text_off, contig_text_off, seg_text, contig_text, lab, seg_partner, site_valid, site_mod};
    auto lo_of = [&](unsigned t) { return n * t / n_thr; };
    std::vector<uint64_t> bytes(n_thr + 1, 0);
    std::vector<int> bad(n_thr, 0);
    auto on_threads = [&](auto fn) {
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < n_thr; ++t) pool.emplace_back([&, t] { fn(t); });
        fn(0);
        for (auto &th : pool) th.join();
    };
    on_threads([&](unsigned t) {
        const uint64_t lo = lo_of(t), hi = lo_of(t + 1);
        for (uint64_t i = lo; i < hi; ++i)
            if (site_contig[i] >= n_contigs || (site_code[i] & lab.mask) >= lab.n || (site_code[i] & ~(lab.mask | lab.minus))) { bad[t] = 1; return; }
        if (seg_partner) {
            uint32_t seg = lo < hi ? sp.seg_of(lo) : 0;
            for (uint64_t i = lo; i < hi; ++i) {
                while (i >= seg_begin[seg + 1]) ++seg;
                if (sp.partner(i, seg) < 0) { bad[t] = 2; return; }
            }
        }
        if (site_valid)
            for (uint64_t i = lo; i < hi; ++i)
                if (!sp.bare(i) && (site_valid[i] == 0 || site_mod[i] > site_valid[i])) { bad[t] = 3; return; }
        bytes[t + 1] = size_range(sp, lo, hi);
    });
    for (unsigned t = 0; t < n_thr; ++t)
        if (bad[t] == 2) return nm_set_error(NM_EINVAL, "a record's partner lies before the start of its contig");
    for (unsigned t = 0; t < n_thr; ++t)
        if (bad[t] == 3) return nm_set_error(NM_EINVAL, "a site's n_valid_cov is 0 or below its n_modified");
    for (unsigned t = 0; t < n_thr; ++t)
        if (bad[t]) return nm_set_error(NM_EINVAL, "a record names a contig >= %u or carries a code that is none of the %u", n_contigs, 2 * lab.n);
    for (unsigned t = 0; t < n_thr; ++t) bytes[t + 1] += bytes[t];
    *n_bytes = bytes[n_thr];
    if (!out) return NM_OK;
    if (capacity < bytes[n_thr]) return nm_set_error(NM_ERANGE, "the text takes %llu bytes, the buffer holds %llu", (unsigned long long)bytes[n_thr], (unsigned long long)capacity);
    on_threads([&](unsigned t) { (void)write_range(sp, lo_of(t), lo_of(t + 1), out + bytes[t]); });
    return NM_OK;
}

}  // namespace

extern "C" int nm_motif_sites_text(uint64_t n, const uint32_t *site_contig, const uint32_t *site_pos, const uint8_t *site_code, uint32_t n_seg,
                                   const uint64_t *seg_begin, const char *seg_text, const uint64_t *seg_text_off, uint32_t n_contigs,
                                   const char *contig_text, const uint64_t *contig_text_off, char *out, uint64_t capacity, uint64_t *n_bytes) {
    return records_text(SITE_LABELS, n, site_contig, site_pos, site_code, n_seg, seg_begin, seg_text, seg_text_off, n_contigs, contig_text,
                        contig_text_off, out, capacity, n_bytes);
}

extern "C" int nm_motif_compare_text(uint64_t n, const uint32_t *site_contig, const uint32_t *site_pos, const uint8_t *site_code, uint32_t n_seg,
                                     const uint64_t *seg_begin, const char *seg_text, const uint64_t *seg_text_off, uint32_t n_contigs,
                                     const char *contig_text, const uint64_t *contig_text_off, char *out, uint64_t capacity, uint64_t *n_bytes) {
    return records_text(TRANSITION_LABELS, n, site_contig, site_pos, site_code, n_seg, seg_begin, seg_text, seg_text_off, n_contigs, contig_text,
                        contig_text_off, out, capacity, n_bytes);
}

extern "C" int nm_motif_strands_text(uint64_t n, const uint32_t *site_contig, const uint32_t *site_pos, const uint8_t *site_code, uint32_t n_seg,
                                     const uint64_t *seg_begin, const char *seg_text, const uint64_t *seg_text_off, const int32_t *seg_partner_offset,
                                     uint32_t n_contigs, const char *contig_text, const uint64_t *contig_text_off, char *out, uint64_t capacity,
                                     uint64_t *n_bytes) {
    return records_text(PAIR_LABELS, n, site_contig, site_pos, site_code, n_seg, seg_begin, seg_text, seg_text_off, n_contigs, contig_text,
                        contig_text_off, out, capacity, n_bytes, seg_partner_offset, true);
}

extern "C" int nm_motif_pileup_text(uint64_t n, const uint32_t *site_contig, const uint32_t *site_pos, const uint8_t *site_code, const uint32_t *site_valid,
                                    const uint32_t *site_mod, uint32_t n_seg, const uint64_t *seg_begin, const char *seg_text, const uint64_t *seg_text_off,
                                    uint32_t n_contigs, const char *contig_text, const uint64_t *contig_text_off, char *out, uint64_t capacity,
                                    uint64_t *n_bytes) {
    return records_text(PILEUP_LABELS, n, site_contig, site_pos, site_code, n_seg, seg_begin, seg_text, seg_text_off, n_contigs, contig_text,
                        contig_text_off, out, capacity, n_bytes, nullptr, false, site_valid, site_mod, true);
}
