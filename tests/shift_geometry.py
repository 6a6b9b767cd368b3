"""The input and the brute force of ``motif_shift`` (tests/test_motif_shift_host.py, tests/test_gpu_motif_shift.py): two samples joined at
every motif site.

Sample A is the geometry input of tests/test_read_methylation_host.py (``H.meth_input``): a 40 kbp contig with sites on 511 | 512, on
32 767 | 32 768 and in the four-lane block, contigs without records, the GA | TC contig border.  Sample B is derived from it record by
record under a seeded rule (``sample_b``) — dropped, dropped by either filter, kept as it is, kept at another coverage with the same
fraction, or drawn again — with records added where A has none, `edge` left without a B record (A only, between `small` and `mid` which
have both), `norec` given B records (B only, between `long` and `endGA`), and the hand-planted sites of `long` set by hand (``PLANTS_B``).
The candidates are those of tests/test_motif_pileup_host.candidates().

The brute force is the definition: plain Python and numpy over dense per-position tables and the site scan of
``H.site_positions``; integers only, the shifted rule in Python's big integers.  Per candidate, contig of its bin in bin order, position,
'+' before '-': the class of the occurrence (PAIRED / ONLY_A / ONLY_B / BARE), the two records, the direction (x = mB vA against
y = mA vB) and ``tmax`` = floor(1000 |x - y| / (vA vB)): the site is SHIFTED at t permille iff x != y and t <= tmax.

``LARGE`` is a second, tiny input: one contig of GATC repeats whose sites carry coverages up to 2^31 - 1 in both samples, chosen so that
the rule restated in wrapping 64-bit arithmetic and the rule restated in float64 each misjudge some of them."""
import functools

import numpy as np

import test_motif_fractions_host as F
import test_motif_pileup_host as P
import test_read_methylation_host as H
from nanomotif_amd.motif import iupac_to_regex

SEED_B = 29
EXTRA = 12
SUMS = ("occurrences", "n_paired", "n_only_a", "n_only_b", "sum_valid_a", "sum_mod_a", "sum_valid_b", "sum_mod_b", "n_up", "n_down", "n_shift_up", "n_shift_down")
PAIRED, ONLY_A, ONLY_B, BARE = 0, 1, 2, 3
EQUAL, UP, DOWN = 0, 1, 2
MINUS_BIT, DOWN_BIT = 4, 1
A_ONLY_CONTIG, B_ONLY_CONTIG = "edge", "norec"
ALL_B = (2, 3, 10, 16)
ALL_T = (0, 1, 250, 500, 501, 1000)
JOIN = np.dtype([("candidate", np.uint32), ("contig", np.uint32), ("pos", np.uint32), ("strand", np.uint8), ("cls", np.uint8), ("va", np.int64), ("ma", np.int64),
                 ("vb", np.int64), ("mb", np.int64), ("dir", np.uint8), ("tmax", np.int64)])
RECORD = np.dtype([("candidate", np.uint32), ("contig", np.uint32), ("pos", np.uint32), ("code", np.uint8), ("n_valid_a", np.uint32), ("n_mod_a", np.uint32),
                   ("n_valid_b", np.uint32), ("n_mod_b", np.uint32)])
# sample B at the hand-planted GATC sites of `long` (A: H.PLANTED): (coverage, modified)
PLANTS_B = {("long", 511, H.PLUS): (22, 6),            # 3 / 11 = 6 / 22: equal at another coverage, on the last bit of a rank block
            ("long", 512, H.MINUS): (12, 6),           # 12 / 12 -> 6 / 12: down by exactly 500
            ("long", 32_767, H.PLUS): (13, 13),        # 0 -> 1: up by 1000, below the 64-block carry
            ("long", 32_768, H.MINUS): (14, 7),        # unchanged, above the carry
            ("long", 36_863, H.PLUS): (30, 15),        # 15 / 15 -> 15 / 30: down by exactly 500
            ("long", 36_864, H.MINUS): (16, 9),        # 1 / 16 -> 9 / 16: up by exactly 500
            ("long", H.LANES_SITE, H.PLUS): (17, 6),   # 5 / 17 -> 6 / 17: up by 58.8: shifted at 58, not at 59
            ("long", H.LANES_SITE + 1, H.MINUS): (36, 18)}


# ------------------------------------------------------------------------------------------------ the rule
def judge(va, ma, vb, mb):
    """(direction, tmax) of one paired site in Python's integers."""
    x, y = int(mb) * int(va), int(ma) * int(vb)
    if x == y:
        return EQUAL, 0
    return (UP if x > y else DOWN), 1000 * abs(x - y) // (int(va) * int(vb))


def shifted(va, ma, vb, mb, t):
    x, y = int(mb) * int(va), int(ma) * int(vb)
    return x != y and 1000 * abs(x - y) >= int(t) * int(va) * int(vb)


def judge_wrapping(va, ma, vb, mb, t):
    """(direction, shifted) with every product and the comparison taken modulo 2^64: what a device without the 128-bit path computes."""
    M = (1 << 64) - 1
    x, y = int(mb) * int(va) & M, int(ma) * int(vb) & M
    d = (x - y if x > y else y - x) & M
    return (EQUAL if x == y else UP if x > y else DOWN), x != y and (1000 * d & M) >= (int(t) * (int(va) * int(vb) & M) & M)


def judge_float(va, ma, vb, mb, t):
    """(direction, shifted) in float64: fractions divided out, their difference against t / 1000."""
    fa, fb = float(ma) / float(va), float(mb) / float(vb)
    return (EQUAL if fa == fb else UP if fb > fa else DOWN), fa != fb and abs(fb - fa) >= float(t) / 1000.0


def site_bin(m, v, B):
    return min(B - 1, int(m) * B // int(v))


# ------------------------------------------------------------------------------------------------ sample B
@functools.lru_cache(maxsize=None)
def sample_b():
    """{(name, code): columns} of sample B, in ascending (position, strand) order."""
    names, seqs, rec_a = H.meth_input()
    rng = np.random.default_rng(SEED_B)
    out = {}
    for code, extra in (("a", 0.12), ("m", 0.10)):
        for name in names:
            if name == A_ONLY_CONTIG:
                continue
            L = len(seqs[name])
            cols = {}
            r = rec_a.get((name, code))
            if r is not None:
                n = len(r["position"])
                u = rng.random(n)
                nv2, nm2 = rng.integers(3, 41, size=n), rng.integers(0, 41, size=n)
                for i, (p, st, nv, nm, nd) in enumerate(zip(r["position"].tolist(), r["strand"].tolist(), r["n_valid"].tolist(), r["n_mod"].tolist(), r["n_diff"].tolist())):
                    if (nv, nm) == (4, 1):
                        cols[(p, st)] = (4, 3, 1)                         # 1 / 4 -> 3 / 4: shifted at 500, not at 501
                    elif (nv, nm) == (4, 2):
                        cols[(p, st)] = (6, 3, 0)                         # 2 / 4 against 3 / 6: equal
                    elif u[i] < 0.15:
                        continue                                         # no record in B
                    elif u[i] < 0.20:
                        cols[(p, st)] = (2, 1, 0)                         # dropped by the coverage filter
                    elif u[i] < 0.25:
                        cols[(p, st)] = (max(nv, 3), min(nm, max(nv, 3)), max(nv, 3))      # dropped by the n_diff filter (0.5 < 0.8)
                    elif u[i] < 0.45:
                        cols[(p, st)] = (nv, nm, nd)                      # unchanged (kept or dropped as in A)
                    elif u[i] < 0.55:
                        cols[(p, st)] = (2 * nv, 2 * nm, 0)               # the same fraction at twice the coverage
                    else:
                        cols[(p, st)] = (int(nv2[i]), int(nm2[i]) % (int(nv2[i]) + 1), 0)
            density = 0.5 if name == B_ONLY_CONTIG else extra
            p, s = np.nonzero(rng.random((L, 2)) < density)              # records where A may have none
            nv3, nm3 = rng.integers(3, 31, size=len(p)), rng.integers(0, 31, size=len(p))
            for i, (pp, ss) in enumerate(zip(p.tolist(), s.tolist())):
                key = (pp, H.MINUS if ss else H.PLUS)
                if key not in cols and not (r is not None and _has(r, key)):
                    cols[key] = (int(nv3[i]), int(nm3[i]) % (int(nv3[i]) + 1), 0)
            if code == "a":
                for (n2, pos, strand), (cov, mod) in PLANTS_B.items():
                    if n2 == name:
                        cols[(pos, strand)] = (cov, mod, 0)
            if not cols:
                continue
            keys = sorted(cols)
            col = lambda j: np.array([cols[k][j] for k in keys], dtype=np.int64)
            out[(name, code)] = dict(position=np.array([k[0] for k in keys], dtype=np.int64), strand=np.array([k[1] for k in keys], dtype=np.uint8), n_valid=col(0),
                                     n_mod=col(1), n_diff=col(2))
    for r in out.values():
        for a in r.values():
            a.setflags(write=False)
    return out


_KEYS = {}


def _has(r, key):
    s = _KEYS.get(id(r))
    if s is None:
        s = _KEYS[id(r)] = set(zip(r["position"].tolist(), r["strand"].tolist()))
    return key in s


# ------------------------------------------------------------------------------------------------ the brute force
def join_records(names, seqs, rec_a, rec_b, bins_of, cands, min_cov=H.MIN_COV, min_frac=H.MIN_FRAC):
    """JOIN[]: every occurrence of every candidate (IUPAC motif, code, mod position, bin) in output order; ``contig`` indexes ``names``."""
    dense_a, dense_b = F.dense_records(seqs, rec_a, min_cov, min_frac), F.dense_records(seqs, rec_b, min_cov, min_frac)
    cache, parts = {}, []
    for k, (motif, code, pos, b) in enumerate(cands):
        for name in bins_of[b]:
            key = (motif, pos, name)
            if key not in cache:
                cache[key] = H.site_positions(seqs[name], iupac_to_regex(motif), pos)
            fwd, rev = cache[key]
            at = np.concatenate([fwd, rev]).astype(np.int64)
            strand = np.concatenate([np.zeros(len(fwd), np.int64), np.ones(len(rev), np.int64)])
            order = np.lexsort((strand, at))
            at, strand = at[order], strand[order]
            rec = np.zeros(len(at), dtype=JOIN)
            rec["candidate"], rec["contig"], rec["pos"], rec["strand"] = k, names.index(name), at, strand
            have = []
            for dense, v, m in ((dense_a, "va", "ma"), (dense_b, "vb", "mb")):
                d = dense.get((name, code))
                cov = d[0][strand, at] if d is not None else np.full(len(at), -1, np.int64)
                have.append(cov >= 0)
                rec[v] = np.where(cov >= 0, cov, 0)
                rec[m] = np.where(cov >= 0, d[1][strand, at], 0) if d is not None else 0
            rec["cls"] = np.where(have[0] & have[1], PAIRED, np.where(have[0], ONLY_A, np.where(have[1], ONLY_B, BARE)))
            for i in np.flatnonzero(rec["cls"] == PAIRED).tolist():
                rec["dir"][i], rec["tmax"][i] = judge(rec["va"][i], rec["ma"][i], rec["vb"][i], rec["mb"][i])
            parts.append(rec)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=JOIN)


def tables(join, names, bins_of, cands, B, t):
    """[uint64[n_contigs, 2, B * B + 12]] per candidate: what nm_motif_shift_count writes."""
    out = []
    start = np.searchsorted(join["candidate"], np.arange(len(cands) + 1))
    for k, c in enumerate(cands):
        mine = join[start[k]:start[k + 1]]
        tab = np.zeros((len(bins_of[c[3]]), 2, B * B + EXTRA), dtype=np.uint64)
        for i, name in enumerate(bins_of[c[3]]):
            here = mine[mine["contig"] == names.index(name)]
            for s in (0, 1):
                on = here[here["strand"] == s]
                pair = on[on["cls"] == PAIRED]
                if len(pair):                                             # site_bin on int64 columns: m B < 2^35
                    cell = np.minimum(B - 1, pair["ma"] * B // pair["va"]) * B + np.minimum(B - 1, pair["mb"] * B // pair["vb"])
                    tab[i, s, :B * B] = np.bincount(cell, minlength=B * B)
                up, down = pair["dir"] == UP, pair["dir"] == DOWN
                far = (pair["dir"] != EQUAL) & (pair["tmax"] >= t)
                tab[i, s, B * B:] = [len(on), len(pair), int((on["cls"] == ONLY_A).sum()), int((on["cls"] == ONLY_B).sum()), int(pair["va"].sum()), int(pair["ma"].sum()),
                                     int(pair["vb"].sum()), int(pair["mb"].sum()), int(up.sum()), int(down.sum()), int((up & far).sum()), int((down & far).sum())]
        out.append(tab)
    return out


def records(join, t, select):
    """RECORD[]: the shifted paired sites at t permille whose direction is in ``select`` (a selection of "up", "down"), in output order."""
    want = (join["cls"] == PAIRED) & (join["dir"] != EQUAL) & (join["tmax"] >= t) & (((join["dir"] == UP) & ("up" in select)) | ((join["dir"] == DOWN) & ("down" in select)))
    j = join[want]
    rec = np.zeros(len(j), dtype=RECORD)
    for f in ("candidate", "contig", "pos"):
        rec[f] = j[f]
    rec["code"] = j["strand"] * MINUS_BIT + (j["dir"] == DOWN) * DOWN_BIT
    rec["n_valid_a"], rec["n_mod_a"], rec["n_valid_b"], rec["n_mod_b"] = j["va"], j["ma"], j["vb"], j["mb"]
    return rec


@functools.lru_cache(maxsize=None)
def geometry():
    """(names, seqs, records of A, records of B, candidates, JOIN[] of every occurrence): computed once, shared with the GPU suite."""
    names, seqs, rec_a = H.meth_input()
    rec_b = sample_b()
    cands = P.candidates()
    join = join_records(names, seqs, rec_a, rec_b, F.BINS_OF, cands)
    join.setflags(write=False)
    return names, seqs, rec_a, rec_b, cands, join


# ------------------------------------------------------------------------------------------------ large coverages
BIG = (1 << 31) - 1
_VB = BIG - 2                                              # coprime to the prime 2^31 - 1
_MA = (-pow(_VB, -1, BIG)) % BIG                           # mB vA - mA vB = 1: the fractions differ by 2^-62
LARGE_SITES = [  # (vA, mA, vB, mB) of the '+' A of consecutive GATC of the contig `huge`
    (4, 1, 4, 3),                                          # the small threshold equality, beside the large ones
    (BIG, _MA, _VB, (_MA * _VB + 1) // BIG),               # up by one part in 2^62: float64 sees two equal fractions
    (_VB, (_MA * _VB + 1) // BIG, BIG, _MA),               # ... and down
    (BIG, 0, BIG, BIG),                                    # 0 -> 1 at full coverage: |x - y| = vA vB near 2^62, 1000 |x - y| wraps
    (BIG, BIG, BIG, 0),
    (BIG - 647, 0, BIG - 647, (BIG - 647) // 4),           # 2 147 483 000: up by exactly 250 permille
    (BIG - 647, (BIG - 647) // 2 + 1, BIG - 647, 0),       # down by one count more than 500 permille
    (BIG - 647, (BIG - 647) // 2 - 1, BIG - 647, 0),       # ... and one count less
    (1 << 27, 1 << 26, (1 << 27) - 1, 5),                  # vA vB just below 2^54: the last of the 64-bit path
    (1 << 27, 5, 1 << 27, 1 << 26),                        # vA vB = 2^54: the first of the 128-bit path
    (BIG, 1 << 30, 3, 1),                                  # a large against a small coverage
    (6, 3, BIG - 1, (BIG - 1) // 2),                       # 3 / 6 against (2^30 - 1) / (2^31 - 2): equal
]
LARGE_NAME, LARGE_CAND = "huge", ("GATC", "a", 1, "bh")
LARGE_SEQ = "GATC" * len(LARGE_SITES) + "TT"


def large_input():
    """(names, seqs, records of A, records of B, bins_of, candidates) of the large-coverage input: '+' records on the A of every GATC."""
    pos = np.arange(len(LARGE_SITES), dtype=np.int64) * 4 + 1
    col = lambda j: np.array([s[j] for s in LARGE_SITES], dtype=np.int64)
    mk = lambda v, m: dict(position=pos, strand=np.full(len(pos), H.PLUS, np.uint8), n_valid=col(v), n_mod=col(m), n_diff=np.zeros(len(pos), np.int64))
    return [LARGE_NAME], {LARGE_NAME: LARGE_SEQ}, {(LARGE_NAME, "a"): mk(0, 1)}, {(LARGE_NAME, "a"): mk(2, 3)}, {"bh": [LARGE_NAME]}, [LARGE_CAND]
