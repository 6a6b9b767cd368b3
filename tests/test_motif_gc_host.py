"""Host side of ``nanomotif motif_gc`` (no GPU): the brute force both suites compare against, the geometry input it runs on and the
conditions that input must meet, a case small enough to check by hand, the rebinning, the statistics on hand-made tables, the four
writers byte for byte, the parser's refusals, the planted GC-noise input of the command test with its margins, and the export in the
header, the binding and the build.

``gc_expected`` is the definition and shares nothing with the engine: plain Python over dense per-position arrays.  Occurrences are
found by comparing the sequence letter by letter with the motif's IUPAC sets (the motif on '+', its reverse complement for '-'), the
state of a site is read from a per-(strand, position) array filled from the pileup rows (>= high: mod, which wins; <= low: nomod), and
the window is counted letter by letter."""
import functools
import math
import os

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192
HALVES = (0, 1, 15, 16, 31)
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
CANONICAL = {"a": "A", "m": "C"}


# ------------------------------------------------------------------------------------------------ the brute force
def motif_sets(text):
    """The motif as a list of letter sets, None for a position that takes any character: ``.`` and ``N``, ``[..]`` groups, IUPAC codes."""
    sets, j = [], 0
    while j < len(text):
        if text[j] == "[":
            e = text.index("]", j)
            sets.append(frozenset(text[j + 1:e]))
            j = e + 1
        else:
            sets.append(None if text[j] in ".N" else frozenset(IUPAC[text[j]]))
            j += 1
    return sets


def stripped(sets, i):
    """(sets, i) without the any-character positions at either end."""
    lo = 0
    while sets[lo] is None:
        lo += 1
    hi = len(sets)
    while sets[hi - 1] is None:
        hi -= 1
    return sets[lo:hi], i - lo


def site_list(seq, motif, i):
    """[(own position p, occurrence strand s)] of the motif with its modified base at index i."""
    sets, i = stripped(motif_sets(motif), i)
    n = len(sets)
    rc = [None if s is None else frozenset(COMPLEMENT[x] for x in s) for s in reversed(sets)]
    out = []
    for s, (ss, own) in enumerate(((sets, i), (rc, n - 1 - i))):
        fixed = [(j, x) for j, x in enumerate(ss) if x is not None]
        for start in range(len(seq) - n + 1):
            if all(seq[start + j] in x for j, x in fixed):
                out.append((start + own, s))
    return out


def state_arrays(length, rows, low=0.3, high=0.7):
    """[2 strands][length]: 0 mod, 1 nomod, 2 nocall from the rows (position, '+' / '-', fraction); a position called both ways is mod."""
    st = [[2] * length, [2] * length]
    for p, strand, f in rows:
        if f <= low and 0 <= p < length:
            st[0 if strand == "+" else 1][p] = 1
    for p, strand, f in rows:
        if f >= high and 0 <= p < length:
            st[0 if strand == "+" else 1][p] = 0
    return st


def window_g(seq, p, half):
    """G + C among the 2 half + 1 letters centred on p, counted one by one; None when the window leaves the contig or holds another letter."""
    if p - half < 0 or p + half >= len(seq):
        return None
    g = 0
    for q in range(p - half, p + half + 1):
        ch = seq[q]
        if ch not in "ACGT":
            return None
        if ch in "GC":
            g += 1
    return g


@functools.lru_cache(maxsize=None)
def g_array(seq, half):
    return [window_g(seq, p, half) for p in range(len(seq))]


@functools.lru_cache(maxsize=None)
def _sites_cached(seq, motif, i):
    return site_list(seq, motif, i)


def gc_expected(contigs, piles, cands, half):
    """Per candidate (bin, mod type, motif, mod position) the int64[n_contigs, 2, 3, W + 2] of ``ScanEngine.motif_gc``.  ``contigs``: bin ->
    [(name, sequence)] in row order; ``piles``: (mod type, contig name) -> [(position, '+' / '-', fraction)]."""
    width = 2 * half + 1
    states = {}
    out = []
    for b, mt, motif, i in cands:
        t = np.zeros((len(contigs[b]), 2, 3, width + 2), dtype=np.int64)
        for c, (name, seq) in enumerate(contigs[b]):
            if (mt, name) not in states:
                states[(mt, name)] = state_arrays(len(seq), piles.get((mt, name), ()))
            st, gs = states[(mt, name)], g_array(seq, half)
            for p, s in _sites_cached(seq, motif, i):
                g = gs[p]
                t[c, s, st[s][p], width + 1 if g is None else g] += 1
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------ a case to check by hand
HAND_SEQ = "GGATCNTGATCCGATC"
HAND_ROWS = [(2, "+", 0.9), (8, "+", 0.1), (3, "-", 0.95), (9, "-", 0.2), (14, "-", 0.8)]
#            g = 0  1  2  3  4  5  edge                      GATC @ 1, half 2 (W = 5).  '+' sites (the A): 2, 8, 13; '-' sites (the T): 3, 9, 14
HAND = [[[0, 0, 0, 1, 0, 0, 0],                            # '+' mod: 2, window GGATC: 3
         [0, 0, 1, 0, 0, 0, 0],                            # '+' nomod: 8, window TGATC: 2
         [0, 0, 0, 1, 0, 0, 0]],                           # '+' nocall: 13, window CGATC: 3
        [[0, 0, 0, 0, 0, 0, 2],                            # '-' mod: 3, window GATCN holds an N; 14, window 12..16 leaves the contig of 16
         [0, 0, 0, 1, 0, 0, 0],                            # '-' nomod: 9, window GATCC: 3
         [0, 0, 0, 0, 0, 0, 0]]]


def test_a_case_checked_by_hand():
    assert sorted(site_list(HAND_SEQ, "GATC", 1)) == [(2, 0), (3, 1), (8, 0), (9, 1), (13, 0), (14, 1)]
    assert [window_g(HAND_SEQ, p, 2) for p in (2, 8, 13, 3, 9, 14)] == [3, 2, 3, None, 3, None]
    t = gc_expected({"b": [("c", HAND_SEQ)]}, {("a", "c"): HAND_ROWS}, [("b", "a", "GATC", 1)], 2)
    assert t[0].shape == (1, 2, 3, 7) and t[0][0].tolist() == HAND
    # half 0: g is the modified base itself read on '+': the A and the T of GATC are 0
    t0 = gc_expected({"b": [("c", HAND_SEQ)]}, {("a", "c"): HAND_ROWS}, [("b", "a", "GATC", 1)], 0)[0][0]
    assert t0[..., 0].tolist() == [[1, 1, 1], [2, 1, 0]] and not t0[..., 1:].any()
    assert site_list("AAGATCAA", "..GATC.", 3) == site_list("AAGATCAA", "GATC", 1) and site_list("CCTGG", "CCWGG", 1) == site_list("CCTGG", "CC[AT]GG", 1) == [(1, 0), (3, 1)]


# ------------------------------------------------------------------------------------------------ the geometry input (shared with the GPU suite)
GC_MOTIFS = [("GATC", 1, "a"), ("CC[AT]GG", 1, "m"), ("ACCT", 0, "a"), ("TGA", 2, "a"), ("A" + "." * 40 + "C", 0, "a"), ("A" + "." * 70 + "T", 0, "a"),
             ("T" + "." * 70 + "A", 71, "a"), ("A", 0, "a"), ("C", 0, "m")]
BIG = 2 * CHUNK + 200
N_SPACING = 160
N_CASES = [(h, 100 + (k * 4 + c) * N_SPACING, c) for k, h in enumerate(HALVES) for c in range(4) if h or c >= 2]   # (half, position of the A, case)


def _random_seq(rng, length, letters="ACGT", block=97):
    """Random letters whose G + C share changes every ``block`` positions, so that g takes many values."""
    out = []
    while len(out) < length:
        gc = rng.choice([0.15, 0.35, 0.5, 0.65, 0.85])
        p = {"A": (1 - gc) / 2, "T": (1 - gc) / 2, "C": gc / 2, "G": gc / 2}
        w = np.array([p[x] for x in letters])
        out += list(rng.choice(list(letters), size=block, p=w / w.sum()))
    return out[:length]


@functools.lru_cache(maxsize=None)
def gc_input():
    """(names in upload order, name -> sequence, name -> bin, bin names, mod type -> (contig id, position, strand, fraction) for
    ``upload_pileup``, (mod type, name) -> rows for the brute force)."""
    rng = np.random.default_rng(2207)
    seqs = {}
    first = _random_seq(rng, 900)
    first[:4] = "ACCT"                                                    # '+' site of ACCT @ 0 on position 0 of the upload
    first[-4:] = "AGGT"                                                   # its '-' site on the last position of the contig
    seqs["first"] = first
    big = _random_seq(rng, BIG)
    for at in (30, 126, CHUNK - 2, 2 * CHUNK - 2):                        # GATC: '+' site on bit 31 | '-' site on bit 0; 127 | 128; 8191 | 8192; 16383 | 16384
        big[at:at + 4] = "GATC"
    big[2 * CHUNK - 9:2 * CHUNK - 4] = "CCAGG"
    seqs["big"] = big
    seqs["gc1"] = _random_seq(rng, 300, "CG")                             # GC only, directly before AT only, directly before GC only
    seqs["at1"] = _random_seq(rng, 300, "AT")
    seqs["gc2"] = _random_seq(rng, 330, "CG")
    nrun = _random_seq(rng, 100 + len(N_CASES) * N_SPACING + 200)
    for h, q, case in N_CASES:                                            # an A whose window has an N first, last, one before, one behind
        nrun[q] = "A"
        nrun[(q - h, q + h, q - h - 1, q + h + 1)[case]] = "N"
    seqs["nrun"] = nrun
    tiny = _random_seq(rng, 40)
    tiny[18:22] = "GATC"
    seqs["tiny"] = tiny
    seqs["mid"] = _random_seq(rng, 777)
    seqs["tail"] = _random_seq(rng, 515)
    seqs = {n: "".join(s) for n, s in seqs.items()}
    names = ["first", "big", "gc1", "at1", "gc2", "nrun", "tiny", "mid", "tail"]
    bins = {"first": "b3", "big": "b1", "gc1": "b2", "at1": "b2", "gc2": "b2", "nrun": "b1", "tiny": "b1", "mid": "b2", "tail": "b3"}
    rows, piles = {}, {}
    for mt in ("a", "m"):
        cid, pos, strand, frac = [], [], [], []
        for c, n in enumerate(names):
            p, s = np.nonzero(rng.random((len(seqs[n]), 2)) < 0.6)
            f = rng.choice([0.0, 0.3, 0.5, 0.7, 1.0], size=len(p))
            piles[(mt, n)] = [(int(a), "+-"[int(b)], float(x)) for a, b, x in zip(p, s, f)]
            cid.append(np.full(len(p), c, np.uint32)); pos.append(p.astype(np.int64)); strand.append(np.where(s == 0, ord("+"), ord("-")).astype(np.uint8)); frac.append(f)
        rows[mt] = tuple(np.concatenate(x) for x in (cid, pos, strand, frac))
    return names, seqs, bins, ["b0_empty", "b1", "b2", "b3"], rows, piles


def gc_contigs():
    names, seqs, bins, bin_names, _, _ = gc_input()
    return {b: [(n, seqs[n]) for n in names if bins[n] == b] for b in bin_names}


def gc_cands():
    """[(bin, mod type, motif, mod position)]: every motif in every bin with a contig, bins and mod types interleaved."""
    return [(b, mt, m, i) for m, i, mt in GC_MOTIFS for b in ("b1", "b2", "b3")]


@functools.lru_cache(maxsize=None)
def gc_tables(half):
    return gc_expected(gc_contigs(), gc_input()[5], gc_cands(), half)


def test_the_input_is_not_degenerate():
    names, seqs, bins, bin_names, rows, piles = gc_input()
    assert names[0] == "first" and (0, 0) in site_list(seqs["first"], "ACCT", 0) and (len(seqs["first"]) - 1, 1) in site_list(seqs["first"], "ACCT", 0)
    assert len(seqs["big"]) == BIG and -(-BIG // CHUNK) == 3 and len(seqs["tiny"]) < 63
    gatc = set(site_list(seqs["big"], "GATC", 1))
    assert {(31, 0), (32, 1), (127, 0), (128, 1), (CHUNK - 1, 0), (CHUNK, 1), (2 * CHUNK - 1, 0), (2 * CHUNK, 1)} <= gatc
    assert (2 * CHUNK - 8, 0) in site_list(seqs["big"], "CC[AT]GG", 1)
    # widths: reach <= 31 (G = 1), <= 63 (G = 2), beyond (G = 3); mod position first, middle and last; a palindrome and others
    reach = sorted({max(i, len(motif_sets(m)) - 1 - i) for m, i, _ in GC_MOTIFS})
    assert reach[0] == 0 and any(31 < r <= 63 for r in reach) and any(r > 63 for r in reach)
    assert {("first" if i == 0 else "last" if i == len(motif_sets(m)) - 1 else "middle") for m, i, _ in GC_MOTIFS if len(motif_sets(m)) > 1} == {"first", "middle", "last"}
    cands = gc_cands()
    assert [c[0] for c in cands[:3]] == ["b1", "b2", "b3"] and {c[1] for c in cands} == {"a", "m"}
    big_sites = {(p, s) for m, i, _ in GC_MOTIFS[-2:] for p, s in site_list(seqs["big"], m, i)}
    a_sites = set(site_list(seqs["nrun"], "A", 0))
    for half in HALVES:
        width = 2 * half + 1
        tables = gc_tables(half)
        # the four positions at which a window starts and stops to fit, on a contig of three chunks: sites of a background candidate
        for p, edge in ((half - 1, True), (half, False), (BIG - 1 - half, False), (BIG - half, True)):
            if 0 <= p < BIG:
                assert {(p, 0), (p, 1)} & big_sites and (window_g(seqs["big"], p, half) is None) == edge, (half, p)
        # the window across the chunk border, with its site either side
        for p in (CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK):
            assert window_g(seqs["big"], p, half) is not None
        # an N first, last (edge), one before, one behind (not edge)
        for h, q, case in N_CASES:
            if h == half:
                assert (q, 0) in a_sites and (window_g(seqs["nrun"], q, half) is None) == (case < 2), (h, q, case)
        for k, (b, mt, m, i) in enumerate(cands):
            t = tables[k]
            assert t.shape == (len(gc_contigs()[b]), 2, 3, width + 2)
            if b == "b1" or len(m) == 1:
                assert t.sum() > 0, (half, b, m)
            if (b == "b1" and len(motif_sets(m)) < 72) or len(m) == 1:    # every state on both strands
                assert (t.sum(axis=(0, 3)) > 0).all() and t[..., :width + 1].sum() > 0, (half, b, m)
            if len(m) == 1 and half >= 15:                                # edge sites
                assert t[..., width + 1].sum() > 0, (half, b, m)
        # a window that reached into the neighbouring contig would change g: GC only | AT only | GC only
        k = cands.index(("b2", "m", "C", 0))
        order = [n for n, _ in gc_contigs()["b2"]]
        assert order[:3] == ["gc1", "at1", "gc2"]
        for name, only in (("gc1", width), ("gc2", width)):
            t = tables[k][order.index(name)]
            assert t[..., only].sum() > 0 and t.sum() == t[..., only].sum() + t[..., width + 1].sum() and t[..., width + 1].sum() == (2 * half if half else 0)
        t = tables[cands.index(("b2", "a", "A", 0))][order.index("at1")]
        assert t[..., 0].sum() > 0 and t.sum() == t[..., 0].sum() + t[..., width + 1].sum() == 300
        # a contig shorter than the window is all edge
        tiny = tables[cands.index(("b1", "a", "GATC", 1))][[n for n, _ in gc_contigs()["b1"]].index("tiny")]
        assert tiny.sum() == 2 and (tiny[..., width + 1].sum() == 2) == (half > 18)
    # half 0: g is the modified base itself: 0 for every 6mA site, 1 for every 5mC site
    for k, (b, mt, m, i) in enumerate(cands):
        t = gc_tables(0)[k]
        assert t[..., 2].sum() == 0 and t[..., 1 if mt == "a" else 0].sum() == 0
    # g takes many values at the widest window
    assert (gc_tables(31)[cands.index(("b1", "a", "A", 0))].sum(axis=(0, 1, 2))[:64] > 0).sum() > 40


# ------------------------------------------------------------------------------------------------ rebinning
@pytest.mark.parametrize("bins", [1, 2, 8, 64])
@pytest.mark.parametrize("width", [1, 3, 63])
def test_every_g_lands_in_exactly_one_bucket(bins, width):
    """bucket = min(B - 1, g * B // (W + 1)) with B = min(bins, W + 1): g takes W + 1 values, so more buckets than that cannot be in use
    (with --gc_bins above W + 1 the formula on ``bins`` itself would leave g = W short of the last bucket: W = 1, bins = 8 gives 4)."""
    from nanomotif_amd.motif_gc import bucket_bounds, bucket_of, effective_bins, rebin
    b = effective_bins(bins, width)
    assert b == min(bins, width + 1)
    got = [bucket_of(g, width, bins) for g in range(width + 1)]
    assert got == [min(b - 1, g * b // (width + 1)) for g in range(width + 1)]
    assert got == sorted(got) and got[0] == 0 and got[-1] == b - 1 and set(got) == set(range(b))
    bounds = bucket_bounds(width, bins)
    assert len(bounds) == b and bounds[0][0] == 0 and bounds[-1][1] == width
    assert all(bounds[k][1] + 1 == bounds[k + 1][0] for k in range(b - 1))
    per_g = np.arange(1, width + 2, dtype=np.int64) * 3
    out = rebin(np.stack([per_g, per_g * 2]), bins)
    assert out.shape == (2, b) and out[0].sum() == per_g.sum() and out[0].tolist() == [int(per_g[lo:hi + 1].sum()) for lo, hi in bounds] and (out[1] == 2 * out[0]).all()


# ------------------------------------------------------------------------------------------------ statistics on hand-made tables
def _per_g(width, cells):
    a = np.zeros(width + 1, dtype=np.int64)
    for g, n in cells.items():
        a[g] = n
    return a


def test_trend_z_on_a_table_worked_by_hand():
    """g = 0, 1, 2 with 10 sites each, 2 / 5 / 8 methylated: N = 30, p = 1/2, gbar = 1, T = -2 + 8 = 6, Var = 1/4 * 20 = 5, z = 6 / sqrt 5."""
    from nanomotif_amd.motif_gc import trend_p, trend_terms, trend_z
    mod, n = [2, 5, 8], [10, 10, 10]
    assert trend_terms(mod, n) == (6.0, 5.0)
    z = trend_z(mod, n)
    assert abs(z - 6 / math.sqrt(5)) < 1e-12 and abs(trend_p(z) - math.erfc(z / math.sqrt(2))) < 1e-15 and trend_p(-z) == trend_p(z)
    assert trend_z(mod[::-1], n) == -z
    assert trend_z([3, 3, 3], n) == 0.0                                   # no trend
    assert trend_z([0, 0, 0], n) == 0.0 and trend_z([10, 10, 10], n) == 0.0 and trend_z([0, 4, 0], [0, 9, 0]) == 0.0 and trend_z([], []) == 0.0
    assert trend_p(0.0) == 1.0


def test_trend_within_contigs_and_the_simpson_case():
    """Two contigs of another GC and another methylation level, no trend inside either: the pooled z is far above --min_z, the within-contig
    one is 0, and the flag stays ``none``."""
    from nanomotif_amd.motif_gc import summary_row, trend_z, trend_z_within
    width = 63
    low = (_per_g(width, {10: 10, 12: 10}), _per_g(width, {10: 100, 12: 100}))       # 10 % methylated at g = 10 and 12
    high = (_per_g(width, {40: 90, 42: 90}), _per_g(width, {40: 100, 42: 100}))      # 90 % at g = 40 and 42
    mod_cg, n_cg = np.stack([low[0], high[0]]), np.stack([low[1], high[1]])
    pooled_z = trend_z(mod_cg.sum(axis=0), n_cg.sum(axis=0))
    assert pooled_z > 15 and trend_z_within(mod_cg, n_cg) == 0.0
    # the same through a row: [n_contigs, 2 strands, 3 states, W + 2]
    table = np.zeros((2, 2, 3, width + 2), dtype=np.int64)
    table[:, 0, 0, :width + 1] = mod_cg
    table[:, 1, 1, :width + 1] = n_cg - mod_cg
    row = summary_row(["b", "CG", "m", 0], table, None)
    assert row[4:6] == [400, "0.500000"] and float(row[8]) > 15 and row[10] == "0.000" and row[11:14] == ["0.100000", "0.900000", "0.800000"] and row[-1] == "none"
    # a real trend inside each contig is summed: each contig has T = 6, Var = 5 (the table above)
    three = (np.array([[2, 5, 8], [2, 5, 8]]), np.array([[10, 10, 10], [10, 10, 10]]))
    assert abs(trend_z_within(*three) - 12 / math.sqrt(10)) < 1e-12
    # a contig with one outcome only takes no part
    assert abs(trend_z_within(np.array([[2, 5, 8], [0, 0, 0], [7, 7, 7]]), np.array([[10, 10, 10], [5, 5, 5], [7, 7, 7]])) - 6 / math.sqrt(5)) < 1e-12


def test_thirds_and_their_ties():
    from nanomotif_amd.motif_gc import thirds
    # 30 sites on six values: the low third is g = 0, 1 (10 sites), the high third g = 4, 5
    assert thirds([0, 1, 2, 3, 4, 5], [5, 5, 5, 5, 5, 5]) == ((1, 10), (9, 10))
    # whole values of g are taken: 4 + 7 >= 30 / 3 needs the second value, and 12 alone is a third from above
    assert thirds([1, 2, 0, 6], [4, 7, 7, 12]) == ((3, 11), (6, 12))
    # the two groups share g = 1: empty
    assert thirds([1, 9, 1], [2, 26, 2]) is None
    assert thirds([3], [9]) is None and thirds([0, 0], [0, 0]) is None
    # two values: each is its own group
    assert thirds([1, 0, 0, 8], [10, 0, 0, 10]) == ((1, 10), (8, 10))


def test_bg_expected_skips_empty_background_buckets():
    from nanomotif_amd.motif_gc import bg_expected
    # the background has no called site at g = 1: the motif's 50 sites there take no part
    assert bg_expected([10, 50, 30], [1, 0, 6], [10, 0, 10]) == (10 * 0.1 + 30 * 0.6) / 40
    assert bg_expected([10, 50, 30], [0, 0, 0], [0, 0, 0]) is None and bg_expected([0, 0, 5], [5, 5, 0], [10, 10, 0]) is None


def _table(width, cells, n_contigs=1):
    """cells: {(contig, strand, state, g or 'edge'): n}"""
    t = np.zeros((n_contigs, 2, 3, width + 2), dtype=np.int64)
    for (c, s, st, g), n in cells.items():
        t[c, s, st, width + 1 if g == "edge" else g] = n
    return t


def test_each_flag():
    from nanomotif_amd.motif_gc import summary_row
    key = ["b", "CCGG", "m", 0]
    rising = _table(7, {(0, 0, 0, 1): 5, (0, 0, 1, 1): 95, (0, 1, 0, 4): 50, (0, 1, 1, 4): 50, (0, 0, 0, 6): 95, (0, 0, 1, 6): 5, (0, 0, 0, "edge"): 1000})
    row = summary_row(key, rising, None)
    assert row[4] == 300 and float(row[10]) > 5 and row[11:14] == ["0.050000", "0.950000", "0.900000"] and row[14:16] == ["", ""] and row[-1] == "gc_dependent"
    assert summary_row(key, rising, None, min_z=50.0)[-1] == "none" and summary_row(key, rising, None, min_delta=0.95)[-1] == "none"
    assert summary_row(key, rising, None, min_called=301)[-1] == "few_sites" and summary_row(key, rising, None, min_called=300)[-1] == "gc_dependent"
    falling = rising[:, :, [1, 0, 2]]                                     # mod and nomod exchanged: the flag is two-sided
    row = summary_row(key, falling, None)
    assert float(row[10]) < -5 and row[13] == "-0.900000" and row[-1] == "gc_dependent"
    flat = _table(7, dict([((0, 0, 0, g), 90) for g in (1, 4, 7)] + [((0, 0, 1, g), 10) for g in (1, 4, 7)]))
    row = summary_row(key, flat, None)
    assert row[8] == "0.000" and row[13] == "0.000000" and row[-1] == "none"
    # all called sites on one g: no thirds, no trend, no flag; edge sites are not called sites
    one = _table(7, {(0, 0, 0, 3): 30, (0, 1, 1, 3): 30, (0, 0, 0, "edge"): 500})
    row = summary_row(key, one, None)
    assert row[4:6] == [60, "0.500000"] and row[11:14] == ["", "", ""] and row[-1] == "none"
    empty = summary_row(key, _table(7, {}), None)
    assert empty[4:8] == [0, "", "", ""] and empty[-1] == "few_sites"
    # against a background with the same curve the excess vanishes
    row = summary_row(key, rising, rising.sum(axis=(0, 1)))
    assert row[14] == "0.500000" and abs(float(row[15])) < 1e-6


# ------------------------------------------------------------------------------------------------ the writers, byte for byte
def test_the_four_files_byte_for_byte():
    from nanomotif_amd.motif_gc import format_files
    from nanomotif_amd.motif_sites import SiteCandidate
    width = 3                                                             # half 1; two buckets: g = 0, 1 | g = 2, 3
    cand = _table(width, {(0, 0, 0, 0): 1, (0, 0, 1, 0): 3, (0, 1, 0, 3): 6, (0, 1, 1, 2): 2, (0, 0, 2, 1): 4, (1, 0, 0, 3): 2, (1, 1, 1, "edge"): 5}, n_contigs=2)
    bg = _table(width, {(0, 0, 0, 1): 10, (0, 0, 1, 0): 30, (1, 1, 0, 2): 30, (1, 1, 1, 3): 10, (0, 0, 2, "edge"): 7, (1, 1, 0, "edge"): 2}, n_contigs=2)
    texts = format_files([SiteCandidate("b1", "GATC", "a", 1)], [(["c1", "c2"], cand)], [("b1", "a")], [(["c1", "c2"], bg)],
                         {"c1": "0.400000", "c2": "0.600000"}, {"b1": "0.480000"}, bins=2, min_called=5)
    assert texts[0] == ("bin\tmotif\tmod_type\tmod_position\tbucket\tgc_lower\tgc_upper\tn_mod\tn_nomod\tn_nocall\tfrac_mod\tbg_frac_mod\n"
                        "b1\tGATC\ta\t1\t0\t0.000000\t0.333333\t1\t3\t4\t0.250000\t0.250000\n"
                        "b1\tGATC\ta\t1\t1\t0.666667\t1.000000\t8\t2\t0\t0.800000\t0.750000\n")
    assert texts[1] == ("bin\tmotif\tmod_type\tmod_position\tbucket\tgc_lower\tgc_upper\tn_mod\tn_nomod\tn_nocall\tfrac_mod\tedge_mod\tedge_nomod\tedge_nocall\tbin_gc\n"
                        "b1\tA\ta\t0\t0\t0.000000\t0.333333\t10\t30\t0\t0.250000\t2\t0\t7\t0.480000\n"
                        "b1\tA\ta\t0\t1\t0.666667\t1.000000\t30\t10\t0\t0.750000\t2\t0\t7\t0.480000\n")
    assert texts[2] == ("bin\tmotif\tmod_type\tmod_position\tcontig\tcontig_gc\tfwd_mod\tfwd_nomod\tfwd_nocall\trev_mod\trev_nomod\trev_nocall\tmean_gc_mod\tmean_gc_nomod\tedge_sites\n"
                        "b1\tGATC\ta\t1\tc1\t0.400000\t1\t3\t4\t6\t2\t0\t0.857143\t0.266667\t0\n"
                        "b1\tGATC\ta\t1\tc2\t0.600000\t2\t0\t0\t0\t5\t0\t1.000000\t\t5\n")
    # called sites with a g: mod 9 (g = 0: 1, g = 3: 8), nomod 5 (g = 0: 3, g = 2: 2).  gbar = 28 / 14 = 2, T = 1 (-2) + 8 (1) = 6,
    # Var = 9/14 * 5/14 * (4 * 4 + 2 * 0 + 8 * 1) = 45 / 196 * 24, z = 6 / sqrt(1080 / 196) = 2.556; within: contig c2 has one outcome, so
    # c1 alone: n = 4, 2, 6 at g = 0, 2, 3, mod 1, 0, 6: gbar = 22 / 12, T = 1 (-11/6) + 6 (7/6) = 31/6, Var = 7/12 * 5/12 * (4 * 121 + 2 + 6 * 49) / 36
    z = 6 / math.sqrt(1080 / 196)
    zw = (31 / 6) / math.sqrt(35 / 144 * 780 / 36)
    # thirds of 14 sites: ascending g = 0 (4 sites, 12 < 14), g = 2 (6 sites): mod 1 of 6; descending g = 3 (8 sites): mod 8 of 8
    # background per g: 0 / 30, 10 / 10, 30 / 30, 0 / 10: expected = (4 * 0 + 2 * 1 + 8 * 0) / 14
    assert texts[3] == ("bin\tmotif\tmod_type\tmod_position\tn_called\tfrac_mod\tmean_gc_mod\tmean_gc_nomod\ttrend_z\ttrend_p\ttrend_z_within\tfrac_mod_low_gc\t"
                        "frac_mod_high_gc\tdelta\tbg_expected\texcess\tflag\n"
                        f"b1\tGATC\ta\t1\t14\t0.642857\t0.888889\t0.266667\t{z:.3f}\t{math.erfc(z / math.sqrt(2)):.3e}\t{zw:.3f}\t0.166667\t1.000000\t0.833333\t"
                        "0.142857\t0.500000\tnone\n")
    assert f"{z:.3f}" == "2.556" and f"{zw:.3f}" == "2.251"
    # a candidate whose bin has no background row still gets its rows
    alone = format_files([SiteCandidate("b1", "GATC", "a", 1)], [(["c1", "c2"], cand)], [], [], {}, {}, bins=2)
    assert alone[0].split("\n")[1].endswith("\t0.250000\t") and alone[1].count("\n") == 1 and alone[3].split("\n")[1].split("\t")[14:16] == ["", ""]


# ------------------------------------------------------------------------------------------------ the parser, the engine's checks, the exports
def test_parser_accepts_motif_gc_and_refuses_bad_values(capsys):
    p = create_parser()
    a = p.parse_args(["motif_gc", "asm.fasta", "p.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "gc"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.out, a.bin_motifs) == ("motif_gc", "asm.fasta", "p.bed", "contig_bin.tsv", "gc", ["out/bin-motifs.tsv"])
    assert (a.half, a.gc_bins, a.min_called, a.min_z, a.min_delta, a.device) == (31, 8, 20, 5.0, 0.2, None)
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage) == (0.3, 0.7, 5)
    a = p.parse_args(["motif_gc", "asm.fasta", "p.bed.gz", "-d", "bins", "--bin_motifs", "a.tsv", "b.tsv", "--half", "0", "--gc_bins", "64", "--min_called", "5", "--min_z", "3.5",
                      "--min_delta", "0.1", "--device", "2"])
    assert (a.directory, a.bin_motifs, a.half, a.gc_bins, a.min_called, a.min_z, a.min_delta, a.device) == ("bins", ["a.tsv", "b.tsv"], 0, 64, 5, 3.5, 0.1, 2)
    for flag, bad in (("--half", "32"), ("--half", "-1"), ("--half", "x"), ("--gc_bins", "0"), ("--gc_bins", "-3"), ("--gc_bins", "1.5")):
        with pytest.raises(SystemExit):
            p.parse_args(["motif_gc", "asm.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "b.tsv", flag, bad])
        assert flag in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["motif_gc", "asm.fasta", "p.bed", "-c", "cb.tsv"])                                  # --bin_motifs is required
    capsys.readouterr()
    assert "motif_gc" in p.format_help()


def test_engine_refuses_a_half_outside_the_range_before_it_needs_a_device():
    from nanomotif_amd.engine import GC_MAX_HALF, ScanEngine
    assert GC_MAX_HALF == 31
    eng = ScanEngine.__new__(ScanEngine)                                  # no context: the check comes first
    for bad in (-1, 32, 100):
        with pytest.raises(ValueError):
            ScanEngine.motif_gc(eng, [], half=bad)
    with pytest.raises(ValueError):
        ScanEngine.motif_gc(eng, [], half=31, max_bytes=0)


def test_export_is_declared_bound_and_built():
    import re
    from nanomotif_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    assert "int nm_motif_gc_count(" in header and "nm_motif_gc_count" in _lib.SYMBOLS
    assert re.search(r"#define\s+NM_GC_MAX_HALF\s+31\b", header)
    assert any(os.path.basename(s) == "nmgc.hip" for s in build.SRC_HIP)
    lib = _lib.load()
    # NULLs and a half above the limit are refused before the context is looked at
    assert lib.nm_motif_gc_count(None, 1, None, None, None, None, None, None, 31, None, None) == -1 and b"NULL" in lib.nm_last_error()
    rows = np.zeros(2, dtype=np.uint64)
    one32, one8, out = np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(6 * 67, np.int64)
    import ctypes as C
    args = [one32.ctypes.data_as(C.POINTER(C.c_uint32)), one8.ctypes.data_as(C.POINTER(C.c_uint8)), one8.ctypes.data_as(C.POINTER(C.c_uint8)),
            one8.ctypes.data_as(C.POINTER(C.c_uint8)), one32.ctypes.data_as(C.POINTER(C.c_uint32)), one8.ctypes.data_as(C.POINTER(C.c_uint8))]
    tail = [rows.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_int64))]
    assert lib.nm_motif_gc_count(None, 1, *args, 32, *tail) == -1 and b"NM_GC_MAX_HALF" in lib.nm_last_error()
    assert lib.nm_motif_gc_count(None, 1, *args, 31, *tail) == -1 and b"ctx" in lib.nm_last_error()


# ------------------------------------------------------------------------------------------------ the planted input of the command test
NOISE_BIN, CLEAN_BIN = "bin_noise", "bin_clean"
PLANTED_HALF = 31
NOISE_MOTIF = (NOISE_BIN, "GCGC", "m", 1)                                 # generic, short, GC-rich: listed for the bin whose C calls follow the local GC
TRUE_MOTIF = (NOISE_BIN, "GATC", "a", 1)                                  # methylated everywhere
PLANTED_CANDS = [NOISE_MOTIF, TRUE_MOTIF, (CLEAN_BIN, "GATC", "a", 1), (CLEAN_BIN, "CCWGG", "m", 1), (NOISE_BIN, "GATC", "21839", 1)]


def planted_metagenome():
    """Two bins of two contigs each whose G + C share changes every few hundred bp.  GATC (6mA) and CCWGG (5mC) are planted and methylated
    everywhere, as ``synth`` does it; in ``bin_noise`` the 5mC rows are replaced: every C (either strand) is called methylated with a
    probability that rises with the G + C among the 63 letters around it, whatever motif it lies in."""
    from nanomotif_amd import synth
    rng = np.random.default_rng(4111)
    names = ["n1", "c1", "n2", "c2"]
    bins = [NOISE_BIN, CLEAN_BIN, NOISE_BIN, CLEAN_BIN]
    seqs = ["".join(_random_seq(rng, length, block=311)) for length in (40_000, 20_000, 33_333, 17_001)]
    mg = synth.from_sequences(names, seqs, bins, [("GATC", 1, "a"), ("CCWGG", 1, "m")], seed=23, mod_types=("a", "m"))

    class GcNoise(type(mg)):
        def contig_pileup(self, i, mod_type):
            p = super().contig_pileup(i, mod_type)
            if mod_type != "m" or self.bin_names[i] != NOISE_BIN:
                return p
            seq = self.contig_str(i)
            gc = np.cumsum([0] + [ch in "GC" for ch in seq])
            pos = p["position"]
            inside = (pos >= 31) & (pos + 31 < len(seq))
            g = np.where(inside, gc[np.minimum(pos + 32, len(seq))] - gc[np.maximum(pos - 31, 0)], 0)
            prob = np.clip((g - 32) / 24.0, 0.0, 1.0)
            u = np.random.default_rng(977 + i).random(len(pos))
            return dict(p, pct_hundredths=np.where(u < prob, 9500, 200).astype(np.int32))
    mg.__class__ = GcNoise
    return mg


def piles_of(mg):
    """(mod types with rows in slot order, (mod type, contig) -> rows of the brute force) after the pre-filters of motif_discovery."""
    from nanomotif_amd.pileup import MOD_TYPES
    from test_gpu_motif_compare import _filtered_piles
    filtered = _filtered_piles(mg)
    targets = [mt for mt in MOD_TYPES if filtered[mt]]
    piles = {(mt, name): [(int(p), chr(int(s)), float(f)) for p, s, f in zip(cp.position, cp.strand, cp.fraction_mod)]
             for mt in targets for name, cp in filtered[mt].items()}
    return targets, piles


def gc_share(seqs) -> str:
    gc = sum(s.count("G") + s.count("C") for s in seqs)
    acgt = gc + sum(s.count("A") + s.count("T") for s in seqs)
    return "%.6f" % (gc / acgt) if acgt else ""


def expected_files(mg, cands, half, bins=8, min_called=20, min_z=5.0, min_delta=0.2):
    """The four files as lists of rows: the brute force over the pre-filtered pileup, through the module's own formatter."""
    from nanomotif_amd.motif_gc import format_files
    from nanomotif_amd.motif_sites import SiteCandidate
    targets, piles = piles_of(mg)
    bin_names = sorted(set(mg.bin_names))
    contigs = {b: [(n, mg.contig_str(i)) for i, n in enumerate(mg.names) if mg.bin_names[i] == b] for b in bin_names}
    known = [c for c in cands if c[2] in targets]
    bg_keys = [(b, mt) for b in bin_names for mt in targets]
    tables = gc_expected(contigs, piles, [(b, mt, m, p) for b, m, mt, p in known] + [(b, mt, CANONICAL[mt], 0) for b, mt in bg_keys], half)
    results = [([n for n, _ in contigs[c[0]]], t) for c, t in zip(known, tables)]
    bg_results = [([n for n, _ in contigs[b]], t) for (b, _), t in zip(bg_keys, tables[len(known):])]
    contig_gc = {n: gc_share([s]) for b in bin_names for n, s in contigs[b]}
    bin_gc = {b: gc_share([s for _, s in contigs[b]]) for b in bin_names}
    texts = format_files([SiteCandidate(*c) for c in known], results, bg_keys, bg_results, contig_gc, bin_gc, bins, min_called, min_z, min_delta)
    return [[line.split("\t") for line in t.split("\n")[:-1]] for t in texts], targets


@functools.lru_cache(maxsize=None)
def planted_expected():
    return expected_files(planted_metagenome(), PLANTED_CANDS, PLANTED_HALF)


def test_the_planted_input_yields_its_flags_with_twice_the_margin():
    """On the brute force alone: the noise motif is ``gc_dependent`` with |trend_z_within| and |delta| at least twice --min_z 5 and
    --min_delta 0.2, the true motif beside it is ``none`` although its bin's 5mC background rises steeply."""
    (f_main, f_bins, f_contigs, f_summary), targets = planted_expected()
    assert targets == ["m", "a"] or sorted(targets) == ["a", "m"]
    by_key = {tuple(r[:4]): dict(zip(f_summary[0], r)) for r in f_summary[1:]}
    assert len(by_key) == 4                                               # the 21839 row is skipped: the pileup holds no such rows
    noise = by_key[(NOISE_BIN, "GCGC", "m", "1")]
    print(noise)
    assert noise["flag"] == "gc_dependent" and abs(float(noise["trend_z_within"])) >= 10.0 and abs(float(noise["delta"])) >= 0.4 and int(noise["n_called"]) > 500
    assert abs(float(noise["excess"])) < 0.1                              # the bin's own background explains it
    true = by_key[(NOISE_BIN, "GATC", "a", "1")]
    print(true)
    assert true["flag"] == "none" and float(true["frac_mod"]) > 0.9 and abs(float(true["delta"])) < 0.1 and float(true["excess"]) > 0.8
    for key in ((CLEAN_BIN, "GATC", "a", "1"), (CLEAN_BIN, "CCWGG", "m", "1")):
        assert by_key[key]["flag"] == "none" and float(by_key[key]["frac_mod"]) > 0.9, by_key[key]
    # the noise curve itself: the background of the noisy bin rises over the buckets, the clean bin's stays flat
    curve = {b: [float(r[10]) for r in f_bins[1:] if r[0] == b and r[2] == "m" and r[10]] for b in (NOISE_BIN, CLEAN_BIN)}
    assert curve[NOISE_BIN][-1] - curve[NOISE_BIN][0] > 0.8 and max(curve[CLEAN_BIN]) < 0.1
    assert len(f_main) - 1 == 4 * 8 and len(f_bins) - 1 == 2 * 2 * 8 and len(f_contigs) - 1 == 4 * 2
