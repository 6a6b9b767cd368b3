"""Reference, wave split and geometry input for the pileup ingest of csrc/nmingest.hip (nm_ingest_pileup).

Three pieces for tests, none of which looks at the product's code path:

* ``expected`` runs ``oracle.pileup.prefilter`` (pinned to the reference's own outputs by fixtures g10 / g14) on a raw table and, on top of it,
  states letter by letter what every position of every contig holds per scored code and strand: ``mod`` (a kept row with fraction >= 0.7),
  ``nomod`` (a kept row with fraction <= 0.3), ``nocall`` (everything else).
* ``wave_split`` / ``wave_ranges`` restate how the ingest kernels cut a call's rows among their waves (``wave_row_range``): a call of at most
  2 097 152 rows gives every wave exactly 64 rows, so the loops of a kernel make more than one trip only with NM_INGEST_WALK_BLOCKS.
* ``build_input`` makes ONE table of ``N_ROWS`` rows, row by row in modkit's order, so that the index of every row is known when it is placed:
  contig, piece, turn and wave borders, key-cache traffic, plane words on the edges of the 32-word window of the store path, candidate runs that
  fill the dense path's queue — for the three grids ``GRIDS`` (NM_INGEST_WALK_BLOCKS unset, 1, 3).  ``census`` counts what the table holds, per
  grid, by replaying the bookkeeping of a wave (rows per piece and turn, a four-entry LRU, the window base, the queue depth) — a test asserts the
  counts, so the input cannot lose a border without a failure.  ``variants`` are single edits of the table that break modkit's order.

Plain Python and numpy, no GPU, not a conftest.
"""
from __future__ import annotations

import functools
from collections import Counter, defaultdict

import numpy as np

from oracle import pileup as op

SCORED = {0: ("m", "C"), 1: ("a", "A"), 2: ("21839", "C")}        # mod code -> (label, canonical base); codes 3, 4, 9 take part in the filters only
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
ABSENT = 0xFFFFFFFF                                                  # engine contig id of a contig the engine does not hold
N_ROWS = 60_000
GRIDS = (None, 1, 3)                                                 # NM_INGEST_WALK_BLOCKS
THR, LOW, HIGH = 0.7, 0.3, 0.7
PLUS, MINUS = ord("+"), ord("-")
WIN = 32                                                             # plane words in a wave's window of the store path
CHUNK_BP = 8192                                                      # contigs begin on a multiple of it in the planes
PREFIXES = (1, 63, 64, 65, 255, 256, 257)                            # calls of so many rows: nothing survives the frequency filter
VARIANT_OFFSETS = (0, 64, 256, 300)                                  # a wave's first row, the second piece, the second dense turn, mid-piece


# ----------------------------------------------------------------------------------------------------
# (a) the wave split
# ----------------------------------------------------------------------------------------------------
def round_up_64(x):
    return (x + 63) // 64 * 64


def walk_blocks(n, k=None):
    blocks = max(1, min((n + 255) // 256, 8192))
    return min(blocks, k) if k else blocks


def wave_split(n, k=None):
    """(waves, rows per wave) of a call of n rows (entries of the candidate list alike) under NM_INGEST_WALK_BLOCKS=k"""
    waves = 4 * walk_blocks(n, k)
    return waves, round_up_64(-(-n // waves))


def wave_ranges(n, k=None):
    waves, per = wave_split(n, k)
    return [(w * per, min(n, (w + 1) * per)) for w in range(waves) if w * per < n]


# ----------------------------------------------------------------------------------------------------
# (b) the reference
# ----------------------------------------------------------------------------------------------------
class Fates:
    """per row of a table: past the coverage filter, past the frequency filter, kept by all three (oracle.pileup)"""

    def __init__(self, table):
        n = len(table["position"])
        t = dict(table, row=np.arange(n))
        cov = op.filter_pileup(t)
        freq = op.filter_pileup_minimummod_frequency(cov)
        kept = op.filter_pileup_adjacency_filter(freq)
        self.cov, self.freq, self.kept = (np.zeros(n, dtype=bool) for _ in range(3))
        self.cov[cov["row"]] = True
        self.freq[freq["row"]] = True
        self.kept[kept["row"]] = True


class Expected:
    pass


def expected(geo, table):
    """What an engine holding ``geo``'s resident contigs must report for ``table``: n_kept, kept[contig][code < 8], the confident rows as a sorted
    list of (contig, position, strand, code), and per scored code the sorted (contig, position, site code) of every occurrence of its one-letter
    motif — site code = 4 for the '-' strand | 0 mod / 1 nomod / 2 nocall."""
    f = Fates(table)
    lut = geo.lut[table["contig"]]
    keep = f.kept & (lut != ABSENT)
    e = Expected()
    e.n_kept = int(keep.sum())
    e.kept = np.zeros((len(geo.seqs), 8), dtype=np.int64)
    sel = keep & (table["mod_type"] < 8)
    np.add.at(e.kept, (lut[sel], table["mod_type"][sel]), 1)
    frac = table["fraction_mod"]
    with np.errstate(invalid="ignore"):
        conf = keep & (frac >= HIGH) & np.isin(table["mod_type"], list(SCORED))
        state_of_row = np.where(frac >= HIGH, 0, np.where(frac <= LOW, 1, 2))
    e.confident = sorted(zip(lut[conf].tolist(), table["position"][conf].tolist(), table["strand"][conf].tolist(), table["mod_type"][conf].tolist()))
    with np.errstate(invalid="ignore"):
        e.n_candidates = int((f.freq & (lut != ABSENT) & (frac >= THR)).sum())                   # entries of the packed candidate list
        e.cap = int((f.cov & (lut != ABSENT) & (frac >= THR)).sum())                             # the counting pass's upper bound of them
    e.sites = {}
    for code, (_, base) in SCORED.items():
        state = {(c, s): [2] * len(seq) for c, seq in enumerate(geo.seqs) for s in (PLUS, MINUS)}
        for i in np.flatnonzero(keep & (table["mod_type"] == code)).tolist():
            state[(int(lut[i]), int(table["strand"][i]))][int(table["position"][i])] = int(state_of_row[i])
        rec = []
        for c, seq in enumerate(geo.seqs):                            # letter by letter
            plus, minus = state[(c, PLUS)], state[(c, MINUS)]
            for p, ch in enumerate(seq):
                if ch == base:
                    rec.append((c, p, plus[p]))
                elif ch == COMPLEMENT[base]:
                    rec.append((c, p, 4 | minus[p]))
        e.sites[code] = rec
    return e


# ----------------------------------------------------------------------------------------------------
# (c) the input
# ----------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self):
        self.rows, self.resident, self.cursor, self.marks = [], [], [], {}

    @property
    def n(self):
        return len(self.rows)

    def contig(self, resident=True):
        self.resident.append(resident)
        self.cursor.append(0)
        return len(self.cursor) - 1

    def here(self, c):
        return self.cursor[c]

    def skip(self, c, to):
        assert to >= self.cursor[c]
        self.cursor[c] = to

    def row(self, c, p, strand, code, frac, cov=20, plant=True):
        """the next row of the table: modkit's order is asserted (the newest contig, position not below the row before)"""
        assert c == len(self.cursor) - 1 and (not self.rows or self.rows[-1][0] != c or self.rows[-1][1] <= p), (c, p)
        self.rows.append((c, p, PLUS if strand == "+" else MINUS, code, frac, cov, plant))
        self.cursor[c] = max(self.cursor[c], p + 1)

    def pad(self, c, n, step=1, extras=(), flood=False, nocall=True):
        """n rows from the contig's cursor on: unmethylated 'm' rows, strands alternating, with a '21839' row on the same cytosine on two positions
        of eight and, with ``nocall``, a fraction of 0.5 on one of seven (``flood``: candidates — 'm' '+' rows tied at 0.9 — instead);
        ``extras`` = (code, fraction, coverage) rows spread evenly among them, each on a position of its own"""
        assert n >= 0
        start, end = self.n, self.n + n
        at = {start + int((j + 0.5) * n / len(extras)): x for j, x in enumerate(extras)}
        assert len(at) == len(extras)
        p = self.cursor[c]
        while self.n < end:
            strand = "+" if (p // step) % 2 == 0 else "-"
            if self.n in at:
                code, frac, cov = at[self.n]
                self.row(c, p, "-" if flood and code in SCORED else strand, code, frac, cov)
            elif flood:
                self.row(c, p, "+", 0, 0.9)
            else:
                self.row(c, p, strand, 0, 0.5 if nocall and p % 7 == 0 else (0.0, 0.1, 0.3)[p % 3])
                if p % 8 in (0, 3) and self.n < end and self.n not in at:
                    self.row(c, p, strand, 2, 0.5 if nocall and p % 5 == 0 else (0.2, 0.0, 0.3)[p % 3])
            p += step
        self.cursor[c] = p

    def align(self, c, target):
        self.pad(c, target - self.n)

    def cands(self, c, n, codes=(0,), frac=0.9, strand="+"):
        """n candidate rows per code on consecutive positions of one strand, tied: all survive"""
        for code in codes:
            for _ in range(n):
                self.row(c, self.cursor[c], strand, code, frac)

    def word_offset(self, c, offset, ahead=0):
        """the first position >= cursor + ahead that lies ``offset`` bits into a plane word"""
        p = self.cursor[c] + ahead
        return p + (offset - p) % 32


def _mixed(b, size, resident=True, every=5):
    """a contig of its own: ``size`` 'm' '+' rows on consecutive positions, every ``every``-th unmethylated, the others tied at 0.9"""
    c = b.contig(resident)
    for j in range(size):
        b.row(c, j, "+", 0, 0.1 if j % every == every - 1 else 0.9)
    return c


def _cluster(b):
    """feature A, from a wave's first row S = b.n on: contig borders at S (the contig before ends on S - 1), S + 64, S + 128, S + 256, in mid-piece
    (S + 356), two borders inside one piece around a contig that fails the frequency filter, a contig the engine does not hold between two it
    holds, and a contig of 65 rows"""
    s = b.n
    assert s % 64 == 0
    for size in (64, 64, 128, 100):
        _mixed(b, size)
    _mixed(b, 102)                       # ends 10 rows into a piece
    assert (b.n - s) % 64 == 10
    b.marks.setdefault("failing_middle", []).append(_mixed(b, 20))
    _mixed(b, 90)
    _mixed(b, 100, resident=False)
    _mixed(b, 80)
    b.marks.setdefault("contig_65", []).append(_mixed(b, 65, every=13))


def _nest(b, c, border):
    """around a wave border inside one plane word: two adjacency pairs that straddle it — '+' at distance 8 (the weaker row goes), '-' at distance 9
    (it stays), each with a stronger row of the other strand closer by — and between them unmethylated rows of both strands and two slots, four
    before the border and four behind it"""
    b.align(c, border - 6)
    p = b.word_offset(c, 8, ahead=9)
    b.row(c, p, "+", 0, 0.8)
    b.row(c, p + 1, "-", 0, 0.8)
    for q, strand in ((p + 2, "+"), (p + 3, "-"), (p + 4, "+"), (p + 5, "-")):
        if q == p + 4:
            assert b.n == border
        b.row(c, q, strand, 0, 0.1)
        b.row(c, q, strand, 2, 0.3)
    b.row(c, p + 8, "+", 0, 0.9)
    b.row(c, p + 10, "-", 0, 0.9)
    b.skip(c, p + 20)


def _share4(b, c, border):
    """a wave border inside one plane word, unmethylated rows of both strands and two slots either side"""
    b.align(c, border - 4)
    p = b.word_offset(c, 8)
    for q, strand in ((p, "+"), (p + 1, "-"), (p + 2, "+"), (p + 3, "-")):
        if q == p + 2:
            assert b.n == border
        b.row(c, q, strand, 0, 0.1)
        b.row(c, q, strand, 2, 0.2)


def _share1(b, c, border):
    """a wave border where the word before it holds 'm' rows of both strands and the rows behind it share only the '+' plane of that word"""
    b.align(c, border - 2)
    q = b.word_offset(c, 29)
    b.row(c, q, "+", 0, 0.1)
    b.row(c, q + 1, "-", 0, 0.1)
    assert b.n == border
    b.row(c, q + 2, "+", 0, 0.1)
    b.row(c, q + 4, "-", 0, 0.1)


def _window(b, c, d, inside):
    """feature C: after a stretch without rows a piece whose lane 0 opens the window on word B, and a row ``d`` words further on — in lane 0 of the
    next piece, or (``inside``) in the same piece"""
    b.align(c, round_up_64(b.n))
    base = b.word_offset(c, 0, ahead=40 * 32)
    near = 40 if inside else 64
    for j in range(near):
        b.row(c, base + j, "+" if j % 2 == 0 else "-", 0, 0.1)
    for j in range(64 if not inside else 24):
        b.row(c, base + d * 32 + j, "+" if j % 2 == 0 else "-", 0, 0.1)
    assert b.n % 64 == 0


def _pair(b, c, border, first, second, d):
    """two candidates ``d`` positions apart, the first on the last row before ``border``: (code, strand, fraction) each"""
    b.align(c, border - 1)
    p = b.here(c) + 9
    b.row(c, p, first[1], first[0], first[2])
    b.row(c, p + d, second[1], second[0], second[2])
    b.skip(c, p + d + 9)


def _interleave(x, y):
    out = []
    for j in range(max(len(x), len(y))):
        out += x[j:j + 1] + y[j:j + 1]
    return out


def _bound_extras(code, n_mod):
    """the rows that put a (contig, code) group on the strict bound of the frequency filter: n_mod rows above 0.7 with coverage above 5 (one of
    them with coverage 6), three rows at exactly 0.7 and two strong rows of coverage 5, which do not count"""
    return [(code, 0.9, 20)] * (n_mod - 1) + [(code, 0.9, 6)] + [(code, 0.7, 20)] * 3 + [(code, 0.9, 5)] * 2


class Geometry:
    pass


@functools.lru_cache(maxsize=None)
def build_input():
    b = _Builder()
    k1 = [s for s, _ in wave_ranges(N_ROWS, 1)]            # 0, 15040, 30080, 45120
    k3 = [s for s, _ in wave_ranges(N_ROWS, 3)]            # multiples of 5056
    nan = float("nan")

    # ---- the first 257 rows: nothing survives the frequency filter in any prefix of them; candidates below position 8, a row on position 0
    e1 = b.contig()
    b.row(e1, 0, "+", 0, 0.1)
    b.row(e1, 3, "+", 0, 0.9)
    b.row(e1, 7, "-", 0, 0.9)
    b.skip(e1, 8)
    b.pad(e1, 300 - b.n)
    b.cands(e1, 52, (0, 2))
    b.pad(e1, 30)
    p = b.here(e1) + 12
    b.row(e1, p, "+", 0, 0.9)                                # L - 9 and L - 1, tied at distance 8: both stay
    b.row(e1, p + 8, "+", 0, 0.9)
    e2 = b.contig()                                          # ... next to the first row of the next contig, on position 0
    b.cands(e2, 52)
    b.pad(e2, 40)

    # ---- feature B: six (contig, code) keys cycling; feature D: runs of 64 | 65, a rising run, a null and a strong row of coverage 5, pairs
    P = b.contig()
    b.cands(P, 52, (0, 1, 2, 3, 9))
    b.skip(P, b.here(P) + 9)
    b.cands(P, 3, (0, 1, 2), strand="-")
    start, turn = b.n, 0
    while b.n < start + 700:
        p = b.here(P)
        for code, frac in ((0, 0.1), (2, 0.2), (3, 0.5), (4, 0.5), (9, 0.5)):
            b.row(P, p, "+", code, frac)
        for code, frac in ((1, (0.1, 0.5, 0.3)[turn % 3]), (3, 0.4)):
            b.row(P, p + 1, "-", code, frac)
        for code, frac in ((1, (0.5, 0.0, 0.2)[turn % 3]), (4, 0.4)):
            b.row(P, p + 2, "+", code, frac)
        turn += 1
    b.align(P, round_up_64(b.n))
    for n_run in (64, 65):
        b.pad(P, 10)
        b.skip(P, b.here(P) + 9)
        b.cands(P, n_run)
        b.skip(P, b.here(P) + 9)
    b.pad(P, 10)
    p = b.here(P) + 9
    for j in range(40):                                      # strictly rising: only the last one is a maximum of its window
        b.row(P, p + j, "+", 0, 0.70 + 0.005 * j)
    p += 40 + 9
    b.row(P, p, "+", 0, 0.8)                                 # neither a null fraction nor a stronger row of coverage 5 suppresses it
    b.row(P, p + 2, "+", 0, nan)
    b.row(P, p + 4, "+", 0, 0.95, cov=5)
    b.skip(P, p + 14)
    border = round_up_64(b.n + 64)
    for first, second, d in (((0, "+", 0.8), (0, "+", 0.9), 8), ((0, "+", 0.8), (0, "+", 0.9), 9), ((0, "+", 0.8), (0, "-", 0.9), 8),
                             ((0, "+", 0.8), (3, "+", 0.9), 8), ((0, "+", 0.8), (3, "+", 0.9), 9), ((0, "+", 0.8), (9, "+", 0.9), 8),
                             ((0, "+", 0.9), (0, "+", 0.9), 8), ((2, "+", 0.8), (0, "+", 0.9), 8)):
        _pair(b, P, border, first, second, d)
        border += 64
    # a piece that holds a code >= 8 between pieces that do not
    b.align(P, round_up_64(b.n))
    b.pad(P, 64 + 30)
    b.row(P, b.here(P), "+", 9, 0.5)
    b.pad(P, 33 + 64)
    b.align(P, k3[1])
    b.skip(P, b.here(P) + 50)

    # ---- feature A at a wave border of k = 3
    _cluster(b)

    # ---- groups of 51 and 50 rows above 0.7 across a wave border of k = 3, with an adjacency nest on the border
    R = b.contig()
    b.cands(R, 52)
    extras = _interleave(_bound_extras(1, 51), _bound_extras(2, 50))
    half = len(extras) // 2
    b.pad(R, k3[2] - 6 - b.n, extras=extras[:half])
    _nest(b, R, k3[2])
    b.pad(R, 2400, extras=extras[half:])

    # ---- K: the contig that crosses two wave borders of k = 1
    K = b.contig()
    b.marks["K"] = K
    b.marks["K_first"] = b.n
    b.cands(K, 52, (0, 2))
    z0 = b.here(K)                                           # unmethylated rows on every second position: the free ones take a displaced row
    b.pad(K, 300, step=2)
    b.marks["zone"] = (z0, b.here(K))
    a_rows, x_rows = _bound_extras(1, 51), _bound_extras(3, 50)
    early, late = _interleave(a_rows[:17], x_rows[:17]), _interleave(a_rows[17:], x_rows[17:])
    b.pad(K, k1[1] - 6 - b.n, extras=early)
    _nest(b, K, k1[1])
    # feature D: 63 candidates wait at the end of the first dense turn of the wave (2 of the nest + 61), then every row is one
    b.pad(K, k1[1] + 256 - 61 - b.n)
    b.skip(K, b.here(K) + 9)
    b.marks["flood"] = b.n
    b.pad(K, 1100, flood=True)
    b.pad(K, k1[2] - 12 - b.n, extras=late, flood=True)
    b.skip(K, b.here(K) + 9)
    # ---- no candidate from here to the end of K: feature C and the rows the variants displace
    _share1(b, K, k1[2])
    b.pad(K, k3[6] + 400 - b.n, nocall=False)
    b.skip(K, b.here(K) + 5000)                              # a gap of several thousand bp
    for j in range(600):                                     # a row on every position and both strands; the letter suits one of the two
        p = b.here(K)
        b.row(K, p, "+", 0, 0.1, plant=j % 2 == 0)
        b.row(K, p, "-", 0, 0.2, plant=j % 2 == 1)
    b.skip(K, max(b.here(K), -(-b.here(K) // CHUNK_BP) * CHUNK_BP - 40))
    b.pad(K, 100)                                            # bits 8191 | 8192 of the planes
    assert b.here(K) % CHUNK_BP < 100
    for d in (15, 16, 17, 31, 32, 33):
        _window(b, K, d, inside=False)
        _window(b, K, d, inside=True)
    _share4(b, K, k3[7])
    _share1(b, K, k3[8])
    b.align(K, k1[3])                                        # K's last row, on L - 1, is the last row of a wave of k = 1

    # ---- feature A at a wave border of k = 1, then a last long contig
    _cluster(b)
    F = b.contig()
    b.cands(F, 52, (0, 2))
    b.pad(F, N_ROWS - b.n)
    b.skip(F, b.here(F) + 50)
    assert b.n == N_ROWS

    g = Geometry()
    cols = list(zip(*b.rows))
    g.table = dict(contig=np.array(cols[0], np.int64), position=np.array(cols[1], np.int64), strand=np.array(cols[2], np.uint8),
                   mod_type=np.array(cols[3], np.int8), fraction_mod=np.array(cols[4], np.float64), Nvalid_cov=np.array(cols[5], np.int64))
    g.marks = b.marks
    g.resident = np.array(b.resident)
    g.length = np.array(b.cursor, np.int64)
    g.lut = np.full(len(b.cursor), ABSENT, dtype=np.int64)
    g.lut[g.resident] = np.arange(int(g.resident.sum()))
    # the rows the position variants displace, each to a free position of the zone at least 40 plane words below the row before it
    z0, z1 = b.marks["zone"]
    free = iter(range(z0 + 1, z1, 2))
    g.variant_rows = sorted({s + o for s in (k1[2], k3[6]) for o in VARIANT_OFFSETS})         # (offset 256 of k = 1 is the first row of a wave of k = 3)
    g.displaced = {}
    letters = defaultdict(dict)
    for i in g.variant_rows:
        c, p, strand, code = b.rows[i][:4]
        assert c == K == b.rows[i - 1][0] and code in SCORED and b.rows[i][4] <= LOW and b.rows[i - 1][1] >= z1 + 40 * 32
        g.displaced[i] = next(free)
        letters[K][g.displaced[i]] = SCORED[code][1] if strand == PLUS else COMPLEMENT[SCORED[code][1]]
    # contigs: random filler, the right letter planted under every row of a scored code
    for c, p, strand, code, _, _, plant in b.rows:
        if code in SCORED and plant:
            ch = SCORED[code][1] if strand == PLUS else COMPLEMENT[SCORED[code][1]]
            assert letters[c].setdefault(p, ch) == ch, (c, p)
    rng = np.random.default_rng(20)
    g.seqs, g.names = [], []
    for c in range(len(b.cursor)):
        if not b.resident[c]:
            continue
        s = rng.choice(list("ACGT"), size=b.cursor[c])
        for p, ch in letters[c].items():
            s[p] = ch
        g.seqs.append("".join(s))
        g.names.append(f"contig_{c}")
    return g


# ----------------------------------------------------------------------------------------------------
# (d) variants: each one edit of the table that breaks modkit's order
# ----------------------------------------------------------------------------------------------------
def variant_names():
    g = build_input()
    return [f"{kind}@{i}" for kind in ("down", "runs") for i in g.variant_rows]


@functools.lru_cache(maxsize=None)
def variant(name):
    """``down@i``: the position of row i goes down, to a free position at least 40 plane words below row i - 1;
    ``runs@i``: K's rows before row i change places with the contig in front of K, so that K comes in two runs and the second begins on row i"""
    g = build_input()
    kind, i = name.split("@")
    i = int(i)
    t = {k: v.copy() for k, v in g.table.items()}
    if kind == "down":
        t["position"][i] = g.displaced[i]
        return t
    a = g.marks["K_first"]
    y = int(np.flatnonzero(t["contig"] == t["contig"][a - 1])[0])
    order = np.concatenate([np.arange(y), np.arange(a, i), np.arange(y, a), np.arange(i, len(t["contig"]))])
    return {k: v[order] for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def expected_of(name="base"):
    """``expected`` for the table itself or one of its variants, computed once"""
    g = build_input()
    return expected(g, g.table if name == "base" else variant(name))


# ----------------------------------------------------------------------------------------------------
# (e) census: what the table holds under one grid
# ----------------------------------------------------------------------------------------------------
def census(g, table, k):
    """Counts, for the waves of NM_INGEST_WALK_BLOCKS=k, of every border the input claims to hold."""
    n = len(table["position"])
    ranges = wave_ranges(n, k)
    contig, pos, strand, code = (table[x] for x in ("contig", "position", "strand", "mod_type"))
    frac, cov = table["fraction_mod"], table["Nvalid_cov"]
    f = Fates(table)
    res = g.lut[contig] != ABSENT
    null = np.isnan(frac)
    with np.errstate(invalid="ignore"):
        counted = res & (cov > 5)                                     # the counting pass: rows that belong to a frequency group
        pre = counted & ~null
        alive = pre & f.freq
        cand = alive & ~(frac < THR)
        non = alive & ~cand & np.isin(code, list(SCORED)) & (frac <= LOW)
        above = counted & (frac > THR)
    word = pos >> 5
    plane = code.astype(np.int64) * 2 + (strand == MINUS)
    out = Counter()
    change = np.flatnonzero(contig[1:] != contig[:-1]) + 1            # rows that begin a run
    wave_of = np.zeros(n, dtype=np.int64)
    for w, (a, e) in enumerate(ranges):
        wave_of[a:e] = w
    start_of = np.array([a for a, _ in ranges])[wave_of]

    # ---- A
    for r in change.tolist():
        off = r - int(start_of[r])
        if res[r] and res[r - 1]:
            out["border_at_offset_%d" % off if off in (0, 64, 128, 256) else "border_mid_piece" if off % 64 else "border_other_piece"] += 1
    runs = list(zip(np.concatenate([[0], change]).tolist(), np.concatenate([change, [n]]).tolist()))
    for j, (a, e) in enumerate(runs):
        inside = (a - int(start_of[a])) // 64 == (e - 1 - int(start_of[a])) // 64 and wave_of[a] == wave_of[e - 1]
        if inside and (a - int(start_of[a])) % 64 and (e - int(start_of[a])) % 64 and e - a < 51 and res[a] and not f.kept[a:e].any():
            out["failing_contig_inside_piece"] += 1
        if not res[a] and 0 < j < len(runs) - 1 and res[a - 1] and res[e]:
            out["absent_between_resident"] += 1
    for w, (a, e) in enumerate(ranges):
        has8 = [bool((pre[s:min(s + 64, e)] & (code[s:min(s + 64, e)] >= 8)).any()) for s in range(a, e, 64)]
        if len(has8) == 1:                                            # 64 rows a wave: the pieces either side are the neighbouring waves'
            prev_next = [bool((pre[s:s + 64] & (code[s:s + 64] >= 8)).any()) for s in (a - 64, a + 64) if 0 <= s < n]
            out["code8_piece_between"] += has8[0] and len(prev_next) == 2 and not any(prev_next)
        else:
            out["code8_piece_between"] += sum(1 for j in range(1, len(has8) - 1) if has8[j] and not has8[j - 1] and not has8[j + 1])

    # ---- B: the counting pass's key cache, a wave at a time
    for w, (a, e) in enumerate(ranges):
        lru, gone, returns, keys = [], set(), 0, set()
        for s in range(a, e, 64):
            seen = []
            for i in range(s, min(s + 64, e)):
                key = (int(contig[i]), int(code[i]))
                if counted[i] and key not in seen:
                    seen.append(key)
            for key in seen:
                keys.add(key)
                if key in lru:
                    lru.remove(key)
                else:
                    returns += key in gone
                    if len(lru) == 4:
                        gone.add(lru.pop())
                lru.insert(0, key)
        out["max_keys_in_a_wave"] = max(out["max_keys_in_a_wave"], len(keys))
        out["max_key_returns_in_a_wave"] = max(out["max_key_returns_in_a_wave"], returns)
    groups = defaultdict(list)
    for i in np.flatnonzero(above).tolist():
        groups[(int(contig[i]), int(code[i]))].append(i)
    for key, rows in groups.items():
        if len(rows) in (50, 51):
            members = counted & (contig == key[0]) & (code == key[1])
            spread = len({int(wave_of[i]) for i in rows}) > 1 and len({i // 256 for i in rows}) > 1
            out["group_of_%d_spread" % len(rows)] += spread
            out["group_of_%d_%s" % (len(rows), "kept" if f.kept[members].any() else "dropped")] += 1
            out["exactly_0.7_in_bound_group"] += int((members & (frac == THR)).sum())
            out["coverage_6_in_bound_group"] += int((members & (cov == 6)).sum())
            out["coverage_5_in_bound_group"] += int((res & (cov == 5) & (contig == key[0]) & (code == key[1])).sum())

    # ---- C: the window of the store path, a wave at a time (rows in modkit's order)
    for w, (a, e) in enumerate(ranges):
        have, base, cur, pieces = False, 0, None, 0
        for s in range(a, e, 64):
            todo = [(int(contig[i]), int(word[i])) for i in range(s, min(s + 64, e)) if non[i]]
            first = True
            pieces += bool(todo)                                      # pieces that put bits into the window as it stands
            while todo:
                lc, lw = todo[0]
                if not have or lc != cur:
                    out["window_contig_change"] += have
                    have, base, cur, pieces = True, lw, lc, 1
                else:
                    assert lw >= base
                    out["window_leader_%s_%d" % ("first" if first else "later", lw - base)] += 1
                    if lw >= base + WIN // 2:
                        out["window_max_pieces"] = max(out["window_max_pieces"], pieces)
                        base, pieces = lw, 1
                mine = [x for x in todo if x[0] == lc and base <= x[1] < base + WIN]
                for x in mine[1:]:
                    out["window_mine_%d" % (x[1] - base)] += 1
                todo = [x for x in todo if not (x[0] == lc and base <= x[1] < base + WIN)]
                first = False
    idx = np.flatnonzero(non)
    out["max_gap_bp"] = int((np.diff(pos) * (contig[1:] == contig[:-1]) * non[1:] * non[:-1]).max())      # between two rows that follow each other
    out["nomod_on_position_0"] = int((non & (pos == 0)).sum())
    out["nomod_on_last_position"] = int((non & (pos == g.length[contig] - 1)).sum())
    where = {(int(contig[i]), int(pos[i])) for i in idx.tolist()}
    out["nomod_on_bits_31_32"] = sum(1 for c, p in where if p % 32 == 31 and (c, p + 1) in where)
    out["nomod_on_bits_8191_8192"] = sum(1 for c, p in where if p % CHUNK_BP == CHUNK_BP - 1 and (c, p + 1) in where)
    by_site = defaultdict(set)
    for i in idx.tolist():
        by_site[(int(contig[i]), int(pos[i]), int(strand[i]))].add(int(code[i]))
    out["m_and_21839_on_one_cytosine"] = sum(1 for v in by_site.values() if {0, 2} <= v)
    for a, _ in ranges[1:]:
        key = (int(contig[a]), int(word[a]))
        before = {int(plane[i]) for i in range(max(0, a - 64), a) if non[i] and (int(contig[i]), int(word[i])) == key}
        behind = {int(plane[i]) for i in range(a, min(n, a + 64)) if non[i] and (int(contig[i]), int(word[i])) == key}
        shared = before & behind
        out["border_in_word_4_planes"] += len(shared) >= 4 and len({q & 1 for q in shared}) == 2 and len({q >> 1 for q in shared}) == 2
        out["border_in_word_1_plane_of_2"] += len(shared) == 1 and len(before) >= 2

    # ---- D
    per_wave = [int(cand[a:e].sum()) for a, e in ranges]
    out["max_candidates_in_a_wave"] = max(per_wave)
    out["empty_wave_between_busy_waves"] = sum(1 for j in range(1, len(per_wave) - 1)
                                               if per_wave[j] == 0 and max(per_wave[:j]) >= 32 and max(per_wave[j + 1:]) >= 32)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], cand.astype(np.int8), [0]])))
    for a, e in zip(edges[::2].tolist(), edges[1::2].tolist()):
        out["candidate_run_of_%d" % (e - a)] += 1
        if wave_of[a] == wave_of[e - 1]:
            out["max_candidate_run_in_a_wave"] = max(out["max_candidate_run_in_a_wave"], e - a)
    for a, e in ranges:                                               # the dense path's queue: 256 rows a turn, judged 64 at a time
        qn = 0
        for s in range(a, e, 256):
            qn += int(cand[s:min(s + 256, e)].sum())
            out["max_queue"] = max(out["max_queue"], qn)
            out["turns_with_63_waiting"] += qn >= 64 and qn % 64 == 63
            qn %= 64
    ci = np.flatnonzero(cand)
    for x, i in enumerate(ci.tolist()):                               # pairs of candidates within 9 positions of each other, in row order
        for j in ci[x + 1:x + 40].tolist():
            if contig[j] != contig[i] or pos[j] - pos[i] > 9:
                break
            d = int(pos[j] - pos[i])
            if frac[j] > frac[i]:
                kind = ("other_strand" if strand[i] != strand[j] else "other_code" if code[i] != code[j] else "same") + "_%d" % d
            elif frac[j] == frac[i] and strand[i] == strand[j]:
                kind = "tied_%d" % d
            else:
                continue
            if kind.startswith("other_strand") and d <= 8:
                kind, d = "other_strand_within_8", 8
            if d in (8, 9):
                if wave_of[i] != wave_of[j]:
                    out["pair_across_wave_" + kind] += 1
                if i // 64 != j // 64:
                    out["pair_across_piece_" + kind] += 1
    out["candidates_below_8"] = int((cand & (pos < 8)).sum())
    out["candidates_above_L_minus_9"] = int((cand & (pos > g.length[contig] - 9)).sum())
    out["last_position_next_to_position_0"] = sum(1 for r in change.tolist() if cand[r - 1] and cand[r] and pos[r] == 0
                                                  and pos[r - 1] == g.length[contig[r - 1]] - 1)
    for i in np.flatnonzero(res & (null | ((cov <= 5) & ~null))).tolist():
        near = [j for j in range(max(0, i - 8), min(n, i + 9)) if f.kept[j] and cand[j] and contig[j] == contig[i] and strand[j] == strand[i]
                and abs(int(pos[j]) - int(pos[i])) <= 8]
        if near and (null[i] or frac[i] > frac[near[0]]):
            out["null_next_to_kept_candidate" if null[i] else "stronger_coverage_5_next_to_kept_candidate"] += 1

    # ---- the oracle's result is not degenerate
    out["dropped_by_coverage"] = int((res & ~f.cov).sum())
    out["dropped_by_frequency"] = int((res & f.cov & ~f.freq).sum())
    out["dropped_by_adjacency"] = int((res & f.freq & ~f.kept).sum())
    with np.errstate(invalid="ignore"):
        for c in SCORED:
            for s, name in ((PLUS, "plus"), (MINUS, "minus")):
                sel = res & f.kept & (code == c) & (strand == s)
                out["mod_%d_%s" % (c, name)] = int((sel & (frac >= HIGH)).sum())
                out["nomod_%d_%s" % (c, name)] = int((sel & (frac <= LOW)).sum())
                out["nocall_%d_%s" % (c, name)] = int((sel & (frac > LOW) & (frac < HIGH)).sum())
    return out
