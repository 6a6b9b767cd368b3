"""The geometry input of the ``motif_regions`` tests and an independent brute force over it, in plain Python: per contig and class a
``set`` of positions built interval by interval, a regex scan for the occurrences on both strands, dense per-position state tables from
the pileup rows.  Nothing here is shared with ``nanomotif_amd/regions.py`` or the engine.

The input: five contigs of at most three chunks in upload order small (92 bp), one (8192), odd (8213), gap (700, no interval, between two
contigs that have some) and long (3 chunks, L % 32 != 0); bins b0_empty (no contig), b1 and b2; mod types a and m interleaved.  The
intervals (``INTERVALS``, given UNSORTED) are listed with what each is for."""
import functools
import re

import numpy as np

CHUNK = 8192
LONG = 2 * CHUNK + 300                      # 16 684: three chunks, L % 32 = 12
LENGTHS = {"small": 92, "one": CHUNK, "odd": CHUNK + 21, "gap": 700, "long": LONG}
NAMES = ["small", "one", "odd", "gap", "long"]
BINS = {"small": "b1", "one": "b1", "odd": "b2", "gap": "b2", "long": "b1"}
BIN_NAMES = ["b0_empty", "b1", "b2"]
MOTIFS = [("GATC", 1, "a"), ("CC[AT]GG", 1, "m"), ("A" + "." * 40 + "C", 0, "a"), ("A" + "." * 70 + "T", 0, "a")]      # G = 1, 1, 2, 3
BACKGROUNDS = [("A", 0, "a"), ("C", 0, "m")]
COMPLEMENT = str.maketrans("ACGT", "TGCA")
KINDS = ("first", "last", "before", "end")  # where a planted site sits relative to its interval [s, e): s, e - 1, s - 1, e
PLANT_CLASS = 5
N_PLANTED = 24                              # kind x strand x state

_L = LONG
_ORDERED = [
    # single-word and word-border intervals, one class each so that every one shows
    ("long", 0, 1, 0), ("long", 31, 32, 1), ("long", 31, 33, 2), ("long", 32, 33, 3), ("long", 0, 32, 4), ("long", 0, 33, 5),
    # a lane border and a chunk border
    ("long", 127, 129, 6), ("long", CHUNK - 1, CHUNK + 1, 7),
    # exactly one whole chunk; the last base of a contig whose length is no multiple of 32; whole contigs of 92, 8192 and 8213 bp
    ("long", CHUNK, 2 * CHUNK, 1), ("long", _L - 1, _L, 0), ("small", 0, 92, 2), ("one", 0, CHUNK, 3), ("odd", 0, CHUNK + 21, 4),
    # one class in every relation: identical twice, nested, partly overlapping, adjacent
    ("long", 300, 400, 5), ("long", 300, 400, 5), ("long", 500, 700, 5), ("long", 550, 600, 5), ("long", 800, 900, 5), ("long", 850, 950, 5),
    ("long", 1000, 1100, 5), ("long", 1100, 1200, 5),
    # two classes over the same positions
    ("long", 2000, 2100, 6), ("long", 2000, 2100, 7),
    # one interval over all three chunks of a contig
    ("long", 5000, 2 * CHUNK + 250, 2),
]
# 200 one-base intervals inside one word (word 40 of the contig: 1280..1311), on eleven of its bits
_ORDERED += [("long", 1280 + (i % 11) * 3, 1281 + (i % 11) * 3, 5) for i in range(200)]
# eight classes on one position (4000)
_ORDERED += [("long", 3990 + c, 4001, c) for c in range(8)]
# the intervals the GATC sites are planted at: kind x strand x state, one interval each
PLANTED = [("one", 100 + 60 * i, 110 + 60 * i, PLANT_CLASS) for i in range(N_PLANTED)]
_ORDERED += PLANTED
SPECIAL = _ORDERED[:24]                     # the intervals the list above names one by one
INTERVALS = [_ORDERED[k] for k in np.random.default_rng(77).permutation(len(_ORDERED)).tolist()]      # unsorted
# The state of the background site (every position is one: A / T carry the 6mA site of '+' / '-', C / G the 5mC site) at the positions
# s - 1, s, e - 1 and e of the intervals of ``long`` listed first above, so that every such border sees as many states as its positions
# allow.  One position carries one site and so one state: [0,1) and [L-1,L) have two border positions inside the contig and see two states;
# [32,33) needs 31, 32, 33 all different, and then position 0 cannot differ from both {31, 32} and {32, 33}: of [0,32) and [0,33) one sees
# two states whatever is chosen ([0,32) here).  Every other listed border sees all three.
FORCED = {0: 0, 1: 1, 30: 2, 31: 0, 32: 1, 33: 2, 126: 0, 127: 1, 128: 2, 129: 0, CHUNK - 2: 0, CHUNK - 1: 1, CHUNK: 2, CHUNK + 1: 0,
          2 * CHUNK - 1: 0, 2 * CHUNK: 1, LONG - 2: 0, LONG - 1: 1}
SITE_OF_LETTER = {"A": ("a", 0), "T": ("a", 1), "C": ("m", 0), "G": ("m", 1)}
SECOND_SET = [("long", 40, 70, 0), ("odd", 8200, 8213, 0), ("small", 3, 4, 0)]


def region_set(k_classes: int, intervals=None):
    """(intervals (contig name, start, end, class), K) of the set with K = 1, 3 or 8 classes: 8 = all of ``INTERVALS``; 3 = the classes 0
    and 5 as 0 and 1 and a declared class 2 without an interval; 1 = class 0 alone."""
    intervals = INTERVALS if intervals is None else intervals
    keep = {8: {c: c for c in range(8)}, 3: {0: 0, 5: 1}, 1: {0: 0}}[k_classes]
    return [(n, s, e, keep[c]) for n, s, e, c in intervals if c in keep], k_classes


def class_sets(intervals, k_classes: int) -> dict:
    """(contig name, class) -> the set of positions inside the class, built interval by interval."""
    out = {(n, c): set() for n in NAMES for c in range(k_classes)}
    for n, s, e, c in intervals:
        out[(n, c)].update(range(s, e))
    return out


def occurrences(seq: str, motif: str, i: int) -> list:
    """[(position of the modified base, strand 0 '+' / 1 '-')] of every occurrence, by a regex scan of the contig and of its reverse
    complement (overlapping matches included)."""
    pat = re.compile("(?=(" + motif + "))")
    n = len(seq)
    out = [(m.start() + i, 0) for m in pat.finditer(seq)]
    out += [(n - 1 - (m.start() + i), 1) for m in pat.finditer(seq.translate(COMPLEMENT)[::-1])]
    return out


def state_tables(length: int, rows, low=0.3, high=0.7) -> list:
    """[2 strands][length]: 0 mod, 1 nomod, 2 nocall from the rows (position, strand 0 / 1, fraction); a position called both ways is mod."""
    st = [[2] * length, [2] * length]
    for p, s, f in rows:
        if f <= low:
            st[s][p] = 1
    for p, s, f in rows:
        if f >= high:
            st[s][p] = 0
    return st


@functools.lru_cache(maxsize=None)
def geometry():
    """(name -> sequence, (mod type, name) -> rows (position, strand, fraction), the planted sites [(kind, strand, state, position)]).
    Random letters and calls; GATC sites planted at the intervals of ``PLANTED``; the states of ``FORCED`` at the listed borders."""
    rng = np.random.default_rng(3109)
    seqs = {n: list(rng.choice(list("ACGT"), size=LENGTHS[n])) for n in NAMES}
    piles = {}
    for mt in ("a", "m"):
        for n in NAMES:
            p, s = np.nonzero(rng.random((LENGTHS[n], 2)) < 0.6)
            f = rng.choice([0.0, 0.3, 0.5, 0.7, 1.0], size=len(p))
            piles[(mt, n)] = [(int(a), int(b), float(x)) for a, b, x in zip(p, s, f)]
    planted = []
    for i, (n, s, e, _) in enumerate(PLANTED):
        kind, strand, state = i % 4, (i // 4) % 2, i // 8
        q = (s, e - 1, s - 1, e)[kind]
        at = q - 1 if strand == 0 else q - 2                              # GATC at x: its '+' site at x + 1, its '-' site at x + 2
        seqs[n][at:at + 4] = "GATC"
        rows = [r for r in piles[("a", n)] if not (r[0] == q and r[1] == strand)]
        if state < 2:
            rows.append((q, strand, 1.0 if state == 0 else 0.0))
        piles[("a", n)] = rows
        planted.append((KINDS[kind], strand, state, q))
    for q, state in FORCED.items():
        mt, strand = SITE_OF_LETTER[seqs["long"][q]]
        rows = [r for r in piles[(mt, "long")] if not (r[0] == q and r[1] == strand)]
        if state < 2:
            rows.append((q, strand, 1.0 if state == 0 else 0.0))
        piles[(mt, "long")] = rows
    return {n: "".join(s) for n, s in seqs.items()}, piles, planted


def contigs_of(b: str) -> list:
    return [n for n in NAMES if BINS[n] == b]


def candidates() -> list:
    """[(bin, mod type, motif, mod position)]: every motif and both backgrounds in both bins with a contig, bins interleaved."""
    return [(b, mt, m, i) for m, i, mt in MOTIFS + BACKGROUNDS for b in ("b1", "b2")]


IUPAC = {"R": "[AG]", "Y": "[CT]", "S": "[CG]", "W": "[AT]", "K": "[GT]", "M": "[AC]", "B": "[CGT]", "D": "[AGT]", "H": "[ACT]", "V": "[ACG]", "N": "."}


def regex_of(iupac: str) -> str:
    """A motif in the IUPAC spelling of bin-motifs.tsv as the regex ``occurrences`` scans for."""
    return "".join(IUPAC.get(x, x) for x in iupac)


def sites_in(contigs, rows_of, motif: str, i: int) -> list:
    """[(contig name, position, strand, state)] of a motif on ``contigs`` = [(name, sequence)] in the engine's order: contigs as given,
    ascending position, '+' first; ``rows_of(name)``: the pileup rows (position, strand 0 / 1, fraction) of the motif's mod type."""
    out = []
    for n, seq in contigs:
        st = state_tables(len(seq), rows_of(n))
        out += [(n, p, s, st[s][p]) for p, s in sorted(occurrences(seq, motif, i))]
    return out


@functools.lru_cache(maxsize=None)
def sites_of(cand) -> list:
    """``sites_in`` of a candidate (bin, mod type, motif, mod position) of the geometry input."""
    b, mt, motif, i = cand
    seqs, piles, _ = geometry()
    return sites_in([(n, seqs[n]) for n in contigs_of(b)], lambda n: piles[(mt, n)], motif, i)


def class_mask(sets: dict, k_classes: int, contig: str, p: int) -> int:
    return sum(1 << c for c in range(k_classes) if p in sets[(contig, c)])


def table_of(sites, names, sets: dict, k_classes: int) -> np.ndarray:
    """int64[len(names), K + 1, 2, 3]: ``sites`` per contig of ``names``, class (cell K: outside), occurrence strand and state."""
    t = np.zeros((len(names), k_classes + 1, 2, 3), dtype=np.int64)
    for n, p, s, state in sites:
        mask = class_mask(sets, k_classes, n, p)
        for c in range(k_classes):
            if mask >> c & 1:
                t[names.index(n), c, s, state] += 1
        if mask == 0:
            t[names.index(n), k_classes, s, state] += 1
    return t


def expected_table(cand, sets: dict, k_classes: int) -> np.ndarray:
    """``table_of`` of a candidate of the geometry input over the contigs of its bin."""
    return table_of(sites_of(cand), contigs_of(cand[0]), sets, k_classes)


def records_of(site_lists, contig_ids: dict, sets: dict, k_classes: int, states=(0, 1, 2), class_set=None, outside=False) -> list:
    """[(candidate index, contig id, position, code, class mask)] in the engine's order from the candidates' ``site_lists``: the sites
    whose state is in ``states`` and that are inside a class of the bit set ``class_set`` (default: every class) or, with ``outside``,
    outside every class."""
    class_set = (1 << k_classes) - 1 if class_set is None else class_set
    out = []
    for j, sites in enumerate(site_lists):
        for n, p, s, state in sites:
            mask = class_mask(sets, k_classes, n, p)
            if state in states and (mask & class_set or (outside and mask == 0)):
                out.append((j, contig_ids[n], p, 4 * s + state, mask))
    return out


def expected_records(cands, sets: dict, k_classes: int, states=(0, 1, 2), class_set=None, outside=False) -> list:
    """``records_of`` of candidates of the geometry input."""
    return records_of([sites_of(c) for c in cands], {n: k for k, n in enumerate(NAMES)}, sets, k_classes, states, class_set, outside)


def pileup_arrays(mt: str):
    """(contig id, position, strand byte, fraction) of one mod type for ``ScanEngine.upload_pileup``."""
    _, piles, _ = geometry()
    cid, pos, strand, frac = [], [], [], []
    for c, n in enumerate(NAMES):
        rows = piles[(mt, n)]
        cid += [c] * len(rows)
        pos += [r[0] for r in rows]
        strand += [ord("+-"[r[1]]) for r in rows]
        frac += [r[2] for r in rows]
    return np.array(cid, np.uint32), np.array(pos, np.int64), np.array(strand, np.uint8), np.array(frac, np.float64)


def interval_arrays(intervals):
    """(contig ids, starts, ends, classes) of ``ScanEngine.upload_regions``."""
    return ([NAMES.index(n) for n, _, _, _ in intervals], [s for _, s, _, _ in intervals], [e for _, _, e, _ in intervals], [c for _, _, _, c in intervals])
