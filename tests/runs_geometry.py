"""The geometry input of the ``motif_runs`` tests and an independent brute force over it, in plain Python: a regex scan of both strands
for the occurrences, dense per-position state tables from the pileup rows, ``itertools.groupby`` for the runs.  Nothing here is shared
with the engine.

Units: word = 32 bp, lane = 128 bp, chunk = 8192 bp.  The input (118 kbp, no contig above four chunks; bins b0_empty, b1, b2; mod types a
and m) is made of letters and of STATES laid over stretches of a contig, the same for both strands and both mod types:
  R random calls    M every position methylated    U every position unmethylated    N no call
and of a few planted arrays (``geometry``).  What each stretch is for is written beside it in ``LAYOUT``; that every case is really there
is asserted on the brute force's output by ``test_motif_runs_host.test_every_planted_case_is_present``."""
import functools
import itertools
import re

import numpy as np

CHUNK = 8192
NAMES = ["small", "one", "odd", "long", "bare", "p3", "j3", "d3", "n3"]
LENGTHS = {"small": 92, "one": CHUNK, "odd": CHUNK + 21, "long": 3 * CHUNK + 300, "bare": 700, "p3": 2 * CHUNK + 616, "j3": 2 * CHUNK + 1000,
           "d3": 2 * CHUNK + 1000, "n3": 2 * CHUNK + 1000}
BINS = {"small": "b1", "one": "b1", "odd": "b1", "long": "b1", "bare": "b1", "p3": "b2", "j3": "b2", "d3": "b2", "n3": "b2"}
BIN_NAMES = ["b0_empty", "b1", "b2"]
MOTIFS = [("GATC", 1, "a"), ("CC[AT]GG", 1, "m"), ("A" + "." * 40 + "C", 0, "a"), ("A" + "." * 70 + "T", 0, "a")]      # G = 1, 1, 2, 3 (regions_geometry's)
BACKGROUNDS = [("A", 0, "a"), ("C", 0, "m")]
COMPLEMENT = str.maketrans("ACGT", "TGCA")
STATE_NAMES = ("mod", "nomod", "nocall")
RUN_LENGTHS = (1, 2, 3, 15, 16, 17, 63, 64, 65)      # R - 1, R, R + 1 for R = 2, 16, 64; min_run - 1 and min_run for min_run = 3

# contig -> [(start, end, state letter)], later entries over earlier ones; everything else is R
LAYOUT = {
    "small": [(0, 92, "M")],
    # the end of `one` and the start of `odd`, neighbours in bin b1, in one state: the runs must not join
    "one": [(CHUNK - 600, CHUNK, "M")],
    "odd": [(0, 600, "M"), (CHUNK - 40, CHUNK + 21, "U")],               # and a run over the border of the last, 21 bp chunk
    # 6000 .. 16884 unmethylated: a run over three chunks whose middle chunk is uniform (n_runs = 1, a continuation AND continued)
    "long": [(6000, 2 * CHUNK + 500, "U")],
    "bare": [],
    # chunk 1 of p3 holds ONE called position (13191, planted below) that starts a run which ends as chunk 2's head
    "p3": [(CHUNK - 300, CHUNK, "M"), (CHUNK, 2 * CHUNK, "N"), (2 * CHUNK, 2 * CHUNK + 300, "U")],
    # chunk 1 of j3 and d3 has no A and no T: no occurrence of the `a` candidates; the border runs have the same / different states
    "j3": [(CHUNK - 600, CHUNK, "M"), (2 * CHUNK, 2 * CHUNK + 600, "M")],
    "d3": [(CHUNK - 600, CHUNK, "M"), (2 * CHUNK, 2 * CHUNK + 600, "U")],
    # chunk 1 of n3 has occurrences and not one call: joins by default, breaks under nocall_breaks
    "n3": [(CHUNK - 600, CHUNK, "M"), (CHUNK, 2 * CHUNK, "N"), (2 * CHUNK, 2 * CHUNK + 600, "M")],
}
POLY_MOD = ("long", 3000, 3300)             # 300 A, all methylated: a background run over two lane borders
POLY_ALT = ("long", 3400, 3700)             # 300 A, the states alternating at every position: 128 starts in lane 27
GATC_ARRAY = ("long", 4000, 4400)           # GATC x 100, random calls: '+' and '-' sites on neighbouring positions
LENGTH_A = ("one", 1000)                    # A x 255: methylated runs of RUN_LENGTHS, one unmethylated A between two of them
LENGTH_GATC = ("one", 3000)                 # GATC x 130: the sites' runs of RUN_LENGTHS[3:], one unmethylated site between two of them
BORDER_GATC = [("long", 30), ("long", 126), ("long", CHUNK - 2)]        # GATC whose two sites sit on 31 | 32, 127 | 128, 8191 | 8192
ONLY = ("p3", 13190)                        # GATC; its '+' site 13191 (and the C at 13193 for mod type m) the only call of the chunk
# GATC inside the stretches of one state either side of the borders above, so that the motif has a site there
EDGE_GATC = [("one", CHUNK - 50), ("odd", 20), ("p3", CHUNK - 100), ("p3", 2 * CHUNK + 50)] + [(n, at) for n in ("j3", "d3", "n3") for at in (CHUNK - 200, 2 * CHUNK + 100)]
BOTH_WAYS =[("one", 5000 + 37 * i) for i in range(40)]                 # positions called both ways on both strands


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


def _rows_of_states(st, rng) -> list:
    """Pileup rows of a dense table st[length][2] of 0 mod / 1 nomod / 2 nocall / 3 called both ways, the fractions drawn at and beyond
    the thresholds; some nocall positions carry a row in between."""
    rows = []
    for p, s in zip(*np.nonzero(st != 2)):
        v = int(st[p, s])
        if v in (0, 3):
            rows.append((int(p), int(s), float(rng.choice([0.7, 1.0]))))
        if v in (1, 3):
            rows.append((int(p), int(s), float(rng.choice([0.0, 0.3]))))
    for p, s in zip(*np.nonzero((st == 2) & (rng.random(st.shape) < 0.2))):
        rows.append((int(p), int(s), 0.5))
    return [rows[k] for k in rng.permutation(len(rows)).tolist()]


def _length_states() -> list:
    """mod runs of RUN_LENGTHS with one nomod element between two of them."""
    out = []
    for n in RUN_LENGTHS:
        out += [0] * n + [1]
    return out[:-1]


@functools.lru_cache(maxsize=None)
def geometry():
    """(name -> sequence, (mod type, name) -> rows (position, strand, fraction))."""
    rng = np.random.default_rng(3111)
    seqs = {n: rng.choice(list("ACGT"), size=LENGTHS[n]) for n in NAMES}
    seqs["bare"] = rng.choice(list("CG"), size=LENGTHS["bare"])                        # no site of an `a` candidate
    seqs["small"] = rng.choice(list("CG"), size=LENGTHS["small"])
    seqs["small"][[10, 51]] = ["A", "C"]                                               # one site of A.{40}C, one site of the background A
    for n in ("j3", "d3"):
        seqs[n][CHUNK:2 * CHUNK] = rng.choice(list("CG"), size=CHUNK)
    for n, s, e in (POLY_MOD, POLY_ALT):
        seqs[n][s:e] = "A"
    n, s, e = GATC_ARRAY
    seqs[n][s:e] = list("GATC" * ((e - s) // 4))
    seqs[LENGTH_A[0]][LENGTH_A[1]:LENGTH_A[1] + len(_length_states())] = "A"
    seqs[LENGTH_GATC[0]][LENGTH_GATC[1]:LENGTH_GATC[1] + 4 * 130] = list("GATC" * 130)
    for n, at in BORDER_GATC + [ONLY] + EDGE_GATC:
        seqs[n][at:at + 4] = list("GATC")
    piles = {}
    for mt in ("a", "m"):
        for n in NAMES:
            L = LENGTHS[n]
            st = rng.choice([0, 1, 2], p=[0.3, 0.3, 0.4], size=(L, 2))
            for s, e, letter in LAYOUT[n]:
                st[s:e] = "MUN".index(letter)
            if n == POLY_MOD[0]:
                st[POLY_MOD[1]:POLY_MOD[2]] = 0
                st[POLY_ALT[1]:POLY_ALT[2], :] = (np.arange(POLY_ALT[2] - POLY_ALT[1]) % 2)[:, None]
                st[POLY_ALT[1] - 1], st[POLY_ALT[2]] = 1, 0                            # (and the positions either side go on alternating)
                for _, at in BORDER_GATC[:2]:
                    st[at - 2:at + 6] = 0                                              # 31 | 32 and 127 | 128 inside one methylated run
            if n == LENGTH_A[0]:
                ls = _length_states()
                st[LENGTH_A[1] - 1] = st[LENGTH_A[1] + len(ls)] = 1                    # (closed either side)
                st[LENGTH_A[1]:LENGTH_A[1] + len(ls)] = np.array(ls)[:, None]
                # the GATC array: site 2 j at 4 j + 1 on '+', site 2 j + 1 at 4 j + 2 on '-'
                gs = [1] + sum(([0] * k + [1] for k in RUN_LENGTHS[3:]), [])
                gs += [1] * (260 - len(gs))
                for j, v in enumerate(gs):
                    st[LENGTH_GATC[1] + 4 * (j // 2) + 1 + j % 2] = v
                for _, p in BOTH_WAYS:
                    st[p] = 3
            if n == ONLY[0]:
                st[ONLY[1] + 1, 0] = st[ONLY[1] + 3, 0] = 1
            piles[(mt, n)] = _rows_of_states(st, rng)
    return {n: "".join(s.tolist()) for n, s in seqs.items()}, piles


def contigs_of(b: str) -> list:
    return [n for n in NAMES if BINS[n] == b]


def candidates() -> list:
    """[(bin, mod type, motif, mod position)]: every motif and both backgrounds in both bins with a contig, bins interleaved."""
    return [(b, mt, m, i) for m, i, mt in MOTIFS + BACKGROUNDS for b in ("b1", "b2")]


def sites_in(contigs, rows_of, motif: str, i: int) -> list:
    """[(contig name, position, strand, state)] of a motif on ``contigs`` = [(name, sequence)]: contigs as given, ascending position,
    '+' first; ``rows_of(name)``: the pileup rows (position, strand 0 / 1, fraction) of the motif's mod type."""
    out = []
    for n, seq in contigs:
        st = state_tables(len(seq), rows_of(n))
        out += [(n, p, s, st[s][p]) for p, s in sorted(occurrences(seq, motif, i))]
    return out


@functools.lru_cache(maxsize=None)
def sites_of(cand) -> list:
    b, mt, motif, i = cand
    seqs, piles = geometry()
    return sites_in([(n, seqs[n]) for n in contigs_of(b)], lambda n: piles[(mt, n)], motif, i)


def runs_in(sites, names, nocall_breaks=False) -> dict:
    """contig name -> [(state, n_sites, start, last)] in order of start: the runs of ``sites`` (``sites_in``'s order) per contig of
    ``names``.  The sequence: the called sites, with ``nocall_breaks`` all of them."""
    out = {}
    for n in names:
        seq = [(p, st) for c, p, _, st in sites if c == n and (nocall_breaks or st != 2)]
        assert len({p for p, _ in seq}) == len(seq)                       # a position carries one site
        runs = []
        for state, grp in itertools.groupby(seq, key=lambda x: x[1]):
            grp = list(grp)
            runs.append((state, len(grp), grp[0][0], grp[-1][0]))
        out[n] = runs
    return out


def count_table(sites, names, max_run: int, nocall_breaks=False) -> np.ndarray:
    """int64[len(names), 3, 3 + R] as ``ScanEngine.motif_run_counts`` defines it."""
    t = np.zeros((len(names), 3, 3 + max_run), dtype=np.int64)
    runs = runs_in(sites, names, nocall_breaks)
    for k, n in enumerate(names):
        for c, _, _, st in sites:
            if c == n:
                t[k, st, 1] += 1
        for state, length, _, _ in runs[n]:
            t[k, state, 0] += 1
            t[k, state, 2] = max(t[k, state, 2], length)
            t[k, state, 3 + min(length, max_run) - 1] += 1
    return t


def run_records(site_lists, names_of, contig_ids: dict, states=(1,), min_run=3, nocall_breaks=False) -> list:
    """[(candidate index, contig id, start, state, last, n_sites)] in the engine's order."""
    out = []
    for j, sites in enumerate(site_lists):
        runs = runs_in(sites, names_of[j], nocall_breaks)
        for n in names_of[j]:
            out += [(j, contig_ids[n], start, state, last, length) for state, length, start, last in runs[n] if state in states and length >= min_run]
    return out


@functools.lru_cache(maxsize=None)
def expected_table(cand, max_run: int, nocall_breaks: bool) -> np.ndarray:
    """Computed once per argument set and shared: never changed by a test."""
    return count_table(sites_of(cand), contigs_of(cand[0]), max_run, nocall_breaks)


@functools.lru_cache(maxsize=None)
def runs_of(cand, nocall_breaks: bool) -> dict:
    return runs_in(sites_of(cand), contigs_of(cand[0]), nocall_breaks)


def expected_records(cands, states=(1,), min_run=3, nocall_breaks=False) -> list:
    """``run_records`` of candidates of the geometry input (the runs of a candidate are computed once)."""
    ids = {n: k for k, n in enumerate(NAMES)}
    out = []
    for j, c in enumerate(cands):
        runs = runs_of(c, bool(nocall_breaks))
        for n in contigs_of(c[0]):
            out += [(j, ids[n], start, state, last, length) for state, length, start, last in runs[n] if state in states and length >= min_run]
    return out


def pileup_arrays(mt: str):
    """(contig id, position, strand byte, fraction) of one mod type for ``ScanEngine.upload_pileup``."""
    _, piles = geometry()
    cid, pos, strand, frac = [], [], [], []
    for c, n in enumerate(NAMES):
        rows = piles[(mt, n)]
        cid += [c] * len(rows)
        pos += [r[0] for r in rows]
        strand += [ord("+-"[r[1]]) for r in rows]
        frac += [r[2] for r in rows]
    return np.array(cid, np.uint32), np.array(pos, np.int64), np.array(strand, np.uint8), np.array(frac, np.float64)
