"""Helper module of the motif_overlap tests (not a conftest): the geometry input, an independent brute force of the contract from Python
sets over a regex scan of the contigs (as ``test_gpu_export_shared.host_occurrences``; nothing shared with the engine), and the
symbolic-nesting oracle written letter by letter.

The contract (include/nmscan.h, nm_motif_overlap_count): a site of a motif is (contig, '+' coordinate of the modified base, strand) of
an occurrence of ``motif_sites``; two motifs share a site when both have it; the state is the position's.  The engine reads a motif
without its leading and trailing dots (nm_parse_motifs), so a site needs the motif's SPECIFIED positions inside the contig only:
``GATC.`` is ``GATC``.  An unstripped regex scan finds 205 of ``GATC.`` against 206 of ``GATC`` on ``long`` (the occurrence on the last
four bases); by the contract both have 206 and the pair is ``identical`` — ``test_the_input_has_what_the_checks_need`` pins both numbers."""
import re

import numpy as np

PLUS, MINUS = ord("+"), ord("-")
BORDER = 8192                                                            # a work item covers 8 192 bp of a contig
NAMES = ["short", "mid", "long"]
LENGTHS = {"short": 300, "mid": 9_000, "long": 17_000}
BIN_OF = {"short": "b0", "mid": "b1", "long": "b0"}
BINS = ["b0", "b1"]
CONTIGS = {b: [n for n in NAMES if BIN_OF[n] == b] for b in BINS}
COMP = str.maketrans("ACGT", "TGCA")
# (motif, mod position) per mod type, in set order
A_SET = [("GATC", 1), ("[AG]GATC[CT]", 2), ("GATC[ACT]", 1), ("[AGT]GATC", 2), ("GATC" + "." * 40 + "T", 1), ("GATC" + "." * 70 + "T", 1), ("GTAC", 2),
         ("GATC.", 1), ("[GC]ATC", 1), ("...GATC", 4)]                   # the last: a second spelling of GATC
M_SET = [("CC[AT]GG", 1), ("CCAGG", 1), ("CCTGG", 1)]                    # two children that partition their parent
SETS = {"a": A_SET, "m": M_SET}
# planted beside the 470 bp grid: modified bases on bit 31 and bit 0 of a word either side of the lane border 127 | 128
EXTRA = {"mid": [(126, "GATC"), (1054, "GATC"), (30, "CCAGG"), (63, "CCTGG"), (2175, "CCAGG"), (4000, "GGATCC"), (4100, "AGATCT"), (4200, "TGATCG"), (4300, "GTAC")],
         "long": [(127, "GATC"), (8190 + 470, "GATC"), (254, "CCTGG"), (127 + 8192, "CCAGG"), (12000, "GGATCC"), (12100, "AGATCT"), (12200, "CGATCG"), (12300, "GTAC")]}


def sequences():
    """Random contigs with GATC planted every 470 bp, across 8 191 | 8 192 and on the last four bases, a T 44 and 74 bp behind each
    (``test_gpu_export_shared.sequences``), and the occurrences of ``EXTRA``."""
    rng = np.random.default_rng(19)
    seqs = {}
    for name in NAMES:
        L = LENGTHS[name]
        s = rng.choice(list("ACGT"), size=L)
        for q in list(range(40, L - 80, 470)) + ([BORDER - 2] if L > BORDER + 80 else []) + [L - 4]:
            s[q:q + 4] = list("GATC")
            if q + 75 <= L:
                s[q + 44] = s[q + 74] = "T"
        for q, word in EXTRA.get(name, []):
            s[q:q + len(word)] = list(word)
        seqs[name] = "".join(s)
    return seqs


def pileup_rows():
    """mod type -> (contig id, position, strand, fraction) as ``upload_pileup`` takes them, and the dense states they mean:
    mod type -> contig -> uint8[2 (strand), length] with 0 mod, 1 nomod, 2 nocall (0.5 is neither; a position without a row has no call)."""
    rng = np.random.default_rng(23)
    rows, states = {}, {}
    for mt in "am":
        cid, pos, strand, frac = [], [], [], []
        states[mt] = {}
        for i, name in enumerate(NAMES):
            st = np.full((2, LENGTHS[name]), 2, np.uint8)
            for s, sign in enumerate((PLUS, MINUS)):
                p = np.flatnonzero(rng.random(LENGTHS[name]) < 0.7)
                f = rng.choice([0.95, 0.05, 0.5], size=len(p))
                cid.append(np.full(len(p), i)); pos.append(p); strand.append(np.full(len(p), sign, np.uint8)); frac.append(f)
                st[s, p[f > 0.7]] = 0
                st[s, p[f < 0.3]] = 1
            states[mt][name] = st
        rows[mt] = tuple(np.concatenate(x) for x in (cid, pos, strand, frac))
    return rows, states


def strip_dots(motif: str, pos: int):
    """The motif without its leading and trailing dots, and the modified position in it."""
    toks = re.findall(r"\[[ACGT]+\]|[ACGT.]", motif)
    lo, hi = 0, len(toks)
    while lo < hi and toks[lo] == ".":
        lo += 1
    while hi > lo and toks[hi - 1] == ".":
        hi -= 1
    return "".join(toks[lo:hi]), pos - lo


def regex_positions(seq, motif, pos):
    """The '+' coordinates of the modified base of every match of ``motif`` AS SPELLED (dots must lie inside the contig) on '+' and on
    '-', overlapping ones included."""
    rx = re.compile("(?=" + motif + ")")
    plus = [m.start() + pos for m in rx.finditer(seq)]
    minus = [len(seq) - 1 - (m.start() + pos) for m in rx.finditer(seq.translate(COMP)[::-1])]
    return plus, minus


def sites(seq, motif, pos) -> set:
    """{(position, strand)} of the contract: the stripped motif scanned on both strands."""
    plus, minus = regex_positions(seq, *strip_dots(motif, pos))
    return {(p, 0) for p in plus} | {(p, 1) for p in minus}


def count6(site_set, state) -> np.ndarray:
    """int64[2, 3] of a set of (position, strand) under the dense ``state`` uint8[2, length]."""
    out = np.zeros((2, 3), np.int64)
    for p, s in site_set:
        out[s, state[s, p]] += 1
    return out


class BruteForce:
    """Every motif's site set per contig, computed once; ``table(bin, mod type, owner, partners)`` = the int64[P + 2, n_contigs, 2, 3]
    the contract asks of the engine for motifs given as (motif, mod position)."""

    def __init__(self, seqs=None, states=None, contigs=None):
        """Default: the geometry input.  Else ``seqs``: contig -> sequence, ``states``: mod type -> contig -> uint8[2, length],
        ``contigs``: bin -> contig names in row order."""
        self.seqs = sequences() if seqs is None else seqs
        self.rows, self.states = pileup_rows() if states is None else (None, states)
        self.contigs = CONTIGS if contigs is None else contigs
        self._sites = {}

    def sites(self, name, motif):
        key = (name, motif)
        if key not in self._sites:
            self._sites[key] = sites(self.seqs[name], *motif)
        return self._sites[key]

    def table(self, b, mt, owner, partners) -> np.ndarray:
        names = self.contigs[b]
        out = np.zeros((len(partners) + 2, len(names), 2, 3), np.int64)
        for r, name in enumerate(names):
            st, own = self.states[mt][name], self.sites(name, owner)
            out[0, r] = count6(own, st)
            rest = set(own)
            for q, p in enumerate(partners):
                both = own & self.sites(name, p)
                out[1 + q, r] = count6(both, st)
                rest -= both
            out[len(partners) + 1, r] = count6(rest, st)
        return out

    def all_others(self, b, mt, ms=None):
        """Per motif of the (bin, mod type) set (``ms``; default: of the geometry input): the table with all other motifs of the set
        as partners, in set order."""
        ms = SETS[mt] if ms is None else ms
        return [self.table(b, mt, m, ms[:i] + ms[i + 1:]) for i, m in enumerate(ms)]


# ---------------------------------------------------------------------------------------------- the symbolic oracle, letter by letter
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT",
         "V": "ACG", "N": "ACGT"}


def letters_at(motif: str, pos: int, d: int) -> str:
    """The letters an IUPAC motif allows ``d`` positions from its modified base; all four outside it."""
    j = pos + d
    return IUPAC[motif[j]] if 0 <= j < len(motif) else "ACGT"


def symbolic_oracle(a, pos_a, b, pos_b) -> str:
    """identical / a_in_b / b_in_a / none of two IUPAC motifs aligned on their modified bases."""
    span = range(-max(pos_a, pos_b), max(len(a) - pos_a, len(b) - pos_b))
    a_in_b = all(set(letters_at(a, pos_a, d)) <= set(letters_at(b, pos_b, d)) for d in span)
    b_in_a = all(set(letters_at(b, pos_b, d)) <= set(letters_at(a, pos_a, d)) for d in span)
    return "identical" if a_in_b and b_in_a else "a_in_b" if a_in_b else "b_in_a" if b_in_a else "none"


def to_iupac(motif: str) -> str:
    """A regex-spelled motif of this file in IUPAC letters."""
    by_set = {"".join(sorted(v)): k for k, v in IUPAC.items()}
    return "".join("N" if t == "." else by_set["".join(sorted(t.strip("[]")))] for t in re.findall(r"\[[ACGT]+\]|[ACGT.]", motif))
