"""``nanomotif motif_strands``: whether the two strands of every motif site agree — fully methylated, hemimethylated, unmethylated.

A restriction-modification methyltransferase methylates both strands of its site: the same motif for a palindrome, the motif and its
reverse complement otherwise.  The reference pairs a motif with its complement by name only (``join_motif_complements``) and never looks
at the sites; modkit has ``pileup-hemi`` for CpG.  Here every occurrence of every motif of a ``bin-motifs.tsv`` is classified ONCE by the
state of its own modified base and of its PARTNER, the modified base of the other strand's motif inside the same site
(``ScanEngine.motif_strand_counts`` / ``motif_strand_sites``, nm_motif_strands_*): the joint 3 x 3 table of (mod, nomod, nocall) of the
own base x (mod, nomod, nocall) of the partner, which two ``motif_sites`` runs only give the marginals of.  It flags freshly replicated
DNA, an orphan single-strand methyltransferase, a complement that discovery missed and a strand bias of the caller.

The pileup goes through the ingest path of ``motif_discovery`` (``loading.load_engine``), so summed over the partner's state the table
gives the row's ``n_mod`` / ``n_nomod`` of ``bin-motifs.tsv``, summed over the own state its ``n_mod_complement`` / ``n_nomod_complement``.

Partner rule per candidate of ``--bin_motifs`` (``motif_sites.candidates_of_files``; ``partner_position`` j counts in the reverse
complement of the motif, include/nmscan.h):
  a row with a ``motif_complement``    j = ``mod_position_complement``; the complement is its own candidate with j = the row's ``mod_position``
  a row without one                    one candidate for every position of the reverse complement whose letter is exactly the mod type's
                                       canonical base (for a palindrome that includes j = mod_position); a motif with no such position is
                                       left out and named in a log warning

Files (tab-separated, header line):
  ``motif-strands.tsv``          per candidate: the nine counts ``n_<own>_<partner>`` summed over contigs and over both occurrence strands —
                                 for ``palindrome`` = 1 (the motif is its own reverse complement and j = mod_position, so the '-'
                                 occurrences are the '+' ones seen from the partner) over the '+' occurrences only: each duplex site
                                 counts once; ``n_full`` / ``n_hemi_own`` / ``n_hemi_partner`` / ``n_unmethylated``, their shares among
                                 the sites called on both strands, and ``strand_bias_p`` = ``motif_compare.mcnemar_p`` of the two hemi counts
  ``motif-strands-contigs.tsv``  per (candidate, contig of its bin): the eighteen per-strand columns as the engine returns them
  ``hemi-sites.bed``             with ``--hemi_sites``: contig, start, end, motif_modtype_modposition, 0, strand, own-partner, bin, partner
                                 position — no header, the records of ``--pairs`` (default mod-nomod,nomod-mod) in candidate order, within a
                                 candidate contigs in bin order, ascending position, '+' before '-'
There is no per-bin background file next to these (``motif-compare-bins.tsv`` has one): the one-letter candidate "canonical base against
the same position on the other strand" (d = 0) can never be called on both strands — the other strand holds the complementary letter
there, which carries no call of this mod type — so its table is the three columns ``motif_sites`` already gives.
"""
from __future__ import annotations

import csv
import logging as log
import math
import os
import time

import numpy as np

from . import fasta
from .engine import HEMI, PAIRS, SITE_STATES, ScanEngine, partner_offset
from .export_run import closing, finish, open_run, split_known, table_text, write_texts
from .motif import MOD_TYPE_TO_CANONICAL, Motif, iupac_to_regex
from .motif_compare import mcnemar_p
from .motif_sites import SiteCandidate, candidates_of_files, write_site_batches

MAIN_NAME = "motif-strands.tsv"
CONTIGS_NAME = "motif-strands-contigs.tsv"
BED_NAME = "hemi-sites.bed"
COUNT_COLUMNS = [f"n_{a}_{b}" for a in SITE_STATES for b in SITE_STATES]
DERIVED_COLUMNS = ["n_full", "n_hemi_own", "n_hemi_partner", "n_unmethylated", "frac_full", "frac_hemi", "frac_unmethylated", "strand_bias_p"]
KEY_COLUMNS = ["bin", "motif", "mod_type", "mod_position", "partner_position", "palindrome"]
MAIN_HEADER = KEY_COLUMNS + COUNT_COLUMNS + DERIVED_COLUMNS
CONTIGS_HEADER = ["bin", "contig", "motif", "mod_type", "mod_position", "partner_position"] + [c + "_fwd" for c in COUNT_COLUMNS] + [c + "_rev" for c in COUNT_COLUMNS]
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_strands.json)


def parse_pairs(text) -> tuple:
    """``--pairs mod-nomod,nomod-mod`` -> the pairs in the canonical order, each once; ValueError names what is none."""
    asked = [t.strip() for t in str(text).split(",") if t.strip()]
    bad = [t for t in asked if t not in PAIRS]
    if bad or not asked:
        raise ValueError(f"--pairs takes a comma-separated selection of {', '.join(PAIRS)}; got {text!r}")
    return tuple(t for t in PAIRS if t in asked)


class StrandCandidate(SiteCandidate):
    """A ``SiteCandidate`` with the position of its partner's modified base in the reverse complement of the motif."""
    __slots__ = ("partner_position",)

    def __init__(self, bin, motif, mod_type, mod_position, partner_position):
        SiteCandidate.__init__(self, bin, motif, mod_type, mod_position)
        self.partner_position = int(partner_position)

    @property
    def key(self):
        return (self.bin, self.motif, self.mod_type, self.mod_position, self.partner_position)

    def _motif(self):
        return Motif(iupac_to_regex(self.motif), self.mod_position)

    @property
    def offset(self) -> int:
        return partner_offset(self._motif(), self.partner_position)

    @property
    def palindrome(self) -> bool:
        """The '-' occurrences are the '+' occurrences seen from the partner: the motif is its own reverse complement and the partner
        is its own modified base."""
        m = self._motif()
        return list(m.reverse_compliment().sets) == list(m.sets) and self.partner_position == self.mod_position

    def engine_candidate(self):
        return (self._motif(), self.mod_type, self.bin, self.partner_position)

    def __repr__(self):
        return f"StrandCandidate({self.bin!r}, {self.name!r}, partner {self.partner_position})"


def complement_partners(paths) -> dict:
    """(bin, motif, mod_type, mod_position) -> [partner positions] from the rows of several bin-motifs.tsv that name a
    ``motif_complement``: the row's motif gets ``mod_position_complement``, the complement the row's ``mod_position``."""
    out = {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f, delimiter="\t"):
                comp = (row.get("motif_complement") or "").strip()
                if not comp or comp.lower() in ("nan", "none", "null"):
                    continue
                i, j = int(float(row["mod_position"])), int(float(row["mod_position_complement"]))
                for key, partner in (((row["reference"], row["motif"], row["mod_type"], i), j), ((row["reference"], comp, row["mod_type"], j), i)):
                    if partner not in out.setdefault(key, []):
                        out[key].append(partner)
    return out


def canonical_partners(motif: str, mod_type: str, mod_position: int) -> list:
    """The positions of the reverse complement of ``motif`` (IUPAC) whose letter is exactly the canonical base of ``mod_type``."""
    rc = Motif(iupac_to_regex(motif), mod_position).reverse_compliment()
    base = Motif(MOD_TYPE_TO_CANONICAL[mod_type], 0).sets[0]
    return [j for j, m in enumerate(rc.sets) if m == base]


def strand_candidates(cands, partners) -> list:
    """The ``StrandCandidate`` list of ``cands`` (``SiteCandidate``, file order) under the partner rule; ``partners``:
    ``complement_partners`` of the same files.  A motif without a partner is left out with a warning."""
    out = []
    for c in cands:
        js = partners.get(c.key)
        if js is None:
            js = canonical_partners(c.motif, c.mod_type, c.mod_position) if c.mod_type in MOD_TYPE_TO_CANONICAL else []
        if not js:
            log.warning(f"{c!r}: the reverse complement holds no {MOD_TYPE_TO_CANONICAL.get(c.mod_type, '?')} the other strand could be modified at; skipped")
        out += [StrandCandidate(c.bin, c.motif, c.mod_type, c.mod_position, j) for j in js]
    return out


def derived_columns(nine) -> list:
    """The text of the derived columns of one summed 3 x 3 table (int[9], index 3 * own state + partner state)."""
    n = [int(x) for x in nine]
    full, hemi_own, hemi_partner, unmeth = n[0], n[1], n[3], n[4]
    both = full + hemi_own + hemi_partner + unmeth                      # called on both strands
    if both:
        shares = ["%.6f" % (full / both), "%.6f" % ((hemi_own + hemi_partner) / both), "%.6f" % (unmeth / both)]
    else:
        shares = ["nan", "nan", "nan"]
    p = mcnemar_p(hemi_partner, hemi_own)
    return [str(full), str(hemi_own), str(hemi_partner), str(unmeth)] + shares + ["nan" if math.isnan(p) else "%.6g" % p]


def summed_nine(table, palindrome: bool) -> list:
    """int64[n_contigs, 18] -> the nine counts over contigs and both occurrence strands ('+' occurrences only for a palindrome)."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, 18).sum(axis=0)
    return [int(x) for x in (t[:9] if palindrome else t[:9] + t[9:])]


def format_main(cands, tables) -> str:
    """motif-strands.tsv: per ``StrandCandidate`` its int64[n_contigs, 18] table."""
    rows = []
    for c, t in zip(cands, tables):
        nine = summed_nine(t, c.palindrome)
        rows.append([c.bin, c.motif, c.mod_type, c.mod_position, c.partner_position, int(c.palindrome)] + nine + derived_columns(nine))
    return table_text(MAIN_HEADER, rows)


def format_contigs(cands, contig_names, tables) -> str:
    """motif-strands-contigs.tsv: one row per (candidate, contig of its bin) with the eighteen per-strand columns."""
    rows = []
    for c, names, t in zip(cands, contig_names, tables):
        t = np.asarray(t, dtype=np.int64).reshape(-1, 18)
        for name, row in zip(names, t):
            rows.append([c.bin, fasta.original_name(name), c.motif, c.mod_type, c.mod_position, c.partner_position] + [int(x) for x in row])
    return table_text(CONTIGS_HEADER, rows)


def export_hemi(eng: ScanEngine, cands: list, pairs, bed_file, max_records=None):
    """Write the records of ``pairs`` of ``cands`` to the open binary file ``bed_file``; returns (records, seconds in the engine,
    seconds in the text writer)."""
    batches = eng.motif_strand_sites([c.engine_candidate() for c in cands], pairs=pairs, max_records=max_records)
    return write_site_batches(eng, batches, cands, bed_file, symbol="nm_motif_strands_text", partner_offsets=[c.offset for c in cands])


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    pairs = HEMI if args.pairs is None else args.pairs if isinstance(args.pairs, tuple) else parse_pairs(args.pairs)
    eng, cands, status = open_run("motif_strands", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        files = [args.bin_motifs] if isinstance(args.bin_motifs, str) else list(args.bin_motifs)
        known = split_known(strand_candidates(cands, complement_partners(files)), eng, eng.slot_of_mod)
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        res = eng.motif_strand_counts([c.engine_candidate() for c in known])
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        tables = [t for _, t in res]
        write_texts(args.out, (MAIN_NAME, CONTIGS_NAME), (format_main(known, tables), format_contigs(known, [n for n, _ in res], tables)))
        t_text = time.perf_counter() - t0
        n_records = 0
        if args.hemi_sites:
            with open(os.path.join(args.out, BED_NAME), "wb") as f:
                n_records, t_e, t_t = export_hemi(eng, known, pairs, f)
            t_eng += t_e
            t_text += t_t
        finish("motif_strands", TIMINGS, t_eng, t_text, candidates=len(known), hemi_records=n_records)
    return 0
