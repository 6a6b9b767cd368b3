"""``nanomotif motif_coverage``: how much of a bin's methylation the motifs of a ``bin-motifs.tsv`` explain.

The reference answers this only in passing: ``find_best_candidates`` logs "x % of sequences remaining" while it removes the windows
each kept motif explains (find_motifs_bin.py:801-823) — before pruning, before the missed candidates are added and before the merge
stage rewrites the motifs, and never into a file.  This command takes the rows that ended up in ``bin-motifs.tsv`` and reports, per
(bin, mod type): the share of the confidently methylated positions that lies on an occurrence of at least one motif of the bin, which
motifs are redundant (every methylated site they hit is also hit by another motif of the bin) and, on request, where the unexplained
methylated positions are.

Arguments and ingest are those of ``motif_sites`` (``loading.load_engine``, ``candidates_of_bin_motifs``: complements included,
duplicates dropped), so the state planes are the ones ``bin-motifs.tsv`` was scored on.  Every bin with a resident contig x every mod
type present in the pileup is a SET, also when ``bin-motifs.tsv`` has no motif for it: that row is how a bin with methylation and
nothing discovered is found.  Sets in the order sorted bin names, mod types in slot order, motifs in file order.

Files: ``motif-coverage.tsv`` (one row per set), ``motif-coverage-contigs.tsv`` (per set and contig, the ten per-strand columns),
``motif-coverage-motifs.tsv`` (per motif: its own counts and the counts only it explains), with ``--unexplained_sites``
``unexplained-sites.bed`` (contig, start, end, mod_type, 0, strand, bin; no header; set order, contigs in bin order, ascending
position, '+' before '-').
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import fasta
from .engine import SITE_MINUS, ScanEngine
from .export_run import closing, finish, open_run, resident_bins, split_known, table_text, write_texts
from .loading import kept_mod_types

SETS_NAME = "motif-coverage.tsv"
CONTIGS_NAME = "motif-coverage-contigs.tsv"
MOTIFS_NAME = "motif-coverage-motifs.tsv"
BED_NAME = "unexplained-sites.bed"
SETS_HEADER = ["bin", "mod_type", "n_motifs", "n_mod", "n_mod_explained", "n_mod_unexplained", "fraction_explained", "n_nomod", "n_nomod_covered",
               "n_nocall_covered"]
STRAND_COLUMNS = ["n_mod", "n_mod_explained", "n_nomod", "n_nomod_covered", "n_nocall_covered"]
CONTIGS_HEADER = ["bin", "contig", "mod_type"] + [c + "_fwd" for c in STRAND_COLUMNS] + [c + "_rev" for c in STRAND_COLUMNS]
MOTIFS_HEADER = ["bin", "motif", "mod_type", "mod_position", "n_mod", "n_nomod", "n_mod_exclusive", "n_nomod_exclusive"]
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_coverage.json)


class CoverageSet:
    """One (bin, mod type) and the candidates (``motif_sites.SiteCandidate``) ``bin-motifs.tsv`` lists for it, in file order."""
    __slots__ = ("bin", "mod_type", "candidates")

    def __init__(self, bin, mod_type, candidates):
        self.bin, self.mod_type, self.candidates = bin, mod_type, list(candidates)

    def engine_set(self):
        return (self.bin, self.mod_type, [c.engine_candidate()[0] for c in self.candidates])

    def __repr__(self):
        return f"CoverageSet({self.bin!r}, {self.mod_type!r}, {[c.name for c in self.candidates]})"


def build_sets(bins, mod_types, cands) -> list:
    """The sets of a run: ``bins`` (names of the bins with a resident contig) sorted x ``mod_types`` in the order given (slot order),
    each with its candidates of ``cands`` in file order — also the sets no candidate belongs to.  Candidates of other bins or mod
    types are left out (the caller warns about them)."""
    by_key = {}
    for c in cands:
        by_key.setdefault((c.bin, c.mod_type), []).append(c)
    return [CoverageSet(b, mt, by_key.get((b, mt), [])) for b in sorted(bins) for mt in mod_types]


def format_sets(sets, tables) -> str:
    """motif-coverage.tsv: per set the ten columns of its int64[n_contigs, 10] table summed over contigs and strands."""
    rows = []
    for s, t in zip(sets, tables):
        t = np.asarray(t, dtype=np.int64).reshape(-1, 10).sum(axis=0)
        n_mod, n_exp = int(t[0] + t[5]), int(t[1] + t[6])
        fraction = "%.6f" % (n_exp / n_mod) if n_mod else "nan"
        rows.append([s.bin, s.mod_type, len(s.candidates), n_mod, n_exp, n_mod - n_exp, fraction, int(t[2] + t[7]), int(t[3] + t[8]), int(t[4] + t[9])])
    return table_text(SETS_HEADER, rows)


def format_contigs(sets, contig_names, tables) -> str:
    """motif-coverage-contigs.tsv: one row per (set, contig of its bin) with the ten per-strand columns as the engine returns them."""
    rows = []
    for s, names, t in zip(sets, contig_names, tables):
        t = np.asarray(t, dtype=np.int64).reshape(-1, 10)
        for name, row in zip(names, t):
            rows.append([s.bin, fasta.original_name(name), s.mod_type] + [int(x) for x in row])
    return table_text(CONTIGS_HEADER, rows)


def format_motifs(sets, site_counts, exclusive) -> str:
    """motif-coverage-motifs.tsv: per candidate, in set order, n_mod / n_nomod of its own ``motif_site_counts`` table (int64[n, 6])
    and of its exclusive table (int64[n, 4]), both summed over the bin's contigs and the strands.  ``site_counts`` / ``exclusive``:
    per set a list with one table per candidate."""
    rows = []
    for s, own, excl in zip(sets, site_counts, exclusive):
        for c, six, four in zip(s.candidates, own, excl):
            six = np.asarray(six, dtype=np.int64).reshape(-1, 6).sum(axis=0)
            four = np.asarray(four, dtype=np.int64).reshape(-1, 4).sum(axis=0)
            rows.append([c.bin, c.motif, c.mod_type, c.mod_position, int(six[0] + six[3]), int(six[1] + six[4]), int(four[0] + four[2]),
                         int(four[1] + four[3])])
    return table_text(MOTIFS_HEADER, rows)


def format_unexplained(rec, sets, contig_names) -> str:
    """The lines of unexplained-sites.bed for a batch of ``ScanEngine.unexplained_sites`` records."""
    if len(rec) == 0:
        return ""
    names = np.array([fasta.original_name(n) for n in contig_names], dtype=object)
    mts = np.array([s.mod_type for s in sets], dtype=object)
    bins = np.array([s.bin for s in sets], dtype=object)
    pos = rec["pos"].astype(np.int64)
    strand = np.where(rec["code"] & SITE_MINUS, "-", "+")
    cols = (names[rec["contig"]], pos.astype(str), (pos + 1).astype(str), mts[rec["set"]], strand, bins[rec["set"]])
    return "".join(f"{c}\t{a}\t{b}\t{mt}\t0\t{st}\t{bn}\n" for c, a, b, mt, st, bn in zip(*cols))


def coverage_tables(eng: ScanEngine, sets: list):
    """(contig names per set, set tables, exclusive tables per set, motif_site_counts tables per set) of ``sets`` (CoverageSet)."""
    res = eng.motif_coverage([s.engine_set() for s in sets])
    flat = [c.engine_candidate() for s in sets for c in s.candidates]
    own = [t for _, t in eng.motif_site_counts(flat)] if flat else []
    site_counts, k = [], 0
    for s in sets:
        site_counts.append(own[k:k + len(s.candidates)])
        k += len(s.candidates)
    return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res], site_counts


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    eng, cands, status = open_run("motif_coverage", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        mod_types = kept_mod_types(eng)
        sets = build_sets(resident_bins(eng), mod_types, split_known(cands, eng, mod_types))
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        names, set_tables, exclusive, site_counts = coverage_tables(eng, sets)
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        write_texts(args.out, (SETS_NAME, CONTIGS_NAME, MOTIFS_NAME),
                    (format_sets(sets, set_tables), format_contigs(sets, names, set_tables), format_motifs(sets, site_counts, exclusive)))
        t_text = time.perf_counter() - t0
        n_records = 0
        if args.unexplained_sites:
            with open(os.path.join(args.out, BED_NAME), "w") as f:
                t0 = time.perf_counter()
                for rec in eng.unexplained_sites([s.engine_set() for s in sets]):
                    t1 = time.perf_counter()
                    t_eng += t1 - t0
                    f.write(format_unexplained(rec, sets, eng.contig_names))
                    n_records += len(rec)
                    t0 = time.perf_counter()
                    t_text += t0 - t1
                t_eng += time.perf_counter() - t0
        finish("motif_coverage", TIMINGS, t_eng, t_text, sets=len(sets), candidates=sum(len(s.candidates) for s in sets), unexplained_records=n_records)
    return 0
