"""``nanomotif motif_compare``: which motifs changed their methylation between two pileups of one assembly.

Two samples mapped to the same assembly (two time points, two conditions, two strains on one reference): a phase-variable
methyltransferase turns a motif ON or OFF between them.  The reference has no counterpart; the nearest is two runs of
``motif_model_contig(..., save_motif_positions=True)`` (find_motifs_bin.py:1285-1331), one per pileup, joined on the host.  Here both
pileups are resident on one engine (sample A under the mod types' names, sample B under ``<mod type>@b``) and every occurrence of every
motif is classified ONCE by its state in both (``ScanEngine.motif_compare_counts`` / ``motif_compare_sites``, nm_motif_compare_*): the
joint 3 x 3 table of (mod, nomod, nocall) in A x (mod, nomod, nocall) in B, which two ``motif_sites`` runs only give the marginals of.

Both pileups go through the ingest path of ``motif_discovery`` (``loading.load_engine``: same readers, pre-filters, thresholds), so
``n_mod_a`` / ``n_nomod_a`` are the counts a ``bin-motifs.tsv`` of sample A holds for the motif, and likewise for B.  ``--bin_motifs``
takes one or more files (typically discovery on A and on B); the candidates are ``candidates_of_bin_motifs`` of each in order,
complements included, a (bin, motif, mod_type, position) seen before is not repeated.  A mod type is compared when at least one of the
two pileups kept a row of it.

Files (tab-separated, header line):
  ``motif-compare.tsv``          per candidate, in candidate order: the nine counts ``n_<a>_<b>`` summed over contigs and strands, the
                                 marginals, ``degree_a`` / ``degree_b`` = share methylated among the sites called in BOTH samples,
                                 ``degree_delta`` = (n_nomod_mod - n_mod_nomod) / sites called in both, and ``mcnemar_p`` (``mcnemar_p``)
  ``motif-compare-contigs.tsv``  per (candidate, contig of its bin): the eighteen per-strand columns as the engine returns them
  ``motif-compare-bins.tsv``     per (bin with a resident contig, sorted) x (compared mod type, slot order): the same columns for the
                                 one-letter motif "canonical base at position 0" — every position that can carry the modification, the
                                 background a motif's switch is read against
  ``switched-sites.bed``         with ``--switched_sites``: contig, start, end, motif_modtype_modposition, 0, strand, a>b, bin — no header,
                                 the records of ``--transitions`` (default mod>nomod,nomod>mod) in candidate order, within a candidate
                                 contigs in bin order, ascending position, '+' before '-'
"""
from __future__ import annotations

import math
import os
import time

import numpy as np

from . import fasta
from .engine import SITE_STATES, SWITCHED, TRANSITIONS, ScanEngine
from .export_run import background_candidates, bin_mod_keys, closing, finish, open_run, split_known, table_text, write_texts
from .loading import kept_mod_types
from .motif_sites import candidates_of_files, write_site_batches      # (candidates_of_files: this command's reader of --bin_motifs)

MAIN_NAME = "motif-compare.tsv"
CONTIGS_NAME = "motif-compare-contigs.tsv"
BINS_NAME = "motif-compare-bins.tsv"
BED_NAME = "switched-sites.bed"
SAMPLE_B_SUFFIX = "@b"                # sample B's classification of mod type x is resident under the label x + "@b"
COUNT_COLUMNS = [f"n_{a}_{b}" for a in SITE_STATES for b in SITE_STATES]
DERIVED_COLUMNS = ["n_mod_a", "n_nomod_a", "n_mod_b", "n_nomod_b", "degree_a", "degree_b", "degree_delta", "mcnemar_p"]
MAIN_HEADER = ["bin", "motif", "mod_type", "mod_position"] + COUNT_COLUMNS + DERIVED_COLUMNS
CONTIGS_HEADER = ["bin", "contig", "motif", "mod_type", "mod_position"] + [c + "_fwd" for c in COUNT_COLUMNS] + [c + "_rev" for c in COUNT_COLUMNS]
BINS_HEADER = ["bin", "mod_type"] + COUNT_COLUMNS + DERIVED_COLUMNS
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_compare.json)


def parse_transitions(text) -> tuple:
    """``--transitions mod>nomod,nomod>mod`` -> the transitions in the canonical order, each once; ValueError names what is none."""
    asked = [t.strip() for t in str(text).split(",") if t.strip()]
    bad = [t for t in asked if t not in TRANSITIONS]
    if bad or not asked:
        raise ValueError(f"--transitions takes a comma-separated selection of {', '.join(TRANSITIONS)}; got {text!r}")
    return tuple(t for t in TRANSITIONS if t in asked)


def labels_of(mod_type):
    """The resident classifications (sample A, sample B) of a mod type."""
    return (mod_type, mod_type + SAMPLE_B_SUFFIX)


def mcnemar_p(g: int, l: int) -> float:
    """Exact two-sided McNemar test on the discordant pairs: min(1, 2 P[X <= min(g, l)]), X ~ Binomial(g + l, 1/2); nan without
    discordant pairs.  float64: the largest term C(n, k) / 2^n through log-gamma, the smaller ones relative to it by the ratios
    C(n, i - 1) / C(n, i) = i / (n - i + 1) <= 1 (a decaying product, summed until it no longer counts)."""
    g, l = int(g), int(l)
    n, k = g + l, min(g, l)
    if n == 0:
        return float("nan")
    if 2 * k >= n:                    # g == l: P[X <= n / 2] >= 1/2
        return 1.0
    log_top = math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1) - n * math.log(2.0)
    total, scale, i = 1.0, 1.0, k     # sum over i = k, k - 1, ..., 0 of C(n, i) / C(n, k)
    while i > 0 and scale > 1e-20 * total:
        step = min(i, 1 << 20)
        idx = np.arange(i, i - step, -1, dtype=np.float64)
        terms = scale * np.cumprod(idx / (n - idx + 1.0))
        total += float(terms.sum())
        scale = float(terms[-1])
        i -= step
    return min(1.0, 2.0 * math.exp(log_top + math.log(total)))


def derived_columns(nine) -> list:
    """The text of the marginals, degrees and test of one summed 3 x 3 table (int[9], index 3 * state_a + state_b)."""
    n = [int(x) for x in nine]
    mod_a, nomod_a = n[0] + n[1] + n[2], n[3] + n[4] + n[5]
    mod_b, nomod_b = n[0] + n[3] + n[6], n[1] + n[4] + n[7]
    both = n[0] + n[1] + n[3] + n[4]                                   # called in both samples
    if both:
        degrees = ["%.6f" % ((n[0] + n[1]) / both), "%.6f" % ((n[0] + n[3]) / both), "%.6f" % ((n[3] - n[1]) / both)]
    else:
        degrees = ["nan", "nan", "nan"]
    p = mcnemar_p(n[3], n[1])
    return [str(mod_a), str(nomod_a), str(mod_b), str(nomod_b)] + degrees + ["nan" if math.isnan(p) else "%.6g" % p]


def _nine(table):
    t = np.asarray(table, dtype=np.int64).reshape(-1, 18).sum(axis=0)
    return [int(x) for x in t[:9] + t[9:]]


def format_main(cands, tables) -> str:
    """motif-compare.tsv: per candidate (``motif_sites.SiteCandidate``) its int64[n_contigs, 18] table summed over contigs and strands."""
    rows = []
    for c, t in zip(cands, tables):
        nine = _nine(t)
        rows.append([c.bin, c.motif, c.mod_type, c.mod_position] + nine + derived_columns(nine))
    return table_text(MAIN_HEADER, rows)


def format_contigs(cands, contig_names, tables) -> str:
    """motif-compare-contigs.tsv: one row per (candidate, contig of its bin) with the eighteen per-strand columns."""
    rows = []
    for c, names, t in zip(cands, contig_names, tables):
        t = np.asarray(t, dtype=np.int64).reshape(-1, 18)
        for name, row in zip(names, t):
            rows.append([c.bin, fasta.original_name(name), c.motif, c.mod_type, c.mod_position] + [int(x) for x in row])
    return table_text(CONTIGS_HEADER, rows)


def format_bins(keys, tables) -> str:
    """motif-compare-bins.tsv: per (bin, mod type) of ``keys`` the table of the one-letter background candidate."""
    rows = []
    for (b, mt), t in zip(keys, tables):
        nine = _nine(t)
        rows.append([b, mt] + nine + derived_columns(nine))
    return table_text(BINS_HEADER, rows)


def export_switched(eng: ScanEngine, cands: list, transitions, bed_file, max_records=None):
    """Write the records of ``transitions`` of ``cands`` to the open binary file ``bed_file``; returns (records, seconds in the engine,
    seconds in the text writer)."""
    batches = eng.motif_compare_sites([c.engine_candidate() for c in cands], labels_of, transitions=transitions, max_records=max_records)
    return write_site_batches(eng, batches, cands, bed_file, symbol="nm_motif_compare_text")


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    transitions = SWITCHED if args.transitions is None else args.transitions if isinstance(args.transitions, tuple) else parse_transitions(args.transitions)
    eng, cands, status = open_run("motif_compare", args, TIMINGS, pileups=[(args.pileup_a, None), (args.pileup_b, lambda mt: mt + SAMPLE_B_SUFFIX)])
    if eng is None:
        return status
    with closing(eng):
        TIMINGS["ingest_a_s"], TIMINGS["ingest_b_s"] = (r["seconds"] for r in eng.pileup_ingests)
        mod_types = kept_mod_types(eng)
        known = split_known(cands, eng, mod_types, wording="neither pileup holds rows")
        bin_keys = bin_mod_keys(eng, mod_types)
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        res = eng.motif_compare_counts([c.engine_candidate() for c in known], labels_of)
        background = eng.motif_compare_counts(background_candidates(bin_keys), labels_of)
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        tables = [t for _, t in res]
        write_texts(args.out, (MAIN_NAME, CONTIGS_NAME, BINS_NAME),
                    (format_main(known, tables), format_contigs(known, [n for n, _ in res], tables), format_bins(bin_keys, [t for _, t in background])))
        t_text = time.perf_counter() - t0
        n_records = 0
        if args.switched_sites:
            with open(os.path.join(args.out, BED_NAME), "wb") as f:
                n_records, t_e, t_t = export_switched(eng, known, transitions, f)
            t_eng += t_e
            t_text += t_t
        finish("motif_compare", TIMINGS, t_eng, t_text, ingest=f" (A {TIMINGS['ingest_a_s']:.2f}s, B {TIMINGS['ingest_b_s']:.2f}s)",
               candidates=len(known), switched_records=n_records)
    return 0
