"""``nanomotif motif_shift``: how the READ FRACTIONS n_modified / n_valid_cov at the sites of the motifs of a ``bin-motifs.tsv`` change
between two pileups of one assembly.

``motif_compare`` reads the thresholded state planes: an occurrence is mod, nomod or nocall in each sample, so a motif that goes from 90 %
to 45 % methylated lands in "mod > nocall" and one that goes from 60 % to 35 % never leaves "nocall > nocall".  A phase-variable
methyltransferase, a mixed population or a shifted subpopulation shows in the fractions only, and a global offset between two basecaller
models can be told from a real change only against the bin's background read the same way.  People run ``modkit dmr pair`` with a motif BED
and join; here both pileups become READ STATISTICS on one assembly (``loading.load_readstats_engine`` with two paths: sample A in the
slots of the mod codes, sample B from slot 3) and are joined at every site on the device (nm_motif_shift_count / nm_motif_shift_sites).

Definitions (include/nmscan.h).  Per strand an occurrence is PAIRED (a kept record under its modified base in both samples), ONLY_A,
ONLY_B or BARE.  A paired site with (vA, mA), (vB, mB) goes UP when mB vA > mA vB, DOWN when smaller, else it is EQUAL; it is SHIFTED when
it moved and |mB / vB - mA / vA| >= ``--min_delta`` (three decimals at most: compared as permille in exact integers on the device).  The
joint histogram has ``--bins`` bins per axis, a site's bin on an axis is ``motif_fractions``' (min(B - 1, m B // v)).  The bin's background
— every A / every C of the bin, per mod type among its candidates — rides in the same engine calls.

Statistics, from the integer tables summed over strands (and contigs), plain Python on the host: ``mean_cov_*`` = sum_valid / n_paired and
``weighted_mean_*`` = sum_mod / sum_valid over the PAIRED sites, ``delta`` = weighted_mean_b - weighted_mean_a, ``sign_p`` the exact
two-sided binomial test on n_up against n_down (``motif_compare.mcnemar_p``), the nine zone counts ``n_<zone in A>_<zone in B>`` of the
joint histogram with ``--methylation_threshold_low`` / ``_high`` snapped to bin edges (``motif_fractions.snap_edges``),
``excess_delta`` = delta - bg_delta.  ``flag``, in float64 on n = n_paired, u = n_shift_up, d = n_shift_down with s = ``--min_share`` and
m = ``--minor_share``, first match: ``few_sites`` if n < ``--min_sites``; ``gained`` if u >= s n and d < m n; ``lost`` if d >= s n and
u < m n; ``mixed`` if u >= m n and d >= m n; else ``stable``.  The flag rule and its defaults (20 sites, 0.5, 0.1, a shift of 0.25) are
design choices of this command pinned on hand-made tables, not on real data; no likelihood stands behind them.

Files (tab-separated, header line; candidates in file order, contigs in bin order):
  ``motif-shift.tsv``          per candidate: the class counts, the statistics, the zones, ``flag`` and the bin's background (``bg_*``)
  ``motif-shift-contigs.tsv``  per (candidate, contig that holds an occurrence): the class counts, the means, the directions and ``flag``
  ``motif-shift-hist.tsv``     long form: per background and candidate, strand and non-zero cell (bin in A, bin in B) the number of sites
  ``shifted-sites.bed``        with ``--shifted_sites``: contig, start, end, motif_modtype_modposition, 0, strand, n_valid_a, n_mod_a,
                               n_valid_b, n_mod_b, up|down, bin — no header, the shifted sites of ``--directions`` in the order of
                               ``motif-pileup.bed``; formatted with numpy in Python
"""
from __future__ import annotations

import logging as log
import math
import os
import time

import numpy as np

from . import fasta
from .engine import SHIFT_DOWN, SHIFT_DTYPE, SHIFT_EXTRA, SHIFT_MAX_BINS, SHIFT_MIN_BINS, SHIFT_MINUS, SHIFT_SUMS, shift_permille
from .export_run import (READ_FILTER_SUFFIX, background_candidates, background_keys, closing, finish, open_readstats_run, parse_int_in, share_text,
                         split_known, table_text, write_texts)
from .motif import MOD_TYPE_TO_CANONICAL
from .motif_compare import mcnemar_p
from .motif_fractions import snap_edges

SUMMARY_NAME = "motif-shift.tsv"
CONTIGS_NAME = "motif-shift-contigs.tsv"
HIST_NAME = "motif-shift-hist.tsv"
BED_NAME = "shifted-sites.bed"
KEY_COLUMNS = ["bin", "motif", "mod_type", "mod_position"]
ZONES = ("low", "mid", "high")
CLASS_COLUMNS = ["n_occurrences", "n_paired", "n_only_a", "n_only_b", "n_bare"]
MEAN_COLUMNS = ["mean_cov_a", "weighted_mean_a", "mean_cov_b", "weighted_mean_b", "delta"]
SUMMARY_HEADER = KEY_COLUMNS + CLASS_COLUMNS + MEAN_COLUMNS + ["n_up", "n_down", "n_equal", "sign_p", "n_shift_up", "n_shift_down"] + [
    f"n_{a}_{b}" for a in ZONES for b in ZONES] + ["flag", "bg_n_paired", "bg_weighted_mean_a", "bg_weighted_mean_b", "bg_delta", "excess_delta"]
CONTIGS_HEADER = ["bin", "contig", "motif", "mod_type", "mod_position"] + CLASS_COLUMNS + MEAN_COLUMNS + ["n_up", "n_down", "n_shift_up", "n_shift_down", "flag"]
HIST_HEADER = KEY_COLUMNS + ["background", "strand", "bin_a", "bin_b", "n_sites"]
FLAGS = ("few_sites", "gained", "lost", "mixed", "stable")
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_shift.json)


def parse_bins(value) -> int:
    """``--bins``: 2..16; ValueError otherwise."""
    return parse_int_in("--bins", value, SHIFT_MIN_BINS, SHIFT_MAX_BINS, what=f"a number in [{SHIFT_MIN_BINS}, {SHIFT_MAX_BINS}]")


def parse_min_delta(value) -> int:
    """``--min_delta`` -> permille: a decimal number in 0..1 with at most three decimals, read as text (0.25 -> 250); ValueError otherwise."""
    text = str(value).strip()
    whole, _, frac = text.partition(".")
    if whole.isdigit() and (frac == "" or frac.isdigit()) and ("." not in text or frac != "") and len(frac) <= 3:
        t = int(whole) * 1000 + int((frac + "000")[:3])
        if t <= 1000:
            return t
    raise ValueError(f"--min_delta takes a number in 0..1 with at most three decimals; got {value!r}")


def flag_of(n_paired: int, n_shift_up: int, n_shift_down: int, min_sites: int, min_share: float, minor_share: float) -> str:
    n, u, d, s, m = float(n_paired), float(n_shift_up), float(n_shift_down), float(min_share), float(minor_share)
    if n < float(min_sites):
        return "few_sites"
    if u >= s * n and d < m * n:
        return "gained"
    if d >= s * n and u < m * n:
        return "lost"
    if u >= m * n and d >= m * n:
        return "mixed"
    return "stable"


def _diff_text(a, b) -> str:
    """b - a as ``%.6f``; empty when either is None."""
    return "" if a is None or b is None else "%.6f" % (b - a)


class Stats:
    """The statistics of one table uint64[..., 2, B B + 12] (a candidate's rows, or one of them) summed over everything but the last axis."""

    def __init__(self, table, bins: int, k_low: int, k_high: int, min_sites: int, min_share: float, minor_share: float):
        cells = bins * bins
        both = [int(x) for x in np.asarray(table, dtype=np.uint64).reshape(-1, cells + SHIFT_EXTRA).astype(object).sum(axis=0)] if np.size(table) else [0] * (cells + SHIFT_EXTRA)
        hist = np.array(both[:cells], dtype=object).reshape(bins, bins)
        self.sums = dict(zip(SHIFT_SUMS, both[cells:]))
        s = self.sums
        self.n_bare = s["occurrences"] - s["n_paired"] - s["n_only_a"] - s["n_only_b"]
        self.n_equal = s["n_paired"] - s["n_up"] - s["n_down"]
        edges = (0, k_low, k_high, bins)
        self.zones = [int(hist[edges[i]:edges[i + 1], edges[j]:edges[j + 1]].sum()) for i in range(3) for j in range(3)]
        self.wm_a, self.wm_b = share_text(s["sum_mod_a"], s["sum_valid_a"]), share_text(s["sum_mod_b"], s["sum_valid_b"])
        self.delta = s["sum_mod_b"] / s["sum_valid_b"] - s["sum_mod_a"] / s["sum_valid_a"] if s["sum_valid_a"] and s["sum_valid_b"] else None
        self.flag = flag_of(s["n_paired"], s["n_shift_up"], s["n_shift_down"], min_sites, min_share, minor_share)

    def classes(self):
        s = self.sums
        return [s["occurrences"], s["n_paired"], s["n_only_a"], s["n_only_b"], self.n_bare]

    def means(self):
        s = self.sums
        return [share_text(s["sum_valid_a"], s["n_paired"]), self.wm_a, share_text(s["sum_valid_b"], s["n_paired"]), self.wm_b, _diff_text(0.0, self.delta)]

    def sign_p(self) -> str:
        p = mcnemar_p(self.sums["n_up"], self.sums["n_down"])
        return "nan" if math.isnan(p) else "%.6g" % p


def hist_rows(key, background: int, table, bins: int) -> list:
    cells = bins * bins
    per_strand = np.asarray(table, dtype=np.uint64).astype(np.int64).reshape(-1, 2, cells + SHIFT_EXTRA).sum(axis=0)
    return [key + [background, "+-"[s], c // bins, c % bins, int(per_strand[s, c])] for s in (0, 1) for c in range(cells) if per_strand[s, c]]


def candidate_rows(cand, names, table, bg_table, bins: int, *args):
    """The rows of one candidate for (motif-shift.tsv, motif-shift-contigs.tsv, motif-shift-hist.tsv).  ``names`` / ``table``: its item of
    ``ScanEngine.motif_shift_counts``; ``bg_table``: the table of the background of its (bin, mod type), or None; ``args``: k_low, k_high,
    min_sites, min_share, minor_share."""
    key = [cand.bin, cand.motif, cand.mod_type, cand.mod_position]
    st = Stats(table, bins, *args)
    if bg_table is None:
        bg_cols = ["", "", "", "", ""]
    else:
        bg = Stats(bg_table, bins, *args)
        bg_cols = [bg.sums["n_paired"], bg.wm_a, bg.wm_b, _diff_text(0.0, bg.delta), _diff_text(bg.delta, st.delta)]
    s = st.sums
    summary = [key + st.classes() + st.means() + [s["n_up"], s["n_down"], st.n_equal, st.sign_p(), s["n_shift_up"], s["n_shift_down"]] + st.zones + [st.flag] + bg_cols]
    contigs = []
    for i, name in enumerate(names):
        c = Stats(table[i], bins, *args)
        if c.sums["occurrences"]:
            contigs.append([cand.bin, fasta.original_name(name), cand.motif, cand.mod_type, cand.mod_position] + c.classes() + c.means() +
                           [c.sums["n_up"], c.sums["n_down"], c.sums["n_shift_up"], c.sums["n_shift_down"], c.flag])
    return summary, contigs, hist_rows(key, 0, table, bins)


def format_files(cands, items, backgrounds, bins: int, k_low: int, k_high: int, min_sites=20, min_share=0.5, minor_share=0.1):
    """(motif-shift.tsv, motif-shift-contigs.tsv, motif-shift-hist.tsv) as text.  ``cands``: ``SiteCandidate`` in file order with their
    ``items`` = (contig names, uint64[n_contigs, 2, bins^2 + 12]) of ``ScanEngine.motif_shift_counts``; ``backgrounds``: [((bin, mod type),
    table)] in ``background_keys`` order — their histograms open motif-shift-hist.tsv."""
    rows = ([], [], [])
    bg_tables = dict(backgrounds)
    for (b, mt), table in backgrounds:
        rows[2].extend(hist_rows([b, MOD_TYPE_TO_CANONICAL[mt], mt, 0], 1, table, bins))
    for c, (names, table) in zip(cands, items):
        got = candidate_rows(c, names, table, bg_tables.get((c.bin, c.mod_type)), bins, k_low, k_high, min_sites, min_share, minor_share)
        for mine, new in zip(rows, got):
            mine += new
    return table_text(SUMMARY_HEADER, rows[0]), table_text(CONTIGS_HEADER, rows[1]), table_text(HIST_HEADER, rows[2])


def format_bed(records, cands, contig_names) -> str:
    """The lines of shifted-sites.bed for ``records`` (``engine.SHIFT_DTYPE``; ``candidate`` indexes ``cands``, ``contig`` ``contig_names``)."""
    if len(records) == 0:
        return ""
    names = np.array([c.name for c in cands], dtype=object)[records["candidate"]]
    bins = np.array([c.bin for c in cands], dtype=object)[records["candidate"]]
    contig = np.array(contig_names, dtype=object)[records["contig"]]
    pos = records["pos"].astype(np.int64)
    strand = np.where(records["code"] & SHIFT_MINUS, "-", "+")
    way = np.where(records["code"] & SHIFT_DOWN, "down", "up")
    cols = [contig, pos, pos + 1, names, np.zeros(len(pos), np.int64), strand, records["n_valid_a"], records["n_mod_a"], records["n_valid_b"], records["n_mod_b"], way, bins]
    return "".join("\t".join(map(str, row)) + "\n" for row in zip(*(c.tolist() for c in cols)))


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    bins, permille = parse_bins(args.bins), shift_permille(args.min_delta)          # (the parser has made permille of --min_delta)
    try:
        k_low, k_high = snap_edges(args.methylation_threshold_low, args.methylation_threshold_high, bins)
    except ValueError as e:
        log.error(str(e))
        return 2
    eng, cands, status = open_readstats_run("motif_shift", args, TIMINGS, pileups=(args.pileup_a, args.pileup_b))
    if eng is None:
        return status
    with closing(eng):
        both = {mt for mt, n in eng.readstats_kept.items() if n} | {mt for mt, n in eng.readstats_kept_b.items() if n}
        known = split_known(cands, eng, both, suffix=READ_FILTER_SUFFIX, wording="neither pileup holds rows")
        bg_keys = background_keys(known)
        os.makedirs(args.out, exist_ok=True)
        # the background's one-letter candidates ride in the same engine call, ahead of the motifs that are read against them
        batch = background_candidates(bg_keys) + [c.engine_candidate() for c in known]
        t0 = time.perf_counter()
        items = [(names, table) for _, names, table in eng.motif_shift_counts(batch, bins=bins, min_delta_permille=permille)]
        records = None
        if args.shifted_sites:
            parts = [sb.records for sb in eng.motif_shift([c.engine_candidate() for c in known], min_delta_permille=permille, select=args.directions)]
            records = np.concatenate(parts) if parts else np.zeros(0, dtype=SHIFT_DTYPE)
        t1 = time.perf_counter()
        texts = format_files(known, items[len(bg_keys):], [(key, items[k][1]) for k, key in enumerate(bg_keys)], bins, k_low, k_high, int(args.min_sites),
                             float(args.min_share), float(args.minor_share))
        bed = None if records is None else format_bed(records, known, [fasta.original_name(n) for n in eng.contig_names])
        write_texts(args.out, (SUMMARY_NAME, CONTIGS_NAME, HIST_NAME, BED_NAME), texts + (bed,))
        finish("motif_shift", TIMINGS, t1 - t0, time.perf_counter() - t1, label="statistics and text", candidates=len(known), background_candidates=len(bg_keys),
               bins=bins, min_delta_permille=permille, shifted_sites=None if records is None else int(len(records)))
    return 0
