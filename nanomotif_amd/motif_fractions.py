"""``nanomotif motif_fractions``: how the READ FRACTIONS n_modified / n_valid_cov are distributed over the sites of the motifs of a
``bin-motifs.tsv``.

``motif_sites`` / ``motif_coverage`` / ``motif_compare`` / ``motif_strands`` / ``motif_profile`` / ``motif_tracks`` read the thresholded
state planes: a site is mod (fraction >= 0.7), nomod (<= 0.3) or nocall, and the number behind the class is gone.  A motif that
``bin-motifs.tsv`` reports at "60 % methylated" is either a MIXTURE of fully methylated and unmethylated sites (an ON/OFF subpopulation, a
chimeric bin, a second overlapping motif) or has EVERY site partially methylated (a phase-variable methyltransferase, a caller that
under-calls in this context); the histogram tells the two apart, shows whether the nocall sites pile up just inside the thresholds, and
whether the thresholds suit the pileup at all.  The reference has nothing here.

Definitions (include/nmscan.h, nm_motif_fractions_count).  The pileup becomes READ STATISTICS (``loading.load_readstats_engine``): a record
is kept when ``n_valid_cov >= --min_valid_read_coverage`` and ``n_valid_cov / (n_valid_cov + n_diff) >= --min_valid_cov_to_diff_fraction``.
A candidate is (bin, motif, mod_position); its occurrences are those of ``motif_sites`` (the stripped motif on '+', its reverse complement
on '-'); a SITE is an occurrence whose modified base carries a kept record of the motif's mod type on the occurrence's strand.  With
``--bins`` = B a site falls in bin min(B - 1, n_modified * B // n_valid_cov): bin k is [k / B, (k + 1) / B), fraction 1 is in the last bin;
integers only, the device and the host agree by construction.  The bin's background — every occurrence of the mod type's canonical base,
the one-letter candidate, under the same coverage — rides in the same engine call, one per (bin, mod type present among the candidates):
the coarse fractions of low coverage show there as well.

Statistics, all from a histogram h summed over the strands (and, for ``motif-fractions.tsv``, over the contigs), n = sum(h), plain numpy on
the host: ``mean_read_cov`` = sum_valid / n, ``weighted_mean`` = sum_mod / sum_valid, the quantiles ``q10 q25 q50 q75 q90`` = the lower edge
k / B of the smallest bin with cum(k) >= max(1, (pct n + 99) // 100).  ``--methylation_threshold_low`` / ``_high`` snap to bin edges,
k = floor(x B + 0.5) with 0 < k_low <= k_high < B required: ``share_low`` is over the bins below k_low, ``share_high`` over the bins from
k_high, ``share_mid`` the rest.  ``flag``, in float64 on the counts c_low, c_mid, c_high with t = ``--minor_share``: ``few_sites`` if
n < ``--min_sites``; else ``methylated`` if c_high >= (1 - t) n; else ``unmethylated`` if c_low >= (1 - t) n; else ``bimodal`` if c_low >= t n
and c_high >= t n and c_mid < min(c_low, c_high); else ``partial``.  The zone rule, its defaults (20 sites, t = 0.1) and the quantile
convention are design choices of this command, like ``motif_tracks``' ``--min_gain``; no likelihood stands behind them.

Files (tab-separated, header line; candidates in file order, contigs in bin order):
  ``motif-fractions.tsv``          per candidate: the statistics, the sites per strand, and the bin's background (``bg_*``)
  ``motif-fractions-contigs.tsv``  per (candidate, contig that holds an occurrence): the counts, the shares, ``q50`` and ``flag``
  ``motif-fractions-hist.tsv``     long form: per background and candidate, strand and bin the number of sites
"""
from __future__ import annotations

import logging as log
import os
import time

import numpy as np

from . import fasta
from .engine import FRACTIONS_EXTRA, FRACTIONS_MAX_BINS, FRACTIONS_MIN_BINS
from .export_run import (READ_FILTER_SUFFIX, background_candidates, background_keys, closing, finish, open_readstats_run, parse_int_in,
                         readstats_mod_types, share_text, split_known, table_text, write_texts)
from .motif import MOD_TYPE_TO_CANONICAL

SUMMARY_NAME = "motif-fractions.tsv"
CONTIGS_NAME = "motif-fractions-contigs.tsv"
HIST_NAME = "motif-fractions-hist.tsv"
KEY_COLUMNS = ["bin", "motif", "mod_type", "mod_position"]
QUANTILES = (10, 25, 50, 75, 90)
SUMMARY_HEADER = KEY_COLUMNS + ["n_occurrences", "n_sites", "mean_read_cov", "weighted_mean"] + ["q%d" % q for q in QUANTILES] + [
    "share_low", "share_mid", "share_high", "low_edge", "high_edge", "flag", "n_sites_fwd", "n_sites_rev", "bg_n_sites", "bg_weighted_mean",
    "bg_share_low", "bg_share_mid", "bg_share_high"]
CONTIGS_HEADER = ["bin", "contig", "motif", "mod_type", "mod_position", "n_occurrences", "n_sites", "mean_read_cov", "weighted_mean", "share_low",
                  "share_mid", "share_high", "q50", "flag"]
HIST_HEADER = KEY_COLUMNS + ["background", "strand", "bin_index", "lower", "upper", "n_sites"]
FLAGS = ("few_sites", "methylated", "unmethylated", "bimodal", "partial")
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_fractions.json)


def parse_bins(value) -> int:
    """``--bins``: 2..64; ValueError otherwise."""
    return parse_int_in("--bins", value, FRACTIONS_MIN_BINS, FRACTIONS_MAX_BINS, what=f"a number in [{FRACTIONS_MIN_BINS}, {FRACTIONS_MAX_BINS}]")


def site_bin(n_modified: int, n_valid_cov: int, bins: int) -> int:
    """The bin of a site: min(bins - 1, n_modified * bins // n_valid_cov) — the rule of nm_motif_fractions_count, in integers."""
    return min(int(bins) - 1, int(n_modified) * int(bins) // int(n_valid_cov))


def snap_edges(low: float, high: float, bins: int):
    """(k_low, k_high): the thresholds snapped to bin edges, k = floor(x bins + 0.5); ValueError unless 0 < k_low <= k_high < bins."""
    k_low, k_high = (int(np.floor(float(x) * bins + 0.5)) for x in (low, high))
    if not 0 < k_low <= k_high < bins:
        raise ValueError(f"--methylation_threshold_low {low} / --methylation_threshold_high {high} snap to the bin edges {k_low} / {k_high} of "
                         f"{bins}: 0 < low edge <= high edge < {bins} is required")
    return k_low, k_high


def quantile_edge(hist, pct: int):
    """The lower edge k / B of the smallest bin with cum(k) >= max(1, (pct n + 99) // 100); None for an empty histogram."""
    h = np.asarray(hist, dtype=np.int64)
    n = int(h.sum())
    if n == 0:
        return None
    need = max(1, (int(pct) * n + 99) // 100)
    return int(np.searchsorted(np.cumsum(h), need)) / len(h)


def zone_counts(hist, k_low: int, k_high: int):
    """(c_low, c_mid, c_high) of a histogram: the bins below k_low, the bins in between, the bins from k_high."""
    h = np.asarray(hist, dtype=np.int64)
    return int(h[:k_low].sum()), int(h[k_low:k_high].sum()), int(h[k_high:].sum())


def flag_of(hist, k_low: int, k_high: int, min_sites: int, minor_share: float) -> str:
    c_low, c_mid, c_high = (float(x) for x in zone_counts(hist, k_low, k_high))
    n, t = c_low + c_mid + c_high, float(minor_share)
    if n < float(min_sites):
        return "few_sites"
    if c_high >= (1.0 - t) * n:
        return "methylated"
    if c_low >= (1.0 - t) * n:
        return "unmethylated"
    if c_low >= t * n and c_high >= t * n and c_mid < min(c_low, c_high):
        return "bimodal"
    return "partial"


def _edge(x) -> str:
    return "" if x is None else "%.6f" % x


class Stats:
    """The statistics of one table uint64[..., 2, B + 3] (a candidate's rows, or one of them) summed over everything but the last axis."""

    def __init__(self, table, bins: int, k_low: int, k_high: int, min_sites: int, minor_share: float):
        t = np.asarray(table, dtype=np.uint64).astype(np.int64).reshape(-1, 2, bins + FRACTIONS_EXTRA)
        per_strand = t.sum(axis=0)
        both = per_strand.sum(axis=0)
        self.hist = both[:bins]
        self.n_occurrences, self.sum_valid, self.sum_mod = (int(x) for x in both[bins:])
        self.n_sites = int(self.hist.sum())
        self.n_fwd, self.n_rev = (int(per_strand[s, :bins].sum()) for s in (0, 1))
        self.zones = zone_counts(self.hist, k_low, k_high)
        self.flag = flag_of(self.hist, k_low, k_high, min_sites, minor_share)
        self.quantiles = [quantile_edge(self.hist, q) for q in QUANTILES]

    def head(self):
        return [self.n_occurrences, self.n_sites, share_text(self.sum_valid, self.n_sites), share_text(self.sum_mod, self.sum_valid)]

    def shares(self):
        return [share_text(z, self.n_sites) for z in self.zones]


def hist_rows(key, background: int, table, bins: int) -> list:
    per_strand = np.asarray(table, dtype=np.uint64).astype(np.int64).reshape(-1, 2, bins + FRACTIONS_EXTRA).sum(axis=0)
    return [key + [background, "+-"[s], k, "%.6f" % (k / bins), "%.6f" % ((k + 1) / bins), int(per_strand[s, k])] for s in (0, 1) for k in range(bins)]


def candidate_rows(cand, names, table, bg_table, bins: int, k_low: int, k_high: int, min_sites: int, minor_share: float):
    """The rows of one candidate for (motif-fractions.tsv, motif-fractions-contigs.tsv, motif-fractions-hist.tsv).  ``names`` / ``table``:
    its item of ``ScanEngine.motif_fractions``; ``bg_table``: the table of the background of its (bin, mod type), or None."""
    args = (bins, k_low, k_high, min_sites, minor_share)
    key = [cand.bin, cand.motif, cand.mod_type, cand.mod_position]
    st = Stats(table, *args)
    if bg_table is None:
        bg_cols = ["", "", "", "", ""]
    else:
        bg = Stats(bg_table, *args)
        bg_cols = [bg.n_sites, share_text(bg.sum_mod, bg.sum_valid)] + bg.shares()
    summary = [key + st.head() + [_edge(q) for q in st.quantiles] + st.shares() + ["%.6f" % (k_low / bins), "%.6f" % (k_high / bins), st.flag,
                                                                                  st.n_fwd, st.n_rev] + bg_cols]
    contigs = []
    for i, name in enumerate(names):
        c = Stats(table[i], *args)
        if c.n_occurrences:
            contigs.append([cand.bin, fasta.original_name(name), cand.motif, cand.mod_type, cand.mod_position] + c.head() + c.shares() +
                           [_edge(c.quantiles[QUANTILES.index(50)]), c.flag])
    return summary, contigs, hist_rows(key, 0, table, bins)


def format_files(cands, items, backgrounds, bins: int, k_low: int, k_high: int, min_sites=20, minor_share=0.1):
    """(motif-fractions.tsv, motif-fractions-contigs.tsv, motif-fractions-hist.tsv) as text.  ``cands``: ``SiteCandidate`` in file order with
    their ``items`` = (contig names, uint64[n_contigs, 2, bins + 3]) of ``ScanEngine.motif_fractions``; ``backgrounds``: [((bin, mod
    type), table)] in ``background_keys`` order — their histograms open motif-fractions-hist.tsv."""
    rows = ([], [], [])
    bg_tables = dict(backgrounds)
    for (b, mt), table in backgrounds:
        rows[2].extend(hist_rows([b, MOD_TYPE_TO_CANONICAL[mt], mt, 0], 1, table, bins))
    for c, (names, table) in zip(cands, items):
        got = candidate_rows(c, names, table, bg_tables.get((c.bin, c.mod_type)), bins, k_low, k_high, min_sites, minor_share)
        for mine, new in zip(rows, got):
            mine += new
    return table_text(SUMMARY_HEADER, rows[0]), table_text(CONTIGS_HEADER, rows[1]), table_text(HIST_HEADER, rows[2])


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    bins = parse_bins(args.bins)
    try:
        k_low, k_high = snap_edges(args.methylation_threshold_low, args.methylation_threshold_high, bins)
    except ValueError as e:
        log.error(str(e))
        return 2
    eng, cands, status = open_readstats_run("motif_fractions", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        known = split_known(cands, eng, readstats_mod_types(eng), suffix=READ_FILTER_SUFFIX)
        bg_keys = background_keys(known)
        os.makedirs(args.out, exist_ok=True)
        # the background's one-letter candidates ride in the same engine call, ahead of the motifs that are read against them
        batch = background_candidates(bg_keys) + [c.engine_candidate() for c in known]
        t0 = time.perf_counter()
        items = [(names, table) for _, names, table in eng.motif_fractions(batch, bins=bins)]
        t1 = time.perf_counter()
        write_texts(args.out, (SUMMARY_NAME, CONTIGS_NAME, HIST_NAME),
                    format_files(known, items[len(bg_keys):], [(key, items[k][1]) for k, key in enumerate(bg_keys)], bins, k_low, k_high,
                                 int(args.min_sites), float(args.minor_share)))
        finish("motif_fractions", TIMINGS, t1 - t0, time.perf_counter() - t1, label="statistics and text", candidates=len(known),
               background_candidates=len(bg_keys), bins=bins)
    return 0
