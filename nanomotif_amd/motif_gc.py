"""``nanomotif motif_gc``: the methylation of the motifs of a ``bin-motifs.tsv`` STRATIFIED BY THE GC CONTENT around their sites.

The reference's known-issues page names two sources of false-positive motifs: calls of one modification type that bleed around a motif
of another (``motif_profile`` answers that one) and "high systematic 5mC noise in high GC% regions", for which it advises to check by
hand.  This command is that check.  A true methyltransferase motif is methylated whatever its surroundings; a noise motif — generic,
short, GC-rich — is methylated where the local GC is high and unmethylated where it is low, and the bin's background (every C, every A)
then shows the same curve.

Definition.  A candidate is (bin, motif, mod_type, mod_position); its occurrences and their states (mod / nomod / nocall) are those of
``motif_sites``.  The window of a site is the W = 2 ``--half`` + 1 contig positions centred on its modified base, g the number of G or
C among them (``ScanEngine.motif_gc``, nm_motif_gc_count: exact integer counts per g = 0..W, the host rebins).  A site whose window
leaves the contig or holds a letter that is not A, C, G or T has no g: an ``edge`` site, counted apart and in no bucket.  Bucket of a
site: min(B - 1, g * B // (W + 1)) in integers with B = min(``--gc_bins``, W + 1) — more buckets than values of g there cannot be, and
with that bound g = W falls in the last bucket.  ``gc_lower`` / ``gc_upper`` are the smallest and largest g of the bucket over W.

Every bin with a contig also gets its background, the one-letter candidates "every A" / "every C" per mod type of the pileup, in the
same engine calls.  The pileup goes through the ingest path of ``motif_discovery`` (``loading.load_engine``), so the counts summed over
g and edge reproduce the row's ``n_mod`` / ``n_nomod`` of ``bin-motifs.tsv``.

Files (tab-separated, header line; candidates in file order):
  ``motif-gc.tsv``           per (candidate, bucket): ``n_mod`` / ``n_nomod`` / ``n_nocall`` summed over strands and contigs, ``frac_mod`` =
                             n_mod / (n_mod + n_nomod) (empty when nothing is called) and ``bg_frac_mod``: the same bucket of the
                             bin's background in the candidate's mod type
  ``motif-gc-bins.tsv``      the bin's noise curve: the same per (bin with a contig, mod type) for the background, ``motif`` = the
                             canonical base, with the edge sites (``edge_mod`` / ``edge_nomod`` / ``edge_nocall``) and ``bin_gc``, the
                             G + C share of the bin's A, C, G and T
  ``motif-gc-contigs.tsv``   per (candidate, contig): ``contig_gc`` from the sequence, the six counts of ``motif_sites`` (edge sites
                             included), ``mean_gc_mod`` / ``mean_gc_nomod`` = the mean g / W at mod / nomod sites, ``edge_sites``
  ``motif-gc-summary.tsv``   per candidate, over the called sites (mod + nomod) that have a g: ``n_called``, ``frac_mod``,
                             ``mean_gc_mod`` / ``mean_gc_nomod``; ``trend_z`` / ``trend_p``: the Cochran-Armitage trend of mod against
                             the integer score g, pooled over contigs — T = sum mod_g (g - gbar), Var = p (1 - p) sum n_g (g - gbar)^2,
                             z = T / sqrt(Var), p = erfc(|z| / sqrt 2); ``trend_z_within``: T and Var summed per contig over the contigs
                             that have both outcomes, so that a contaminant contig of another GC and another methylation level does
                             not pass as a trend; ``frac_mod_low_gc`` / ``frac_mod_high_gc``: the lower and upper third of the
                             candidate's own called sites by g — whole values of g taken in ascending / descending order until a
                             third of the sites is reached, both empty when the two groups share a value —, ``delta`` = high - low;
                             ``bg_expected`` = sum n_g bg_frac_mod(g) / sum n_g over the g at which the background has called sites,
                             ``excess`` = frac_mod - bg_expected; ``flag`` = ``few_sites`` below ``--min_called`` called sites,
                             ``gc_dependent`` when |trend_z_within| >= ``--min_z`` and |delta| >= ``--min_delta``, else ``none``

``--min_z`` 5, ``--min_delta`` 0.2 and the thirds are design choices: they are pinned on hand-made tables
(``tests/test_motif_gc_host.py``), not on real data.
"""
from __future__ import annotations

import math
import os
import time

import numpy as np

from . import fasta
from .engine import GC_MAX_HALF
from .export_run import (background_candidates, bin_mod_keys, closing, finish, frac_text, open_run, parse_int_in, share_text, split_known, table_text,
                         write_texts)
from .loading import kept_mod_types
from .motif import MOD_TYPE_TO_CANONICAL

MAIN_NAME = "motif-gc.tsv"
BINS_NAME = "motif-gc-bins.tsv"
CONTIGS_NAME = "motif-gc-contigs.tsv"
SUMMARY_NAME = "motif-gc-summary.tsv"
KEY_COLUMNS = ["bin", "motif", "mod_type", "mod_position"]
BUCKET_COLUMNS = ["bucket", "gc_lower", "gc_upper", "n_mod", "n_nomod", "n_nocall", "frac_mod"]
MAIN_HEADER = KEY_COLUMNS + BUCKET_COLUMNS + ["bg_frac_mod"]
BINS_HEADER = KEY_COLUMNS + BUCKET_COLUMNS + ["edge_mod", "edge_nomod", "edge_nocall", "bin_gc"]
CONTIGS_HEADER = KEY_COLUMNS + ["contig", "contig_gc", "fwd_mod", "fwd_nomod", "fwd_nocall", "rev_mod", "rev_nomod", "rev_nocall", "mean_gc_mod", "mean_gc_nomod",
                                "edge_sites"]
SUMMARY_HEADER = KEY_COLUMNS + ["n_called", "frac_mod", "mean_gc_mod", "mean_gc_nomod", "trend_z", "trend_p", "trend_z_within", "frac_mod_low_gc",
                                "frac_mod_high_gc", "delta", "bg_expected", "excess", "flag"]
FLAGS = ("none", "gc_dependent", "few_sites")
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_gc.json)


def parse_half(value) -> int:
    """``--half``: an integer in 0..31 (the window is 2 half + 1 positions; one word of halo either side); ValueError otherwise."""
    return parse_int_in("--half", value, 0, GC_MAX_HALF)


def parse_gc_bins(value) -> int:
    """``--gc_bins``: an integer of at least 1; ValueError otherwise."""
    return parse_int_in("--gc_bins", value, 1)


def effective_bins(bins: int, width: int) -> int:
    """Buckets in use for a window of ``width`` positions: g takes width + 1 values, more buckets than that would stay empty."""
    return min(int(bins), int(width) + 1)


def bucket_of(g: int, width: int, bins: int) -> int:
    """The bucket of a site with g G or C among ``width`` positions, in integers: min(B - 1, g * B // (width + 1)), B = ``effective_bins``."""
    b = effective_bins(bins, width)
    return min(b - 1, int(g) * b // (int(width) + 1))


def bucket_bounds(width: int, bins: int) -> list:
    """Per bucket (smallest g, largest g) of the values of g that fall in it."""
    b = effective_bins(bins, width)
    out = [[None, None] for _ in range(b)]
    for g in range(int(width) + 1):
        k = bucket_of(g, width, bins)
        if out[k][0] is None:
            out[k][0] = g
        out[k][1] = g
    return [tuple(x) for x in out]


def rebin(per_g, bins: int) -> np.ndarray:
    """int64[..., W + 1] (per g) -> int64[..., B] (per bucket)."""
    per_g = np.asarray(per_g, dtype=np.int64)
    width = per_g.shape[-1] - 1
    out = np.zeros(per_g.shape[:-1] + (effective_bins(bins, width),), dtype=np.int64)
    for g in range(width + 1):
        out[..., bucket_of(g, width, bins)] += per_g[..., g]
    return out


def pooled(table) -> np.ndarray:
    """int64[n_contigs, 2 (occurrence strand), 3 (state), W + 2] of one candidate -> int64[3, W + 2] over strands and contigs."""
    return np.asarray(table, dtype=np.int64).sum(axis=(0, 1))


def mean_gc_text(per_g) -> str:
    """The mean g / W of the sites counted per g = 0..W; empty without a site."""
    per_g = np.asarray(per_g, dtype=np.int64)
    n, width = int(per_g.sum()), len(per_g) - 1
    return "%.6f" % (int((per_g * np.arange(width + 1)).sum()) / (n * width)) if n else ""


def trend_terms(mod_g, n_g):
    """(T, Var) of the Cochran-Armitage trend of ``mod_g`` methylated among ``n_g`` called sites against the score g:
    T = sum mod_g (g - gbar), Var = p (1 - p) sum n_g (g - gbar)^2; (0, 0) without a site."""
    mod_g, n_g = np.asarray(mod_g, dtype=np.float64), np.asarray(n_g, dtype=np.float64)
    n = n_g.sum()
    if n == 0:
        return 0.0, 0.0
    g = np.arange(len(n_g), dtype=np.float64)
    p = mod_g.sum() / n
    d = g - (n_g * g).sum() / n
    return float((mod_g * d).sum()), float(p * (1.0 - p) * (n_g * d * d).sum())


def z_of(t: float, var: float) -> float:
    return t / math.sqrt(var) if var > 0 else 0.0


def trend_z(mod_g, n_g) -> float:
    """The pooled trend statistic; 0 when it is undefined (one value of g, or one outcome only)."""
    return z_of(*trend_terms(mod_g, n_g))


def trend_p(z: float) -> float:
    """Two-sided normal tail of z."""
    return math.erfc(abs(z) / math.sqrt(2.0))


def trend_z_within(mod_cg, n_cg) -> float:
    """The trend with T and Var summed per contig ([n_contigs, W + 1] each), over the contigs that have both outcomes."""
    t_sum = v_sum = 0.0
    for mod_g, n_g in zip(np.asarray(mod_cg, dtype=np.int64), np.asarray(n_cg, dtype=np.int64)):
        m, n = int(mod_g.sum()), int(n_g.sum())
        if 0 < m < n:
            t, v = trend_terms(mod_g, n_g)
            t_sum += t
            v_sum += v
    return z_of(t_sum, v_sum)


def thirds(mod_g, n_g):
    """((mod, called) of the low-GC third, (mod, called) of the high-GC third) of the called sites by g: whole values of g in ascending /
    descending order until three times the group reaches the total.  None when the groups share a value of g or nothing is called."""
    mod_g, n_g = [int(x) for x in mod_g], [int(x) for x in n_g]
    total = sum(n_g)
    if total == 0:
        return None
    order = [g for g in range(len(n_g)) if n_g[g]]

    def take(values):
        used, m, n = [], 0, 0
        for g in values:
            used.append(g)
            m += mod_g[g]
            n += n_g[g]
            if 3 * n >= total:
                break
        return used, (m, n)
    low_g, low = take(order)
    high_g, high = take(order[::-1])
    if set(low_g) & set(high_g):
        return None
    return low, high


def bg_expected(n_g, bg_mod_g, bg_n_g):
    """sum n_g bg_frac_mod(g) / sum n_g over the g at which the background has called sites; None when there is none among the
    candidate's sites."""
    num, den = 0.0, 0
    for n, bm, bn in zip(n_g, bg_mod_g, bg_n_g):
        if int(bn) > 0 and int(n) > 0:
            num += int(n) * (int(bm) / int(bn))
            den += int(n)
    return num / den if den else None


def bucket_rows(key, cells, bins: int, tail=None, bg=None) -> list:
    """The rows of one candidate in motif-gc.tsv / motif-gc-bins.tsv (``cells`` = ``pooled`` of its table; ``bg``: the pooled cells of
    its background, whose frac_mod closes a row of motif-gc.tsv; ``tail``: columns appended as they are)."""
    width = cells.shape[-1] - 2
    per_bucket = rebin(cells[:, :width + 1], bins)
    bg_bucket = rebin(bg[:, :width + 1], bins) if bg is not None else None
    rows = []
    for k, (lo, hi) in enumerate(bucket_bounds(width, bins)):
        n = [int(v) for v in per_bucket[:, k]]
        row = list(key) + [k, "%.6f" % (lo / width), "%.6f" % (hi / width)] + n + [frac_text(n[0], n[1])]
        if bg_bucket is not None:
            row.append(frac_text(bg_bucket[0, k], bg_bucket[1, k]))
        rows.append(row + list(tail or []))
    return rows


def contig_rows(key, names, contig_gc, table) -> list:
    """The rows of one candidate in motif-gc-contigs.tsv (``table``: int64[n_contigs, 2, 3, W + 2]; ``contig_gc``: name -> text)."""
    table = np.asarray(table, dtype=np.int64)
    width = table.shape[-1] - 2
    rows = []
    for name, t in zip(names, table):
        both = t.sum(axis=0)
        rows.append(list(key) + [fasta.original_name(name), contig_gc.get(name, "")] + [int(v) for v in t.sum(axis=-1).reshape(6)] +
                    [mean_gc_text(both[0, :width + 1]), mean_gc_text(both[1, :width + 1]), int(both[:, width + 1].sum())])
    return rows


def summary_row(key, table, bg_cells, min_called=20, min_z=5.0, min_delta=0.2) -> list:
    """One row of motif-gc-summary.tsv (``table``: int64[n_contigs, 2, 3, W + 2] of the candidate; ``bg_cells``: ``pooled`` of its
    background, or None)."""
    table = np.asarray(table, dtype=np.int64)
    width = table.shape[-1] - 2
    per_contig = table.sum(axis=1)[:, :, :width + 1]                        # [n_contigs, 3, W + 1]
    mod_cg, n_cg = per_contig[:, 0], per_contig[:, 0] + per_contig[:, 1]
    mod_g, n_g = mod_cg.sum(axis=0), n_cg.sum(axis=0)
    n_mod, n_called = int(mod_g.sum()), int(n_g.sum())
    z = trend_z(mod_g, n_g)
    zw = trend_z_within(mod_cg, n_cg)
    cut = thirds(mod_g, n_g)
    low_text = high_text = delta_text = ""
    delta = None
    if cut is not None:
        (lm, ln), (hm, hn) = cut
        delta = hm / hn - lm / ln
        low_text, high_text, delta_text = "%.6f" % (lm / ln), "%.6f" % (hm / hn), "%.6f" % delta
    exp = bg_expected(n_g, bg_cells[0, :width + 1], bg_cells[0, :width + 1] + bg_cells[1, :width + 1]) if bg_cells is not None else None
    if n_called < int(min_called):
        flag = "few_sites"
    elif abs(zw) >= float(min_z) and delta is not None and abs(delta) >= float(min_delta):
        flag = "gc_dependent"
    else:
        flag = "none"
    return (list(key) + [n_called, frac_text(n_mod, n_called - n_mod), mean_gc_text(mod_g), mean_gc_text(n_g - mod_g), "%.3f" % z, "%.3e" % trend_p(z), "%.3f" % zw,
                         low_text, high_text, delta_text, "%.6f" % exp if exp is not None else "",
                         "%.6f" % (n_mod / n_called - exp) if exp is not None and n_called else "", flag])


def format_files(cands, results, bg_keys, bg_results, contig_gc, bin_gc, bins=8, min_called=20, min_z=5.0, min_delta=0.2):
    """(motif-gc.tsv, motif-gc-bins.tsv, motif-gc-contigs.tsv, motif-gc-summary.tsv) as text.  ``cands``: ``SiteCandidate`` in file
    order with ``results`` = their (contig names, int64[n_contigs, 2, 3, W + 2]) of ``ScanEngine.motif_gc``; ``bg_keys`` = [(bin, mod
    type)] with the same of the one-letter candidates; ``contig_gc`` / ``bin_gc``: name -> text of the G + C share."""
    bg_cells = {key: pooled(t) for key, (_, t) in zip(bg_keys, bg_results)}
    bins_rows, main_rows, contigs_rows, summary_rows = [], [], [], []
    for (b, mt), cells in bg_cells.items():
        width = cells.shape[-1] - 2
        bins_rows += bucket_rows([b, MOD_TYPE_TO_CANONICAL[mt], mt, 0], cells, bins, tail=[int(v) for v in cells[:, width + 1]] + [bin_gc.get(b, "")])
    for c, (names, t) in zip(cands, results):
        key = [c.bin, c.motif, c.mod_type, c.mod_position]
        bg = bg_cells.get((c.bin, c.mod_type))
        cells = pooled(t)
        main_rows += bucket_rows(key, cells, bins, bg=bg if bg is not None else np.zeros_like(cells))
        contigs_rows += contig_rows(key, names, contig_gc, t)
        summary_rows.append(summary_row(key, t, bg, min_called, min_z, min_delta))
    return (table_text(MAIN_HEADER, main_rows), table_text(BINS_HEADER, bins_rows), table_text(CONTIGS_HEADER, contigs_rows),
            table_text(SUMMARY_HEADER, summary_rows))


def sequence_gc(eng):
    """(contig name -> G + C share of its A, C, G and T as text, bin name -> the same over the bin's contigs), from the resident
    sequence."""
    counts = {x: eng.contig_base_counts(x, 0).astype(np.int64) for x in "ACGT"}
    gc, acgt = counts["C"] + counts["G"], counts["A"] + counts["C"] + counts["G"] + counts["T"]
    contig_gc = {name: share_text(gc[i], acgt[i]) for i, name in enumerate(eng.contig_names)}
    bin_gc = {}
    for b in eng.bin_index:
        ids = [eng.contig_index[n] for n in eng.bin_contigs(b)]
        bin_gc[b] = share_text(gc[ids].sum(), acgt[ids].sum()) if ids else ""
    return contig_gc, bin_gc


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    half, bins = parse_half(args.half), parse_gc_bins(args.gc_bins)
    eng, cands, status = open_run("motif_gc", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        mod_types = kept_mod_types(eng)
        known = split_known(cands, eng, mod_types)
        bg_keys = bin_mod_keys(eng, mod_types)
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        # the background's one-letter candidates ride in the same engine calls as the motifs
        results = list(eng.motif_gc([c.engine_candidate() for c in known] + background_candidates(bg_keys), half=half))
        contig_gc, bin_gc = sequence_gc(eng)
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        n = len(known)
        write_texts(args.out, (MAIN_NAME, BINS_NAME, CONTIGS_NAME, SUMMARY_NAME),
                    format_files(known, results[:n], bg_keys, results[n:], contig_gc, bin_gc, bins, int(args.min_called), float(args.min_z), float(args.min_delta)))
        finish("motif_gc", TIMINGS, t_eng, time.perf_counter() - t0, candidates=n, background_candidates=len(bg_keys), half=half, gc_bins=bins)
    return 0
