"""``nanomotif motif_pileup``: the read counts under every site of the motifs of a ``bin-motifs.tsv`` — for each occurrence the
``n_valid_cov`` and ``n_modified`` of the pileup record under its modified base.

``motif_sites`` says where a motif occurs and in which thresholded state; ``motif_fractions`` reduces the sites' read fractions to a
histogram.  This command writes the values themselves: the table behind per-site plots, a differential test of one's own, a genome-browser
track, or a look at the sites near the 0.3 / 0.7 thresholds — what ``modkit motif bed`` + ``bedtools intersect`` against the bedMethyl file
yield.  The reference has nothing here.

Definitions (include/nmscan.h, nm_motif_pileup_sites) are those of ``motif_fractions``.  The pileup becomes READ STATISTICS
(``loading.load_readstats_engine``): a record is kept when ``n_valid_cov >= --min_valid_read_coverage`` and ``n_valid_cov / (n_valid_cov +
n_diff) >= --min_valid_cov_to_diff_fraction``.  A candidate is (bin, motif, mod_position); its occurrences are those of ``motif_sites`` (the
stripped motif on '+', its reverse complement on '-'); a SITE is an occurrence whose modified base carries a kept record of the motif's mod
type on the occurrence's strand, a BARE occurrence one without.

Files:
  ``motif-pileup.bed``          no header; contig, start, end, motif_modtype_modposition, n_valid_cov, strand, n_modified,
                                percent_modified, bin — one line per site, with ``--all_occurrences`` also per bare occurrence (0, 0 and an
                                empty percentage).  ``percent_modified`` = 100 n_modified / n_valid_cov with two decimals, rounded half up in
                                integers (``percent_text``).  Candidates in ``bin-motifs.tsv`` order, within a candidate contigs in bin
                                order, ascending position, '+' before '-'.
  ``motif-pileup-summary.tsv``  per (bin, contig that holds an occurrence, motif): occurrences and sites per strand, the sums of
                                n_valid_cov and n_modified over the sites, ``mean_read_cov`` = sum_valid_cov / n_sites and
                                ``weighted_mean`` = sum_modified / sum_valid_cov — the numbers of ``motif-fractions-contigs.tsv``.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from . import _lib, fasta
from .export_run import READ_FILTER_SUFFIX, closing, finish, open_readstats_run, readstats_mod_types, share_text, split_known, table_text, write_texts

BED_NAME = "motif-pileup.bed"
SUMMARY_NAME = "motif-pileup-summary.tsv"
SUMMARY_HEADER = ["bin", "contig", "motif", "mod_type", "mod_position", "n_occurrences_fwd", "n_occurrences_rev", "n_sites_fwd", "n_sites_rev",
                  "sum_valid_cov", "sum_modified", "mean_read_cov", "weighted_mean"]
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_pileup.json)


def percent_text(n_modified: int, n_valid_cov: int) -> str:
    """100 n_modified / n_valid_cov with two decimals, rounded half up in integers — the rule of nm_motif_pileup_text."""
    h = (20000 * int(n_modified) + int(n_valid_cov)) // (2 * int(n_valid_cov))
    return "%d.%02d" % (h // 100, h % 100)


def format_pileup(contig, pos, code, n_valid, n_mod, seg_begin, seg_names, seg_bins, contig_names) -> bytes:
    """The lines of motif-pileup.bed for records (contig, pos, code, n_valid, n_mod) cut into runs [seg_begin[s], seg_begin[s + 1]) that
    share a name and a bin (nm_motif_pileup_text: native, on up to NM_POST_THREADS threads)."""
    text = _lib.load().nm_motif_pileup_text
    n = len(contig)
    if n == 0:
        return b""
    contig, pos, n_valid, n_mod = (np.ascontiguousarray(a, dtype=np.uint32) for a in (contig, pos, n_valid, n_mod))
    code = np.ascontiguousarray(code, dtype=np.uint8)
    seg_begin = np.ascontiguousarray(seg_begin, dtype=np.uint64)
    parts = [x.encode() for pair in zip(seg_names, seg_bins) for x in pair]
    seg_off = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in parts], out=seg_off[1:])
    cparts = [x.encode() for x in contig_names]
    c_off = np.zeros(len(cparts) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in cparts], out=c_off[1:])
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    args = (n, p(contig, C.c_uint32), p(pos, C.c_uint32), p(code, C.c_uint8), p(n_valid, C.c_uint32), p(n_mod, C.c_uint32), len(seg_names),
            p(seg_begin, C.c_uint64), b"".join(parts), p(seg_off, C.c_uint64), len(cparts), b"".join(cparts), p(c_off, C.c_uint64))
    size = C.c_uint64(0)
    _lib.check(text(*args, None, 0, C.byref(size)))
    buf = np.empty(size.value, dtype=np.uint8)
    _lib.check(text(*args, buf.ctypes.data_as(C.c_void_p), size.value, C.byref(size)))
    return buf.tobytes()


def format_summary(summary) -> str:
    """motif-pileup-summary.tsv as text.  ``summary``: [(candidate, contig name, int64[4] = fwd site, fwd bare, rev site, rev bare,
    sum_valid_cov, sum_modified)] in candidate, contig order; a contig without an occurrence has no row."""
    rows = []
    for c, contig, four, sum_valid, sum_mod in summary:
        fs, fb, rs, rb = (int(x) for x in four)
        if fs + fb + rs + rb:
            rows.append([c.bin, fasta.original_name(contig), c.motif, c.mod_type, c.mod_position, fs + fb, rs + rb, fs, rs, int(sum_valid), int(sum_mod),
                         share_text(sum_valid, fs + rs), share_text(sum_mod, sum_valid)])
    return table_text(SUMMARY_HEADER, rows)


def export_pileup(eng, cands: list, all_occurrences: bool, bed_file, max_records=None):
    """Write the records of ``cands`` (SiteCandidate) to the open binary file ``bed_file``; returns the summary rows ``format_summary``
    takes and the seconds spent in (engine, text)."""
    select = ("site", "bare") if all_occurrences else ("site",)
    contig_names = [fasta.original_name(n) for n in eng.contig_names]
    n_contigs = len(eng.contig_names)
    counts = []                                                              # per candidate (contig names, int64[n, 4])
    sums = {}                                                                # candidate * n_contigs + engine contig -> [sum_valid, sum_mod]
    t_eng = t_text = 0.0
    t0 = time.perf_counter()
    for sb in eng.motif_pileup([c.engine_candidate() for c in cands], select=select, max_records=max_records):
        t1 = time.perf_counter()
        t_eng += t1 - t0
        group = cands[sb.first_candidate:sb.first_candidate + sb.n_candidates]
        if sb.counts is not None:
            counts += sb.counts
        rec = sb.records
        if len(rec):
            seg_begin = np.searchsorted(rec["candidate"], np.arange(sb.first_candidate, sb.first_candidate + sb.n_candidates + 1))
            bed_file.write(format_pileup(rec["contig"], rec["pos"], rec["code"], rec["n_valid"], rec["n_mod"], seg_begin, [c.name for c in group],
                                         [c.bin for c in group], contig_names))
            # (the records are sorted by candidate and contig: a window holds few distinct keys; the sums stay below 2^53)
            keys, inverse = np.unique(rec["candidate"].astype(np.int64) * n_contigs + rec["contig"], return_inverse=True)
            valid, mod = (np.bincount(inverse, weights=rec[f].astype(np.float64), minlength=len(keys)).astype(np.int64) for f in ("n_valid", "n_mod"))
            for key, v, m in zip(keys.tolist(), valid.tolist(), mod.tolist()):
                held = sums.setdefault(key, [0, 0])
                held[0] += v
                held[1] += m
        t0 = time.perf_counter()
        t_text += t0 - t1
    t_eng += time.perf_counter() - t0
    index = {n: i for i, n in enumerate(eng.contig_names)}
    summary = [(c, name, table[i], *sums.get(k * n_contigs + index[name], (0, 0)))
               for k, (c, (names, table)) in enumerate(zip(cands, counts)) for i, name in enumerate(names)]
    return summary, (t_eng, t_text)


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    eng, cands, status = open_readstats_run("motif_pileup", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        known = split_known(cands, eng, readstats_mod_types(eng), suffix=READ_FILTER_SUFFIX)
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, BED_NAME), "wb") as f:
            summary, (t_eng, t_text) = export_pileup(eng, known, bool(args.all_occurrences), f)
        t1 = time.perf_counter()
        write_texts(args.out, (SUMMARY_NAME,), (format_summary(summary),))
        finish("motif_pileup", TIMINGS, t_eng, t_text + time.perf_counter() - t1, candidates=len(known))
    return 0
