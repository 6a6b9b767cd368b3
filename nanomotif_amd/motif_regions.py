"""``nanomotif motif_regions``: the methylation of the motifs of a ``bin-motifs.tsv`` INSIDE THE REGIONS OF AN ANNOTATION — a prophage,
genomic-island or plasmid prediction (is recently acquired DNA unmethylated at the host's motifs?), a GFF3 (do the unmethylated sites sit
in front of genes?), a repeat or low-mappability mask (are the ``nocall`` and ``nomod`` sites just bad regions?).  What today takes
``motif_sites``, ``bedtools intersect`` and a hand-written group-by.

Definition.  A candidate is (bin, motif, mod_type, mod_position); its sites and their states (mod / nomod / nocall) are those of
``motif_sites`` (same ingest, ``loading.load_engine``).  ``--regions`` is a BED or GFF3 file (``regions.read_regions``); its classes —
BED column 4, GFF3 column 3, ordered and selected by ``--classes``, at most eight — become bit planes on the device
(``ScanEngine.upload_regions``).  A site is INSIDE class c when the position of its MODIFIED BASE lies in at least one interval of the
class: the motif's span does not matter, neither does the interval's strand; overlapping intervals of a class are a union.  Classes are
independent, a site may be inside several; it is ``outside`` when it is inside none.  ``--upstream N`` adds the class ``upstream``, the
N bases in front of every stranded interval.

Every bin with a contig also gets its background, the one-letter candidates "every A" / "every C" per mod type of the pileup, in the same
engine calls.

Files (tab-separated, header line; candidates in file order, classes in plane order, ``outside`` last):
  ``motif-regions.tsv``          per (candidate, class): ``n_mod`` / ``n_nomod`` / ``n_nocall`` over strands and contigs, ``frac_mod``;
                                 ``frac_mod_rest`` = the same over the candidate's sites NOT in the class, ``delta`` = frac_mod -
                                 frac_mod_rest; ``z`` = the pooled two-proportion statistic of mod among the called sites in the class
                                 against those not in it (0 when undefined), ``p`` = erfc(|z| / sqrt 2); ``bg_frac_mod``: the bin's
                                 background in that class and mod type; ``sites_per_kbp`` = the sites per 1000 positions of the class
                                 on the bin's contigs (empty for ``outside``); ``flag`` = ``few_sites`` when the class or the rest has
                                 fewer than ``--min_called`` called sites, ``depleted`` / ``enriched`` by the sign of delta when
                                 |z| >= ``--min_z`` and |delta| >= ``--min_delta``, else ``none``
  ``motif-regions-contigs.tsv``  per (candidate, contig, class): the six per-strand counts of ``motif_sites``
  ``motif-regions-bins.tsv``     per (bin with a contig, mod type, class): the background's counts and ``frac_mod``, ``covered_bp`` and
                                 its share of the bin's positions (both empty for ``outside``)
  ``region-sites.bed``           (``--region_sites``) the sites of ``--states`` inside the classes of ``--inside`` (class names and / or
                                 ``outside``; default every class): motif-sites.bed's eight columns, then the names of ALL classes the
                                 site is inside, comma-joined in plane order, or ``outside``
  ``motif-regions-intervals.tsv`` (``--intervals``) per (interval of a selected class, candidate of the bin of the interval's contig)
                                 with at least one site: class, interval name, bounds, the six counts.  This one is a HOST join —
                                 ``np.searchsorted`` per (candidate, contig) over the device's records of all states inside any class —
                                 not a device table; a device-side segmented count per interval is the open item (docs/NEXT.md).

``--min_z`` 5, ``--min_delta`` 0.2 and ``--min_called`` 20 are ``motif_gc``'s, reused as design choices: they are pinned on hand-made
tables (``tests/test_motif_regions_host.py``), not on real data.
"""
from __future__ import annotations

import logging as log
import math
import os
import time

import numpy as np

from . import fasta, regions
from .engine import REGION_OUTSIDE, SITE_MINUS, SITE_STATES, region_class_set
from .export_run import background_candidates, bin_mod_keys, closing, finish, frac_text, open_run, share_text, split_known, table_text, write_texts
from .loading import kept_mod_types
from .motif import MOD_TYPE_TO_CANONICAL
from .motif_gc import trend_p
from .motif_sites import parse_states

MAIN_NAME = "motif-regions.tsv"
CONTIGS_NAME = "motif-regions-contigs.tsv"
BINS_NAME = "motif-regions-bins.tsv"
SITES_NAME = "region-sites.bed"
INTERVALS_NAME = "motif-regions-intervals.tsv"
KEY_COLUMNS = ["bin", "motif", "mod_type", "mod_position"]
SIX = ["fwd_mod", "fwd_nomod", "fwd_nocall", "rev_mod", "rev_nomod", "rev_nocall"]
MAIN_HEADER = KEY_COLUMNS + ["class", "n_mod", "n_nomod", "n_nocall", "frac_mod", "frac_mod_rest", "delta", "z", "p", "bg_frac_mod", "sites_per_kbp", "flag"]
CONTIGS_HEADER = KEY_COLUMNS + ["contig", "class"] + SIX
BINS_HEADER = KEY_COLUMNS + ["class", "n_mod", "n_nomod", "n_nocall", "frac_mod", "covered_bp", "covered_share"]
INTERVALS_HEADER = ["class", "interval", "contig", "start", "end"] + KEY_COLUMNS + SIX
FLAGS = ("none", "depleted", "enriched", "few_sites")
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_regions.json)


def parse_inside(text) -> tuple:
    """``--inside A,outside``: class names and / or ``outside``, each once, in the order given; ValueError for an empty list.  Whether a
    name is a class of the annotation is known once the file is read."""
    asked = [s.strip() for s in str(text).split(",") if s.strip()]
    if not asked or len(set(asked)) != len(asked):
        raise ValueError(f"--inside takes a comma-separated list of distinct class names and / or {REGION_OUTSIDE}; got {text!r}")
    return tuple(asked)


def two_proportion_z(mod_in: int, called_in: int, mod_rest: int, called_rest: int) -> float:
    """The pooled two-proportion statistic of mod_in / called_in against mod_rest / called_rest; 0 when it is undefined (a group without
    a called site, or one outcome only)."""
    n1, n2 = int(called_in), int(called_rest)
    if n1 == 0 or n2 == 0:
        return 0.0
    p = (int(mod_in) + int(mod_rest)) / (n1 + n2)
    var = p * (1.0 - p) * (1.0 / n1 + 1.0 / n2)
    return (int(mod_in) / n1 - int(mod_rest) / n2) / math.sqrt(var) if var > 0 else 0.0


def flag_of(called_in: int, called_rest: int, z: float, delta, min_called=20, min_z=5.0, min_delta=0.2) -> str:
    if called_in < int(min_called) or called_rest < int(min_called):
        return "few_sites"
    if delta is not None and abs(z) >= float(min_z) and abs(delta) >= float(min_delta):
        return "depleted" if delta < 0 else "enriched"
    return "none"


def class_rows(key, class_names, cells, total, bg_cells, covered, min_called=20, min_z=5.0, min_delta=0.2) -> list:
    """The rows of one candidate in motif-regions.tsv.  ``cells``: int64[K + 1, 3] (mod, nomod, nocall per class, outside last) over
    strands and contigs; ``total``: int64[3] of all its sites; ``bg_cells``: the same cells of its background, or None; ``covered``:
    K covered positions on the bin's contigs; ``class_names``: the K names."""
    names = list(class_names)
    rows = []
    for c, name in enumerate(list(names) + [REGION_OUTSIDE]):
        m, u, n = (int(v) for v in cells[c])
        rm, ru = int(total[0]) - m, int(total[1]) - u
        frac, rest = frac_text(m, u), frac_text(rm, ru)
        delta = m / (m + u) - rm / (rm + ru) if m + u and rm + ru else None
        z = two_proportion_z(m, m + u, rm, rm + ru)
        per_kbp = "%.3f" % ((m + u + n) * 1000.0 / int(covered[c])) if c < len(names) and int(covered[c]) else ""
        rows.append(list(key) + [name, m, u, n, frac, rest, "%.6f" % delta if delta is not None else "", "%.3f" % z, "%.3e" % trend_p(z),
                                 frac_text(bg_cells[c][0], bg_cells[c][1]) if bg_cells is not None else "", per_kbp,
                                 flag_of(m + u, rm + ru, z, delta, min_called, min_z, min_delta)])
    return rows


def format_files(cands, results, totals, bg_keys, bg_results, class_names, covered, contig_len, min_called=20, min_z=5.0, min_delta=0.2):
    """(motif-regions.tsv, motif-regions-contigs.tsv, motif-regions-bins.tsv) as text.  ``cands``: ``SiteCandidate`` in file order with
    ``results`` = their (contig names, int64[n_contigs, K + 1, 2, 3]) of ``ScanEngine.motif_regions_counts`` and ``totals`` = their
    (contig names, int64[n_contigs, 6]) of ``motif_site_counts``; ``bg_keys`` = [(bin, mod type)] with ``bg_results``, the same tables of
    the one-letter candidates; ``covered``: contig name -> K covered positions; ``contig_len``: contig name -> length."""
    class_names = list(class_names)
    k = len(class_names)
    all_names = class_names + [REGION_OUTSIDE]
    bg_cells, bin_covered, bin_bp = {}, {}, {}
    bins_rows, main_rows, contigs_rows = [], [], []
    for (b, mt), (names, t) in zip(bg_keys, bg_results):
        cells = np.asarray(t, dtype=np.int64).reshape(-1, k + 1, 2, 3).sum(axis=(0, 2))
        bg_cells[(b, mt)] = cells
        bin_covered[b] = np.sum([np.asarray(covered[n], dtype=np.int64) for n in names], axis=0) if names else np.zeros(k, dtype=np.int64)
        bin_bp[b] = sum(int(contig_len[n]) for n in names)
        for c, name in enumerate(all_names):
            m, u, n = (int(v) for v in cells[c])
            inside = c < k
            bins_rows.append([b, MOD_TYPE_TO_CANONICAL[mt], mt, 0, name, m, u, n, frac_text(m, u), int(bin_covered[b][c]) if inside else "",
                              share_text(bin_covered[b][c], bin_bp[b]) if inside else ""])
    for cand, (names, t), (_, six) in zip(cands, results, totals):
        key = [cand.bin, cand.motif, cand.mod_type, cand.mod_position]
        t = np.asarray(t, dtype=np.int64).reshape(-1, k + 1, 2, 3)
        total = np.asarray(six, dtype=np.int64).reshape(-1, 2, 3).sum(axis=(0, 1))
        cov = bin_covered.get(cand.bin)
        if cov is None:
            cov = np.sum([np.asarray(covered[n], dtype=np.int64) for n in names], axis=0) if names else np.zeros(k, dtype=np.int64)
        main_rows += class_rows(key, class_names, t.sum(axis=(0, 2)), total, bg_cells.get((cand.bin, cand.mod_type)), cov, min_called, min_z, min_delta)
        for name, row in zip(names, t):
            for c, cls in enumerate(all_names):
                contigs_rows.append(key + [fasta.original_name(name), cls] + [int(v) for v in row[c].reshape(6)])
    return table_text(MAIN_HEADER, main_rows), table_text(CONTIGS_HEADER, contigs_rows), table_text(BINS_HEADER, bins_rows)


def class_text(mask: int, class_names) -> str:
    """The names of the classes of a record's mask, comma-joined in plane order; ``outside`` for 0."""
    return ",".join(n for c, n in enumerate(class_names) if mask >> c & 1) or REGION_OUTSIDE


def format_sites(records, cands, contig_names, class_names) -> str:
    """The lines of region-sites.bed for ``records`` (``engine.REGION_DTYPE``; ``candidate`` indexes ``cands``): contig, start, end,
    motif_modtype_modposition, 0, strand, state, bin, classes."""
    texts = [class_text(m, class_names) for m in range(1 << len(class_names))]
    out = []
    for cand, contig, pos, code, mask in zip(records["candidate"].tolist(), records["contig"].tolist(), records["pos"].tolist(), records["code"].tolist(),
                                             records["classes"].tolist()):
        c = cands[cand]
        out.append(f"{contig_names[contig]}\t{pos}\t{pos + 1}\t{c.name}\t0\t{'-' if code & SITE_MINUS else '+'}\t{SITE_STATES[code & 3]}\t{c.bin}\t{texts[mask]}\n")
    return "".join(out)


def interval_rows(region_set, records, cands, contig_names) -> list:
    """The rows of motif-regions-intervals.tsv: a host join of the intervals of ``region_set`` (``regions.RegionSet``) with ``records``
    (``engine.REGION_DTYPE`` in the engine's order: candidate, contig, ascending position) — per (candidate, contig) one
    ``np.searchsorted`` of the intervals' bounds in the positions.  Rows in interval order, then candidate order; pairs without a site
    are left out."""
    by_contig = {}
    for i, contig in enumerate(region_set.contig.tolist()):
        by_contig.setdefault(contig, []).append(i)
    found = {}
    cand_col, contig_col = records["candidate"], records["contig"]
    edges = np.flatnonzero(np.diff(cand_col.astype(np.int64) * (len(contig_names) + 1) + contig_col)) + 1 if len(records) else np.zeros(0, dtype=np.int64)
    bounds = [0] + edges.tolist() + ([len(records)] if len(records) else [])
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        j, contig = int(cand_col[lo]), int(contig_col[lo])
        idx = by_contig.get(contig)
        if not idx:
            continue
        pos = records["pos"][lo:hi].astype(np.int64)
        code = records["code"][lo:hi]
        cell = (code >> 2).astype(np.int64) * 3 + (code & 3)
        first = np.searchsorted(pos, region_set.start[idx].astype(np.int64), side="left")
        last = np.searchsorted(pos, region_set.end[idx].astype(np.int64), side="left")
        for i, a, b in zip(idx, first.tolist(), last.tolist()):
            if b > a:
                found[(i, j)] = np.bincount(cell[a:b], minlength=6)[:6]
    rows = []
    for (i, j), six in sorted(found.items()):
        c = cands[j]
        rows.append([region_set.class_names[int(region_set.cls[i])], region_set.names[i], fasta.original_name(contig_names[int(region_set.contig[i])]),
                     int(region_set.start[i]), int(region_set.end[i]), c.bin, c.motif, c.mod_type, c.mod_position] + [int(v) for v in six])
    return rows


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    states = args.states if isinstance(args.states, tuple) else parse_states(args.states)
    upstream = int(args.upstream or 0)
    # the command's own refusals come before anything is loaded: the annotation's rows, its classes and --inside need no contig
    try:
        rows = regions.parse_rows(args.regions)
        inside = region_class_set(regions.select_classes(rows, args.classes, upstream), args.inside)
    except (ValueError, OSError) as e:
        log.error(f"motif_regions: {e}")
        return 2
    eng, cands, status = open_run("motif_regions", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        mod_types = kept_mod_types(eng)
        known = split_known(cands, eng, mod_types)
        bg_keys = bin_mod_keys(eng, mod_types)
        try:                                                              # (an interval past its contig's end shows only now)
            rs = regions.read_regions(args.regions, eng.contig_index, eng.contig_lengths, args.classes, upstream, rows=rows)
        except ValueError as e:
            log.error(f"motif_regions: {e}")
            return 2
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        eng.upload_regions(rs.contig, rs.start, rs.end, rs.cls, rs.class_names)
        # the background's one-letter candidates ride in the same engine calls as the motifs
        engine_cands = [c.engine_candidate() for c in known] + background_candidates(bg_keys)
        results = list(eng.motif_regions_counts(engine_cands))
        totals = eng.motif_site_counts(engine_cands)
        cov = eng.region_covered()
        covered = {name: cov[:, i] for i, name in enumerate(eng.contig_names)}
        contig_len = {name: int(eng.contig_lengths[i]) for i, name in enumerate(eng.contig_names)}
        n = len(known)
        contig_names = [fasta.original_name(x) for x in eng.contig_names]
        sites_text = intervals_text = None
        if args.region_sites:
            picked = [s for s in rs.class_names if inside[0] >> rs.class_names.index(s) & 1] + ([REGION_OUTSIDE] if inside[1] else [])
            batches = eng.motif_regions_sites(engine_cands[:n], states=states, classes=picked)
            sites_text = "".join(format_sites(sb.records, known, contig_names, rs.class_names) for sb in batches)
        if args.intervals:
            rec = [sb.records for sb in eng.motif_regions_sites(engine_cands[:n])]
            rec = np.concatenate(rec) if rec else np.zeros(0, dtype=[("candidate", "u4"), ("contig", "u4"), ("pos", "u4"), ("code", "u1"), ("classes", "u1")])
            intervals_text = table_text(INTERVALS_HEADER, interval_rows(rs, rec, known, eng.contig_names))
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        texts = format_files(known, results[:n], totals[:n], bg_keys, results[n:], rs.class_names, covered, contig_len, int(args.min_called), float(args.min_z),
                             float(args.min_delta))
        write_texts(args.out, (MAIN_NAME, CONTIGS_NAME, BINS_NAME, SITES_NAME, INTERVALS_NAME), texts + (sites_text, intervals_text))
        finish("motif_regions", TIMINGS, t_eng, time.perf_counter() - t0, candidates=n, background_candidates=len(bg_keys), classes=len(rs.class_names),
               intervals=len(rs), dropped_intervals=rs.dropped)
    return 0
