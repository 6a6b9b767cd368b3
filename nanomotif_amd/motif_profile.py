"""``nanomotif motif_profile``: the methylation of every position AROUND the sites of the motifs of a ``bin-motifs.tsv``, on both strands
and under every mod type of the pileup.

``motif_sites`` / ``motif_coverage`` / ``motif_compare`` / ``motif_strands`` read a motif's own modified base (``motif_strands``: plus one
partner position).  Most of the doubt about a discovered motif sits next to that base: is ``mod_position`` the right one (discovery
sometimes reports the neighbour of the true position), is a weak call bleed from the true site one base on, is the site in fact another
mod type's (``m`` and ``21839`` are both called on C).  The answer is the state of the neighbours of every occurrence, which lives only in
the device planes (``ScanEngine.motif_profile``, nm_motif_profile_count).

Definition.  A candidate is (bin, motif, mod_position); its occurrences are those of ``motif_sites``: the stripped motif on '+', its
reverse complement on '-'.  An occurrence has its modified base at '+' coordinate p on occurrence strand s.  For an offset o in the
motif's reading direction, -R <= o <= R (``--radius``), and a relative strand (``same``: the occurrence's strand, ``opposite``: the other
one) the probed position is p + o for an occurrence on '+' and p - o for one on '-'.  Under a target mod type with canonical base B the
probe is ``mod`` (methylated; a position called both ways is methylated), ``nomod`` (unmethylated), ``nocall`` (neither, inside the
contig, and the contig's letter read on the probed strand is B) or ``other`` (another letter, N, outside the contig).  The four classes
sum to ``n_sites``.  With the candidate's own mod type as target, (same, 0) is the motif's row of ``motif_sites`` and (opposite, d) gives
the partner marginals of ``motif_strands`` for the partner offset d.

The pileup goes through the ingest path of ``motif_discovery`` (``loading.load_engine``), so (own target, same, 0) reproduces the row's
``n_mod`` / ``n_nomod`` of ``bin-motifs.tsv``.

Files (tab-separated, header line; candidates in file order, targets in slot order, ``same`` before ``opposite``, ascending offset):
  ``motif-profile.tsv``          per (candidate, target, relative strand, offset): the four counts pooled over both occurrence strands and
                                 all contigs of the bin, ``frac_mod`` = n_mod / (n_mod + n_nomod) (empty when nothing is called) and
                                 ``bg_frac_mod``, the same cell of the bin's background
  ``motif-profile-bins.tsv``     the background, one block per (bin with a contig, canonical base present among the targets): the profile
                                 of the one-letter candidate — every occurrence of that base — under every target of that base, same
                                 columns (``motif`` = the base, ``mod_type`` = the target, ``bg_frac_mod`` = its own ``frac_mod``).  Its
                                 ``opposite`` rows are the state of any two canonical bases d apart on opposite strands, for every d at once
  ``motif-profile-summary.tsv``  per candidate: ``own_frac_mod`` / ``own_called`` at (own target, same, 0); among all OTHER cells with at
                                 least ``--min_called`` called sites and a background with a called site, the one with the highest
                                 ``frac_mod - bg_frac_mod`` (ties: lowest target index, same before opposite, smallest |offset|, negative
                                 before positive) as ``best_*``, empty when no cell qualifies; ``flag`` = ``shifted`` when that cell is
                                 (own target, same, o != 0) and its frac_mod exceeds own_frac_mod, ``other_mod_type`` when it is (another
                                 target, same, 0) and exceeds it, else ``none``.  An own cell without a called site is exceeded by any.
"""
from __future__ import annotations

import logging as log
import os
import time

import numpy as np

from .engine import PROFILE_MAX_RADIUS, ScanEngine
from .export_run import closing, finish, frac_text, open_run, parse_int_in, resident_bins, table_text, write_texts
from .loading import kept_mod_types
from .motif import MOD_TYPE_TO_CANONICAL, Motif
from .pileup import MOD_TYPES

MAIN_NAME = "motif-profile.tsv"
BINS_NAME = "motif-profile-bins.tsv"
SUMMARY_NAME = "motif-profile-summary.tsv"
STRANDS = ("same", "opposite")
KEY_COLUMNS = ["bin", "motif", "mod_type", "mod_position"]
MAIN_HEADER = KEY_COLUMNS + ["target", "strand", "offset", "n_sites", "n_mod", "n_nomod", "n_nocall", "n_other", "frac_mod", "bg_frac_mod"]
SUMMARY_HEADER = KEY_COLUMNS + ["own_frac_mod", "own_called", "best_target", "best_strand", "best_offset", "best_frac_mod", "best_bg_frac_mod", "best_called",
                                "flag"]
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_profile.json)


def parse_targets(text) -> tuple:
    """``--targets a,m`` -> the mod types in the order of ``pileup.MOD_TYPES``, each once; ValueError names what is none."""
    asked = [t.strip() for t in str(text).split(",") if t.strip()]
    bad = [t for t in asked if t not in MOD_TYPES]
    if bad or not asked:
        raise ValueError(f"--targets takes a comma-separated selection of {', '.join(MOD_TYPES)}; got {text!r}")
    return tuple(t for t in MOD_TYPES if t in asked)


def parse_radius(value) -> int:
    """``--radius``: an integer in 0..31 (one v_alignbit of two neighbouring words per offset); ValueError otherwise."""
    return parse_int_in("--radius", value, 0, PROFILE_MAX_RADIUS)


def pooled(table) -> np.ndarray:
    """int64[n_targets, W, 2 (occurrence strand), 2 (relative strand), 4] of one candidate -> int64[n_targets, 2 (relative strand), W, 4]
    over both occurrence strands: the row order of the files."""
    return np.asarray(table, dtype=np.int64).sum(axis=2).transpose(0, 2, 1, 3)


def background_keys(bins, targets) -> list:
    """[(bin, base)] of the background blocks: per bin the canonical bases of ``targets`` in the order they first appear."""
    bases = []
    for t in targets:
        if MOD_TYPE_TO_CANONICAL[t] not in bases:
            bases.append(MOD_TYPE_TO_CANONICAL[t])
    return [(b, base) for b in bins for base in bases]


def profile_rows(key, targets, n_sites: int, cells, bg_cells, only_base=None) -> list:
    """The rows of one candidate (``key``: its four key columns; ``cells`` = ``pooled`` of its table; ``bg_cells``: target index ->
    the background's int64[2, W, 4] of the candidate's bin, or None).  ``only_base``: write the targets of that canonical base only
    and name the target in the mod_type column (a background block)."""
    rows = []
    width = cells.shape[2]
    radius = (width - 1) // 2
    for ti, target in enumerate(targets):
        if only_base is not None and MOD_TYPE_TO_CANONICAL[target] != only_base:
            continue
        bg = bg_cells.get(ti)
        for r, strand in enumerate(STRANDS):
            for w in range(width):
                n = [int(x) for x in cells[ti, r, w]]
                k = list(key) if only_base is None else [key[0], key[1], target, key[3]]
                rows.append(k + [target, strand, w - radius, int(n_sites)] + n +
                            [frac_text(n[0], n[1]), frac_text(bg[r, w, 0], bg[r, w, 1]) if bg is not None else ""])
    return rows


def best_cell(targets, cells, bg_cells, own, min_called: int):
    """The cell of one candidate with the highest frac_mod - bg_frac_mod among those that are not ``own`` = (target index, 0, centre),
    hold at least ``min_called`` called sites and have a background with a called site: (target index, relative strand, offset index) or
    None.  Ties: lowest target index, same before opposite, smallest |offset|, negative before positive."""
    width = cells.shape[2]
    radius = (width - 1) // 2
    best, best_key = None, None
    for ti in range(len(targets)):
        bg = bg_cells.get(ti)
        if bg is None:
            continue
        for r in range(2):
            for w in range(width):
                if (ti, r, w) == own:
                    continue
                called = int(cells[ti, r, w, 0] + cells[ti, r, w, 1])
                bg_called = int(bg[r, w, 0] + bg[r, w, 1])
                if called < max(int(min_called), 1) or bg_called == 0:
                    continue
                excess = int(cells[ti, r, w, 0]) / called - int(bg[r, w, 0]) / bg_called
                o = w - radius
                key = (-excess, ti, r, abs(o), o)
                if best_key is None or key < best_key:
                    best, best_key = (ti, r, w), key
    return best


def summary_row(key, mod_type, targets, cells, bg_cells, min_called: int) -> list:
    """One row of motif-profile-summary.tsv."""
    width = cells.shape[2]
    radius = (width - 1) // 2
    own_t = targets.index(mod_type) if mod_type in targets else None
    own = (own_t, 0, radius) if own_t is not None else None
    own_mod, own_called = (int(cells[own][0]), int(cells[own][0] + cells[own][1])) if own is not None else (0, 0)
    row = list(key) + [frac_text(own_mod, own_called - own_mod) if own is not None else "", own_called if own is not None else ""]
    best = best_cell(targets, cells, bg_cells, own, min_called)
    if best is None:
        return row + [""] * 6 + ["none"]
    ti, r, w = best
    n_mod, called = int(cells[best][0]), int(cells[best][0] + cells[best][1])
    bg = bg_cells[ti]
    flag = "none"
    exceeds = own is not None and (own_called == 0 or n_mod * own_called > own_mod * called)       # integer comparison of the two shares
    if exceeds and r == 0:
        if ti == own_t and w != radius:
            flag = "shifted"
        elif ti != own_t and w == radius:
            flag = "other_mod_type"
    return row + [targets[ti], STRANDS[r], w - radius, frac_text(n_mod, called - n_mod), frac_text(bg[r, w, 0], bg[r, w, 1]), called, flag]


def format_files(cands, targets, sites, tables, bg_keys, bg_sites, bg_tables, min_called: int):
    """(motif-profile.tsv, motif-profile-bins.tsv, motif-profile-summary.tsv) as text.  ``cands``: ``SiteCandidate`` in file order with
    ``sites`` int64[n, 2] and ``tables`` int64[n, n_targets, W, 2, 2, 4] of ``ScanEngine.motif_profile``; ``bg_keys`` = [(bin, base)] with
    the same of the one-letter candidates."""
    targets = list(targets)
    bg_of = {}                                                            # bin -> {target index -> int64[2, W, 4]}
    bins_rows = []
    for (b, base), s, t in zip(bg_keys, bg_sites, bg_tables):
        cells = pooled(t)
        mine = {ti: cells[ti] for ti, target in enumerate(targets) if MOD_TYPE_TO_CANONICAL[target] == base}
        bg_of.setdefault(b, {}).update(mine)
        bins_rows += profile_rows([b, base, "", 0], targets, int(np.sum(s)), cells, mine, only_base=base)
    main_rows, summary_rows = [], []
    for c, s, t in zip(cands, sites, tables):
        cells = pooled(t)
        key = [c.bin, c.motif, c.mod_type, c.mod_position]
        bg_cells = bg_of.get(c.bin, {})
        main_rows += profile_rows(key, targets, int(np.sum(s)), cells, bg_cells)
        summary_rows.append(summary_row(key, c.mod_type, targets, cells, bg_cells, min_called))
    return table_text(MAIN_HEADER, main_rows), table_text(MAIN_HEADER, bins_rows), table_text(SUMMARY_HEADER, summary_rows)


def run_targets(eng: ScanEngine, asked) -> list:
    """The targets of a run in slot order: ``asked`` (``parse_targets``), or every mod type the pileup holds rows of; a mod type asked for
    that the pileup holds no rows of is left out with a warning."""
    have = kept_mod_types(eng)
    if asked is None:
        return have
    for t in asked:
        if t not in have:
            log.warning(f"--targets: the pileup holds no rows of mod type {t}; left out")
    return [t for t in have if t in asked]


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    radius = parse_radius(args.radius)
    asked = None if args.targets is None else args.targets if isinstance(args.targets, tuple) else parse_targets(args.targets)
    eng, cands, status = open_run("motif_profile", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        targets = run_targets(eng, asked)
        if not targets:
            log.error("motif_profile: the pileup holds no rows of any target mod type")
            return 2
        known = []          # this command's own rule, in one pass: a mod type outside the targets is kept (the targets are read under any motif)
        for c in cands:
            if c.bin not in eng.bin_index:
                log.warning(f"{c!r}: the bin has no contig in the assembly; skipped")
            else:
                known.append(c)
                if c.mod_type not in targets:
                    log.warning(f"{c!r}: mod type {c.mod_type} is not among the targets; its own columns stay empty")
        bg_keys = background_keys(resident_bins(eng), targets)
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        # the background's one-letter candidates ride in the same engine call as the motifs
        batch = [c.engine_candidate() for c in known] + [(Motif(base, 0), None, b) for b, base in bg_keys]
        _, sites, table = eng.motif_profile(batch, targets=targets, radius=radius)
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        n = len(known)
        write_texts(args.out, (MAIN_NAME, BINS_NAME, SUMMARY_NAME),
                    format_files(known, targets, sites[:n], table[:n], bg_keys, sites[n:], table[n:], int(args.min_called)))
        finish("motif_profile", TIMINGS, t_eng, time.perf_counter() - t0, candidates=n, background_candidates=len(bg_keys), targets=len(targets), radius=radius)
    return 0
