"""``nanomotif motif_context``: the sequence AROUND the sites of the motifs of a ``bin-motifs.tsv``, counted apart by the methylation state
of the site.

``motif_sites`` … ``motif_fractions`` accept a discovered motif as given and read its methylation.  The first question about a motif
reported at 60 % methylated is whether it is under-specified: if discovery stopped at ``GATC`` and the methyltransferase recognises
``RGATCY``, the sites with R before and Y behind are methylated and the rest are not.  ``motif_fractions`` shows that as ``bimodal`` and
``motif_tracks`` as ``uniform``; this command names the position and the letters that separate the two populations.  One pass over a
motif's sites counts the letter at every offset per state (``ScanEngine.motif_context``, nm_motif_context_count): the cell (offset o,
letter X) is the ``n_mod`` / ``n_nomod`` row ``motif_sites`` would give the motif narrowed to X at o, so one call scores every
one-position refinement of every motif, and the counts are exact.

Definition.  A candidate is (bin, motif, mod_type, mod_position); its occurrences and their states (mod / nomod / nocall, in the
candidate's own mod type) are those of ``motif_sites``.  An occurrence has its modified base at '+' coordinate p on occurrence strand s;
for an offset o in the motif's reading direction, -R <= o <= R (``--radius``), the probed position is p + o on '+' and p - o on '-', and
its letter is the contig's read on strand s (the complement on '-'): A, C, G or T.  N, any other character and a position outside the
contig have no letter (``other`` in the engine's table; not a row of the files, but the fifth group of the gain below).

The pileup goes through the ingest path of ``motif_discovery`` (``loading.load_engine``), so offset 0 summed over the letters reproduces
the row's ``n_mod`` / ``n_nomod`` of ``bin-motifs.tsv``.

Files (tab-separated, header line; candidates in file order, ascending offset, letters A, C, G, T):
  ``motif-context.tsv``          per (candidate, offset, letter): ``n_mod`` / ``n_nomod`` / ``n_nocall`` pooled over both occurrence strands
                                 and all contigs of the bin, ``frac_mod`` = n_mod / (n_mod + n_nomod) (empty when nothing is called),
                                 ``share_mod`` / ``share_nomod`` = the letter's share among the candidate's mod / nomod sites, and
                                 ``refined_motif`` / ``refined_mod_position``: the motif this cell is the row of — the candidate with the
                                 position at o narrowed to the letter, padded with ``.`` (``N`` in the IUPAC spelling of the files) when o
                                 lies outside it; empty when the motif excludes the letter there or the result would exceed the engine's
                                 motif length / reach limit
  ``motif-context-bins.tsv``     the background, the bin's methylation logo: the same table for the one-letter candidate (every A / every
                                 C of the bin) per (bin with a contig, mod type of the pileup), ``motif`` = the canonical base
  ``motif-context-summary.tsv``  per candidate: its ``n_mod`` / ``n_nomod`` / ``n_nocall`` / ``frac_mod``; ``best_offset`` / ``best_gain``: the
                                 offset with the largest gain(o) = sum over the letter groups L of ll(m_L, c_L) - ll(m, c), the binomial
                                 likelihood-ratio gain of splitting the called sites (m of c methylated) by the letter at o
                                 (``motif_tracks.log_likelihood``; the sites whose probe is ``other`` are a fifth group; ties: smallest
                                 |o|, negative before positive); ``keep``: the letters at that offset with a called site and a frac_mod
                                 >= the candidate's own; ``refined_*``: the motif narrowed to ``keep`` there (an IUPAC set) and its counts;
                                 ``kept_mod_share`` = refined_n_mod / n_mod; ``dropped_called`` / ``dropped_frac_mod``: the called sites
                                 that are not kept; ``flag`` = ``few_sites`` below ``--min_called`` called sites, ``underspecified``
                                 when best_gain >= ``--min_gain`` and dropped_called >= ``--min_called``, else ``none``

``--min_gain`` 30 and ``--min_called`` 20 are design choices taken over from ``motif_tracks``: they are pinned on hand-made tables
(``tests/test_motif_context_host.py``), not on real data.
"""
from __future__ import annotations

import os
import time

import numpy as np

from .engine import CONTEXT_MAX_RADIUS, MAX_MOTIF_LEN, MAX_REACH
from .export_run import (background_candidates, bin_mod_keys, closing, finish, frac_text, open_run, parse_int_in, share_text, split_known, table_text,
                         write_texts)
from .loading import kept_mod_types
from .motif import _BIT, ANY, MOD_TYPE_TO_CANONICAL, Motif, iupac_to_regex
from .motif_tracks import log_likelihood

MAIN_NAME = "motif-context.tsv"
BINS_NAME = "motif-context-bins.tsv"
SUMMARY_NAME = "motif-context-summary.tsv"
LETTERS = "ACGT"
KEY_COLUMNS = ["bin", "motif", "mod_type", "mod_position"]
MAIN_HEADER = KEY_COLUMNS + ["offset", "letter", "n_mod", "n_nomod", "n_nocall", "frac_mod", "share_mod", "share_nomod", "refined_motif", "refined_mod_position"]
SUMMARY_HEADER = KEY_COLUMNS + ["n_mod", "n_nomod", "n_nocall", "frac_mod", "best_offset", "best_gain", "keep", "refined_motif", "refined_mod_position",
                                "refined_n_mod", "refined_n_nomod", "refined_frac_mod", "kept_mod_share", "dropped_called", "dropped_frac_mod", "flag"]
FLAGS = ("none", "underspecified", "few_sites")
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_context.json)


def parse_radius(value) -> int:
    """``--radius``: an integer in 0..31; ValueError otherwise."""
    return parse_int_in("--radius", value, 0, CONTEXT_MAX_RADIUS)


def pooled(table) -> np.ndarray:
    """int64[W, 2 (occurrence strand), 3 (state), 5] of one candidate -> int64[W, 3, 5] over both occurrence strands."""
    return np.asarray(table, dtype=np.int64).sum(axis=1)


def refined(motif: str, mod_position: int, offset: int, letters: str):
    """(motif in the IUPAC spelling of bin-motifs.tsv, mod_position) of the candidate narrowed to ``letters`` at ``offset`` from its
    modified base, padded with ``.`` when the offset lies outside it; ("", "") when the motif excludes all of ``letters`` there, when
    ``letters`` is empty, or when the result is beyond the engine's motif length / reach limit."""
    m = Motif(iupac_to_regex(motif), int(mod_position))
    sets, pos = list(m.sets), int(mod_position)
    at = pos + int(offset)
    if at < 0:
        sets, pos, at = [ANY] * (-at) + sets, pos - at, 0
    elif at >= len(sets):
        sets = sets + [ANY] * (at + 1 - len(sets))
    want = 0
    for ch in letters:
        want |= _BIT[ch]
    sets[at] &= want
    if not sets[at]:
        return "", ""
    out = Motif.from_sets(sets, pos).new_stripped_motif()
    n = len(out.tokens)
    if n > MAX_MOTIF_LEN or out.mod_position > MAX_REACH + 1 or n - 1 - out.mod_position > MAX_REACH:
        return "", ""
    return out.iupac(), out.mod_position


def context_rows(key, cells) -> list:
    """The rows of one candidate in motif-context.tsv (``key``: its four key columns; ``cells`` = ``pooled`` of its table)."""
    width = cells.shape[0]
    radius = (width - 1) // 2
    total = cells[0].sum(axis=1)                                          # the candidate's sites per state: every offset sums to them
    rows = []
    for w in range(width):
        for x, letter in enumerate(LETTERS):
            n = [int(v) for v in cells[w, :, x]]
            rows.append(list(key) + [w - radius, letter] + n + [frac_text(n[0], n[1]), share_text(n[0], total[0]), share_text(n[1], total[1])] +
                        list(refined(key[1], key[3], w - radius, letter)))
    return rows


def gains(cells) -> np.ndarray:
    """float64[W]: per offset the binomial likelihood-ratio gain of splitting the called sites by the letter group (A, C, G, T, other)."""
    m = cells[:, 0, :].astype(np.int64)
    c = m + cells[:, 1, :]
    return log_likelihood(m, c).sum(axis=1) - log_likelihood(m.sum(axis=1), c.sum(axis=1))


def best_offset(gain) -> int:
    """Index of the largest gain; ties: smallest |offset|, negative before positive."""
    radius = (len(gain) - 1) // 2
    return min(range(len(gain)), key=lambda w: (-float(gain[w]), abs(w - radius), w - radius))


def summary_row(key, cells, min_called: int, min_gain: float) -> list:
    """One row of motif-context-summary.tsv."""
    width = cells.shape[0]
    radius = (width - 1) // 2
    n_mod, n_nomod, n_nocall = (int(v) for v in cells[0].sum(axis=1))
    called = n_mod + n_nomod
    gain = gains(cells)
    w = best_offset(gain)
    m_l, c_l = cells[w, 0, :4], cells[w, 0, :4] + cells[w, 1, :4]
    # frac_mod of the letter >= the candidate's own, as an integer comparison of the two shares
    keep = "".join(ch for x, ch in enumerate(LETTERS) if c_l[x] > 0 and int(m_l[x]) * called >= n_mod * int(c_l[x]))
    r_mod = sum(int(m_l[x]) for x, ch in enumerate(LETTERS) if ch in keep)
    r_called = sum(int(c_l[x]) for x, ch in enumerate(LETTERS) if ch in keep)
    d_mod, d_called = n_mod - r_mod, called - r_called
    if called < int(min_called):
        flag = "few_sites"
    elif float(gain[w]) >= float(min_gain) and d_called >= int(min_called):
        flag = "underspecified"
    else:
        flag = "none"
    return (list(key) + [n_mod, n_nomod, n_nocall, frac_text(n_mod, n_nomod), w - radius, "%.3f" % float(gain[w]), keep] + list(refined(key[1], key[3], w - radius, keep)) +
            [r_mod, r_called - r_mod, frac_text(r_mod, r_called - r_mod), share_text(r_mod, n_mod), d_called, frac_text(d_mod, d_called - d_mod), flag])


def format_files(cands, tables, bg_keys, bg_tables, min_called=20, min_gain=30.0):
    """(motif-context.tsv, motif-context-bins.tsv, motif-context-summary.tsv) as text.  ``cands``: ``SiteCandidate`` in file order with
    ``tables`` int64[n, W, 2, 3, 5] of ``ScanEngine.motif_context``; ``bg_keys`` = [(bin, mod type)] with the same of the one-letter
    candidates."""
    bins_rows, main_rows, summary_rows = [], [], []
    for (b, mt), t in zip(bg_keys, bg_tables):
        bins_rows += context_rows([b, MOD_TYPE_TO_CANONICAL[mt], mt, 0], pooled(t))
    for c, t in zip(cands, tables):
        cells = pooled(t)
        key = [c.bin, c.motif, c.mod_type, c.mod_position]
        main_rows += context_rows(key, cells)
        summary_rows.append(summary_row(key, cells, min_called, min_gain))
    return table_text(MAIN_HEADER, main_rows), table_text(MAIN_HEADER, bins_rows), table_text(SUMMARY_HEADER, summary_rows)


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    radius = parse_radius(args.radius)
    eng, cands, status = open_run("motif_context", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        mod_types = kept_mod_types(eng)
        known = split_known(cands, eng, mod_types)
        bg_keys = bin_mod_keys(eng, mod_types)
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        # the background's one-letter candidates ride in the same engine call as the motifs
        _, table = eng.motif_context([c.engine_candidate() for c in known] + background_candidates(bg_keys), radius=radius)
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        n = len(known)
        write_texts(args.out, (MAIN_NAME, BINS_NAME, SUMMARY_NAME),
                    format_files(known, table[:n], bg_keys, table[n:], int(args.min_called), float(args.min_gain)))
        finish("motif_context", TIMINGS, t_eng, time.perf_counter() - t0, candidates=n, background_candidates=len(bg_keys), radius=radius)
    return 0
