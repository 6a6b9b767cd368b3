"""``nanomotif motif_tracks``: the methylation of the motifs of a ``bin-motifs.tsv`` ALONG the contigs of their bins, and its breakpoints.

``motif_sites`` / ``motif_coverage`` / ``motif_compare`` / ``motif_strands`` / ``motif_profile`` reduce a motif to one row per bin or per contig.
Where along a contig the methylation sits is what tells a chimeric contig (``detect_contamination`` sees an averaged fraction; along the
contig it is a step function with one breakpoint) from recently acquired DNA (an unmethylated stretch inside a methylated contig) and from
a local loss of calls (``nocall`` rises while ``frac_mod`` stays put).  The reference has nothing here: ``motif_model_contig``
(find_motifs_bin.py:1285-1331) sums over the contig.

Definitions (include/nmscan.h, nm_motif_tracks_count).  ``--window`` = W is a multiple of 128 in [128, 2^30]; a contig of length L has
max(1, ceil(L / W)) windows, window i covers [i W, min((i + 1) W, L)).  A candidate is (bin, motif, mod_position); its occurrences and their
states (mod, nomod, nocall; a position called both ways is mod) are those of ``motif_sites``: the stripped motif on '+', its reverse
complement on '-'.  An occurrence belongs to the window that holds its modified base, on either strand.  The bin's background — every
occurrence of the mod type's canonical base, the one-letter candidate — rides in the same engine calls, one per (bin, mod type present
among the candidates).

Segmentation (host, numpy float64, from the integer tables).  Per (candidate, contig) the windows' m_i = mod and u_i = nomod over both
strands, c_i = m_i + u_i.  A split of the segment [a, b) of windows at k is admissible when either side holds at least ``--min_called``
called sites; its gain is the likelihood-ratio statistic G = 2 [ll(m_L, c_L) + ll(m_R, c_R) - ll(m, c)] with
ll(m, n) = m ln(m / n) + (n - m) ln((n - m) / n), 0 ln 0 = 0.  Binary segmentation: start with the whole contig; repeatedly take the
segment whose best admissible split has the highest gain (ties: the leftmost segment; within a segment the lowest k) and split it while
the gain is >= ``--min_gain`` and fewer than ``--max_segments`` segments exist.  The default of 30 is a design choice: the chi-square(1)
tail beyond 30 is about 4e-8, which leaves room for the ~1e5 split positions a long contig offers; real pileups are overdispersed, which
is why it is a knob.

Files (tab-separated, header line; candidates in file order, contigs in bin order):
  ``motif-tracks-contigs.tsv``   per (candidate, contig): length, n_windows, the counts over both strands, ``frac_mod`` = n_mod / (n_mod +
                                 n_nomod) (empty when nothing is called), ``n_segments``, the best admissible first split of the whole
                                 contig whether or not it was accepted (``best_split`` in bp, ``best_gain``, ``frac_left``,
                                 ``frac_right``; empty when none is admissible) and ``flag``: ``uniform`` for 1 segment, ``breakpoint``
                                 for 2, ``islands`` for 3 or more
  ``motif-tracks-segments.tsv``  per segment: ``segment``, ``start``, ``end``, the three counts and ``frac_mod``, and the background over
                                 the same windows (``bg_n_mod``, ``bg_n_nomod``, ``bg_frac_mod``)
  ``motif-tracks.tsv``           with ``--tracks``: per (candidate, contig, window) that holds an occurrence the six counts and ``frac_mod``
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import fasta
from .engine import TRACKS_MAX_WINDOW, TRACKS_MIN_WINDOW
from .export_run import background_candidates, background_keys, closing, finish, frac_text, open_run, parse_int_in, split_known, table_text

CONTIGS_NAME = "motif-tracks-contigs.tsv"
SEGMENTS_NAME = "motif-tracks-segments.tsv"
TRACKS_NAME = "motif-tracks.tsv"
KEY_COLUMNS = ["bin", "contig", "motif", "mod_type", "mod_position"]
CONTIGS_HEADER = KEY_COLUMNS + ["length", "n_windows", "n_mod", "n_nomod", "n_nocall", "frac_mod", "n_segments", "best_split", "best_gain", "frac_left",
                                "frac_right", "flag"]
SEGMENTS_HEADER = KEY_COLUMNS + ["segment", "start", "end", "n_mod", "n_nomod", "n_nocall", "frac_mod", "bg_n_mod", "bg_n_nomod", "bg_frac_mod"]
TRACKS_HEADER = ["contig", "start", "end", "bin", "motif", "mod_type", "mod_position", "n_mod_fwd", "n_nomod_fwd", "n_nocall_fwd", "n_mod_rev", "n_nomod_rev",
                 "n_nocall_rev", "frac_mod"]
FLAGS = ("uniform", "breakpoint", "islands")
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_tracks.json)


def parse_window(value) -> int:
    """``--window``: a multiple of 128 in [128, 2^30] (128 = one lane's span of a wave-chunk); ValueError otherwise."""
    return parse_int_in("--window", value, TRACKS_MIN_WINDOW, TRACKS_MAX_WINDOW, step=TRACKS_MIN_WINDOW,
                        what=f"a multiple of {TRACKS_MIN_WINDOW} in [{TRACKS_MIN_WINDOW}, 2^30]")


# ------------------------------------------------------------------------------------------------ segmentation
def _xlogx(m, n):
    """m ln(m / n) elementwise, 0 where m = 0."""
    m = np.asarray(m, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    out = np.zeros(np.broadcast(m, n).shape, dtype=np.float64)
    pos = m > 0
    np.multiply(m, np.log(np.divide(m, n, out=np.ones_like(out), where=pos)), out=out, where=pos)
    return out


def log_likelihood(m, n):
    """ll(m, n) = m ln(m / n) + (n - m) ln((n - m) / n) with 0 ln 0 = 0: the maximised binomial log-likelihood of m of n."""
    m = np.asarray(m, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    return _xlogx(m, n) + _xlogx(n - m, n)


def best_split(cum_m, cum_c, a: int, b: int, min_called: int):
    """The best admissible split of the windows [a, b): (k, gain) with a < k < b, the lowest k among equal gains, or None.  ``cum_m`` /
    ``cum_c``: int64[n + 1] prefixes of the windows' mod counts and called counts."""
    if b - a < 2:
        return None
    k = np.arange(a + 1, b)
    m_l, c_l = cum_m[k] - cum_m[a], cum_c[k] - cum_c[a]
    m_r, c_r = cum_m[b] - cum_m[k], cum_c[b] - cum_c[k]
    ok = (c_l >= min_called) & (c_r >= min_called)
    if not ok.any():
        return None
    gain = 2.0 * (log_likelihood(m_l, c_l) + log_likelihood(m_r, c_r) - log_likelihood(cum_m[b] - cum_m[a], cum_c[b] - cum_c[a]))
    gain = np.where(ok, np.maximum(gain, 0.0), -1.0)
    i = int(np.argmax(gain))                                            # the first of equal maxima: the lowest k
    return int(k[i]), float(gain[i])


def segment(mod, nomod, min_gain: float, min_called: int, max_segments: int):
    """Binary segmentation of one (candidate, contig): ``mod`` / ``nomod`` = the windows' counts over both strands.  Returns (bounds,
    first): ``bounds`` = the ascending window indices [0, ..., n] that delimit the segments, ``first`` = the best admissible split of the
    whole contig, (k, gain, (m_L, c_L), (m_R, c_R)), whether or not it was accepted, or None."""
    mod = np.asarray(mod, dtype=np.int64)
    called = mod + np.asarray(nomod, dtype=np.int64)
    n = len(mod)
    cum_m, cum_c = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    np.cumsum(mod, out=cum_m[1:])
    np.cumsum(called, out=cum_c[1:])
    min_called = max(int(min_called), 0)
    whole = best_split(cum_m, cum_c, 0, n, min_called)
    first = None
    if whole is not None:
        k = whole[0]
        first = (k, whole[1], (int(cum_m[k]), int(cum_c[k])), (int(cum_m[n] - cum_m[k]), int(cum_c[n] - cum_c[k])))
    segs = [(0, n, whole)]                                              # ascending start; (a, b, best split of [a, b))
    while len(segs) < int(max_segments):
        pick = None
        for i, (_, _, s) in enumerate(segs):                            # the highest gain, the leftmost among equal ones
            if s is not None and (pick is None or s[1] > segs[pick][2][1]):
                pick = i
        if pick is None or segs[pick][2][1] < float(min_gain):
            break
        a, b, (k, _) = segs[pick]
        segs[pick:pick + 1] = [(a, k, best_split(cum_m, cum_c, a, k, min_called)), (k, b, best_split(cum_m, cum_c, k, b, min_called))]
    return [s[0] for s in segs] + [n], first


# ------------------------------------------------------------------------------------------------ the files
def candidate_rows(cand, names, prefix, table, bg_table, lengths, window: int, min_gain: float, min_called: int, max_segments: int, tracks: bool):
    """The rows of one candidate for the three files.  ``names`` / ``prefix`` / ``table``: its item of ``ScanEngine.motif_tracks``;
    ``bg_table``: the table of the background of its (bin, mod type) in the same layout, or None; ``lengths``: contig name -> length."""
    contig_rows, segment_rows, track_rows = [], [], []
    table = np.asarray(table, dtype=np.int64)
    for i, name in enumerate(names):
        w0, w1 = int(prefix[i]), int(prefix[i + 1])
        six = table[w0:w1]
        length = int(lengths[name])
        shown = fasta.original_name(name)
        key = [cand.bin, shown, cand.motif, cand.mod_type, cand.mod_position]
        three = six[:, :3] + six[:, 3:]
        bounds, first = segment(three[:, 0], three[:, 1], min_gain, min_called, max_segments)
        total = three.sum(axis=0)
        n_seg = len(bounds) - 1
        split = ["", "", "", ""]
        if first is not None:
            k, gain, (m_l, c_l), (m_r, c_r) = first
            split = [k * window, "%.3f" % gain, frac_text(m_l, c_l - m_l), frac_text(m_r, c_r - m_r)]
        contig_rows.append(key + [length, w1 - w0, int(total[0]), int(total[1]), int(total[2]), frac_text(total[0], total[1]), n_seg] + split +
                           [FLAGS[min(n_seg, 3) - 1]])
        bg = None if bg_table is None else np.asarray(bg_table[w0:w1], dtype=np.int64)
        for s in range(n_seg):
            a, b = bounds[s], bounds[s + 1]
            n = three[a:b].sum(axis=0)
            if bg is None:
                bg_cols = ["", "", ""]
            else:
                g = bg[a:b].sum(axis=0)
                bg_cols = [int(g[0] + g[3]), int(g[1] + g[4]), frac_text(g[0] + g[3], g[1] + g[4])]
            segment_rows.append(key + [s, a * window, min(b * window, length), int(n[0]), int(n[1]), int(n[2]), frac_text(n[0], n[1])] + bg_cols)
        if tracks:
            for j in np.flatnonzero(six.any(axis=1)).tolist():
                r = six[j].tolist()
                track_rows.append([shown, j * window, min((j + 1) * window, length), cand.bin, cand.motif, cand.mod_type, cand.mod_position] + r +
                                  [frac_text(r[0] + r[3], r[1] + r[4])])
    return contig_rows, segment_rows, track_rows


def format_files(cands, items, bg_tables, lengths, window: int, min_gain=30.0, min_called=20, max_segments=8, tracks=False):
    """(motif-tracks-contigs.tsv, motif-tracks-segments.tsv, motif-tracks.tsv or None) as text.  ``cands``: ``SiteCandidate`` in file order
    with their ``items`` of ``ScanEngine.motif_tracks``; ``bg_tables``: (bin, mod type) -> the background's table."""
    rows = ([], [], [])
    for c, (names, prefix, table) in zip(cands, items):
        got = candidate_rows(c, names, prefix, table, bg_tables.get((c.bin, c.mod_type)), lengths, window, min_gain, min_called, max_segments, tracks)
        for mine, new in zip(rows, got):
            mine += new
    return table_text(CONTIGS_HEADER, rows[0]), table_text(SEGMENTS_HEADER, rows[1]), table_text(TRACKS_HEADER, rows[2]) if tracks else None


def _body(text: str) -> str:
    return text[text.index("\n") + 1:]


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    window = parse_window(args.window)
    eng, cands, status = open_run("motif_tracks", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        known = split_known(cands, eng, eng.slot_of_mod)
        bg_keys = background_keys(known)
        lengths = {n: int(eng.contig_lengths[eng.contig_index[n]]) for b in {c.bin for c in known} for n in eng.bin_contigs(b)}
        os.makedirs(args.out, exist_ok=True)
        # the background's one-letter candidates ride in the same engine calls, ahead of the motifs that are read against them
        batch = background_candidates(bg_keys) + [c.engine_candidate() for c in known]
        items = eng.motif_tracks(batch, window=window)
        t_eng = t_text = 0.0
        bg_tables = {}
        names = (CONTIGS_NAME, SEGMENTS_NAME) + ((TRACKS_NAME,) if args.tracks else ())
        files = [open(os.path.join(args.out, n), "w") for n in names]
        try:
            for f, header in zip(files, (CONTIGS_HEADER, SEGMENTS_HEADER, TRACKS_HEADER)):
                f.write("\t".join(header) + "\n")
            t0 = time.perf_counter()
            for k, item in enumerate(items):
                t1 = time.perf_counter()
                t_eng += t1 - t0
                if k < len(bg_keys):
                    bg_tables[bg_keys[k]] = item[2].copy()
                else:
                    texts = format_files([known[k - len(bg_keys)]], [item], bg_tables, lengths, window, float(args.min_gain), int(args.min_called),
                                         int(args.max_segments), bool(args.tracks))
                    for f, text in zip(files, texts):
                        f.write(_body(text))
                t0 = time.perf_counter()
                t_text += t0 - t1
            t_eng += time.perf_counter() - t0
        finally:
            for f in files:
                f.close()
        finish("motif_tracks", TIMINGS, t_eng, t_text, label="segmentation and text", candidates=len(known), background_candidates=len(bg_keys), window=window)
    return 0
