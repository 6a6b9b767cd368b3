"""``nanomotif motif_kmers``: the methylation of EVERY sequence context of every bin — the k-mer table users of modkit and nanodisco
know — without a motif as input.  Every other command after ``motif_discovery`` starts from the motifs of a ``bin-motifs.tsv``; this one
is the independent check on them: what did the greedy search miss, and what did it over-generalise?

    python -m nanomotif_amd motif_kmers ASSEMBLY PILEUP -c CONTIG_BIN --out OUT [--shape 'NNN*NNN'] [--bin_motifs F.tsv ...]
                                        [--min_called 20] [--min_frac 0.7]

Ingest, thresholds and filters are ``motif_sites``' (``loading.load_engine``).  ``--shape``: ``N`` a counted position, ``.`` a skipped
one, exactly one ``*`` for the modified base (``NNN*......NNN`` asks for a bipartite table); at most 10 counted positions, each within
31 of the modified base.  For every bin with a contig and every mod type the pileup holds rows of, one pass over the resident planes
fills the table [4^F][mod, nomod, nocall] (``ScanEngine.kmer_methylation``, nm_kmer_methylation, ``csrc/nmkmers.hip``): a SITE is an A
(or C) on '+' or its complement on '-', its k-mer the letters at the counted offsets read on the site's strand, its state that of
``motif_sites``.  Sites whose window leaves the contig or holds an N are counted in the bin's totals only.

``kmer-methylation.tsv``       bin, mod_type, kmer, n_mod, n_nomod, n_nocall, frac_mod, bin_frac_mod (the bin's background: all its sites),
                               for the k-mers with n_mod + n_nomod >= --min_called; sorted by bin, mod type, row.  The k-mer is spelled
                               with the canonical base at the modified position and ``.`` at the skipped positions.
``kmer-methylation-bins.tsv``  per (bin, mod type) the six totals, the incomplete sites per state and the number of rows written.
With ``--bin_motifs`` a motif, aligned by its ``mod_position``, IMPLIES a k-mer when every position it constrains falls on a counted
offset (or the modified base) and admits the k-mer's letter; it is COMPATIBLE when it admits the letters on the overlap but constrains a
position the shape does not count.  Then the first file has the columns ``implied_by`` and ``compatible_with`` (the bin's motifs of
that mod type, ``;``-separated), and two more files are written:
``kmer-unexplained.tsv``       the written rows with frac_mod >= --min_frac that no motif implies or is compatible with: discovery's
                               candidates for a miss.
``kmer-overcalled.tsv``        the written rows a motif implies whose frac_mod is below 0.3: contexts where the motif is over-general.
``--min_frac`` 0.7 and the 0.3 are the pileup's own call thresholds reused as design choices; they are checked on hand-made tables
(``tests/test_motif_kmers_host.py``), not on real data.  The text is one pure function of the tables (``format_files``).
"""
from __future__ import annotations

import os
import time

import numpy as np

from .engine import KMER_LETTERS, kmer_shape, kmer_text
from .export_run import bin_mod_keys, closing, finish, frac_text, open_run, table_text, write_texts
from .loading import kept_mod_types
from .motif import _BIT, ANY, MOD_TYPE_TO_CANONICAL, Motif, iupac_to_regex

MAIN_NAME = "kmer-methylation.tsv"
BINS_NAME = "kmer-methylation-bins.tsv"
UNEXPLAINED_NAME = "kmer-unexplained.tsv"
OVERCALLED_NAME = "kmer-overcalled.tsv"
MAIN_HEADER = ["bin", "mod_type", "kmer", "n_mod", "n_nomod", "n_nocall", "frac_mod", "bin_frac_mod"]
MOTIF_COLUMNS = ["implied_by", "compatible_with"]
BINS_HEADER = ["bin", "mod_type", "n_mod_fwd", "n_nomod_fwd", "n_nocall_fwd", "n_mod_rev", "n_nomod_rev", "n_nocall_rev", "incomplete_mod", "incomplete_nomod",
               "incomplete_nocall", "rows_written"]
OVERCALLED_BELOW = 0.3
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_kmers.json)


def constraints(motif: str, mod_position: int) -> dict:
    """{offset from the modified base: base set} of the positions a motif (IUPAC spelling) constrains."""
    sets = Motif(iupac_to_regex(motif), int(mod_position)).sets
    return {j - int(mod_position): int(m) for j, m in enumerate(sets) if int(m) != ANY}


def relation(motif: str, mod_position: int, shape, canonical: str, row: int) -> str:
    """"implied", "compatible" or "" : how the motif, aligned by its modified base, stands to the k-mer of ``row`` under ``shape``."""
    offsets = kmer_shape(shape)
    letter = {0: canonical}
    for f, o in enumerate(offsets):
        letter[o] = KMER_LETTERS[(int(row) >> 2 * (len(offsets) - 1 - f)) & 3]
    outside = False
    for o, m in constraints(motif, mod_position).items():
        if o not in letter:
            outside = True
        elif not m & _BIT[letter[o]]:
            return ""
    return "compatible" if outside else "implied"


def format_files(requests, totals, tables, shape, motifs=None, min_called=20, min_frac=0.7):
    """The files as text: (kmer-methylation.tsv, kmer-methylation-bins.tsv), and with ``motifs`` (a list, possibly empty, of
    ``SiteCandidate``) also (kmer-unexplained.tsv, kmer-overcalled.tsv).  ``requests`` = [(bin, mod type)] with ``totals`` int64[n, 2, 3]
    and ``tables`` int64[n, 4^F, 3] of ``ScanEngine.kmer_methylation`` under ``shape``."""
    offsets = kmer_shape(shape)
    header = MAIN_HEADER + (MOTIF_COLUMNS if motifs is not None else [])
    order = sorted(range(len(requests)), key=lambda k: (requests[k][0], requests[k][1]))
    main, bins, unexplained, overcalled = [], [], [], []
    for k in order:
        b, mt = requests[k]
        canonical = MOD_TYPE_TO_CANONICAL[mt]
        tot, tab = np.asarray(totals[k], dtype=np.int64), np.asarray(tables[k], dtype=np.int64)
        both = tot.sum(axis=0)
        bg = frac_text(both[0], both[1])
        own = [c for c in motifs or [] if c.bin == b and c.mod_type == mt]
        written = 0
        for row in np.nonzero(tab[:, 0] + tab[:, 1] >= int(min_called))[0].tolist():
            n_mod, n_nomod, n_nocall = (int(v) for v in tab[row])
            line = [b, mt, kmer_text(offsets, canonical, row), n_mod, n_nomod, n_nocall, frac_text(n_mod, n_nomod), bg]
            written += 1
            if motifs is not None:
                rel = [relation(c.motif, c.mod_position, offsets, canonical, row) for c in own]
                implied = [c.name for c, r in zip(own, rel) if r == "implied"]
                compatible = [c.name for c, r in zip(own, rel) if r == "compatible"]
                line += [";".join(implied), ";".join(compatible)]
                called = n_mod + n_nomod
                if called and n_mod / called >= float(min_frac) and not implied and not compatible:
                    unexplained.append(line)
                if called and implied and n_mod / called < OVERCALLED_BELOW:
                    overcalled.append(line)
            main.append(line)
        bins.append([b, mt] + [int(v) for v in tot.reshape(6)] + [int(v) for v in both - tab.sum(axis=0)] + [written])
    texts = (table_text(header, main), table_text(BINS_HEADER, bins))
    if motifs is not None:
        texts += (table_text(header, unexplained), table_text(header, overcalled))
    return texts


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    shape = kmer_shape(args.shape)
    # (without --bin_motifs nothing is opened before the engine, so a multi-rank launch is not refused: a known quirk, docs/NEXT.md)
    eng, motifs, status = open_run("motif_kmers", args, TIMINGS, with_candidates=bool(args.bin_motifs))
    if eng is None:
        return status
    with closing(eng):
        requests = bin_mod_keys(eng, kept_mod_types(eng))
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        totals, tables = eng.kmer_methylation([(mt, b) for b, mt in requests], shape)
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        # (two texts without motifs: the two further names stay without a file)
        write_texts(args.out, (MAIN_NAME, BINS_NAME, UNEXPLAINED_NAME, OVERCALLED_NAME),
                    format_files(requests, totals, tables, shape, motifs, int(args.min_called), float(args.min_frac)))
        finish("motif_kmers", TIMINGS, t_eng, time.perf_counter() - t0, requests=len(requests), flanks=len(shape))
    return 0
