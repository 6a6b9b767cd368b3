"""Readers of a user's ANNOTATION for ``motif_regions``: BED and GFF3, plain or ``.gz``, into the interval arrays
``ScanEngine.upload_regions`` takes.  Host code in numpy; nothing here needs the engine or the library.

  GFF3   detected by a ``##gff-version`` line or a ``.gff`` / ``.gff3`` suffix (before ``.gz``).  Coordinates are 1-based and inclusive:
         a feature start..end is the interval [start - 1, end).  The class is column 3 (the feature type), the strand column 7, the
         interval's name the ``ID=`` attribute, or else ``contig:start-end`` in the interval's own 0-based coordinates.
  BED    [start, end) as written.  The class is column 4 when the file has at least 4 columns, else the single class ``region``; the
         strand column 6 when present; the name ``contig:start-end``.  ``#`` lines and the lines whose first word is ``track`` or ``browser``
         are skipped (a contig named ``track_12`` is a contig).

Contig names are the assembly's: a contig placed in several bins (``fasta.original_name``) takes the interval on every placement.  An
interval on a contig the engine does not hold is dropped, and all of them are counted in ONE warning line — the pileup readers treat
unbinned contigs the same way.  A bad row (too few columns, coordinates that are not integers or negative, ``end <= start``, an end past
the contig) is a ValueError that names the file and the line.

``classes`` selects and orders the classes (a selected class without an interval stays, with an empty plane); without it the order is
first appearance in the file.  More than ``MAX_CLASSES`` after selection is refused with every class and its interval count.
``upstream`` = N > 0 adds a last class ``upstream``: for every STRANDED interval of a selected class the N bases in front of its start
in its own direction — [max(0, s - N), s) on '+', [e, min(L, e + N)) on '-'; an unstranded interval adds nothing, neither does one that
starts at its contig's end.  The added class counts against the eight."""
from __future__ import annotations

import gzip
import logging as log

import numpy as np

from . import fasta

MAX_CLASSES = 8                 # engine.REGION_MAX_CLASSES (include/nmscan.h NM_REGION_MAX_CLASSES)
PIECE_MAX_WORDS = 2048          # plane words one wave rasterises by default (csrc/nmregions.hip; NM_REGIONS_PIECE_WORDS)
DEFAULT_CLASS = "region"
UPSTREAM_CLASS = "upstream"


class RegionSet:
    """The intervals of an annotation on the engine's contigs: ``class_names`` in plane order; per interval ``contig`` (engine id),
    ``start`` / ``end`` (0-based, half-open), ``cls`` (index into ``class_names``), ``strand`` ('+', '-' or '.') and ``names``;
    ``dropped`` = the intervals on contigs the engine does not hold."""

    def __init__(self, class_names, contig, start, end, cls, strand, names, dropped=0):
        self.class_names = list(class_names)
        self.contig = np.asarray(contig, dtype=np.uint32)
        self.start = np.asarray(start, dtype=np.uint64)
        self.end = np.asarray(end, dtype=np.uint64)
        self.cls = np.asarray(cls, dtype=np.uint8)
        self.strand = list(strand)
        self.names = list(names)
        self.dropped = int(dropped)

    def __len__(self):
        return len(self.names)


def parse_classes(text) -> tuple:
    """``--classes A,B``: the names in the order given, each once; ValueError for an empty list or a name given twice."""
    asked = [s.strip() for s in str(text).split(",") if s.strip()]
    if not asked or len(set(asked)) != len(asked):
        raise ValueError(f"--classes takes a comma-separated list of distinct class names; got {text!r}")
    return tuple(asked)


def parse_upstream(value) -> int:
    """``--upstream``: an integer of at least 0 (0 = off); ValueError otherwise."""
    from .export_run import parse_int_in
    return parse_int_in("--upstream", value, 0)


def is_gff(path: str, first_line: str = "") -> bool:
    p = path[:-3] if path.endswith(".gz") else path
    return p.endswith((".gff", ".gff3")) or first_line.startswith("##gff-version")


def _open_text(path: str):
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path)


def _coordinate(text: str, path: str, line_no: int) -> int:
    if not text.strip().isdigit():
        raise ValueError(f"{path}:{line_no}: coordinate {text!r} is not a non-negative integer")
    return int(text)


def parse_rows(path: str) -> list:
    """The rows of a BED / GFF3 file as (line number, contig, start, end, class, strand, name), [start, end) 0-based; ValueError with
    file and line for a row whose columns or coordinates are bad (the contig's length is not known here)."""
    rows = []
    with _open_text(path) as f:
        lines = f.read().split("\n")
    gff = is_gff(path, next((ln for ln in lines if ln.strip()), ""))
    for line_no, line in enumerate(lines, 1):
        line = line.rstrip("\r")
        if gff and line.startswith("##FASTA"):
            break
        if not line.strip() or line.startswith("#") or (not gff and line.split(None, 1)[0] in ("track", "browser")):
            continue
        col = line.split("\t")
        if len(col) < (8 if gff else 3):
            raise ValueError(f"{path}:{line_no}: {len(col)} columns, a {'GFF3' if gff else 'BED'} row has at least {8 if gff else 3}")
        if gff:
            first, end = _coordinate(col[3], path, line_no), _coordinate(col[4], path, line_no)
            if first < 1:
                raise ValueError(f"{path}:{line_no}: GFF3 coordinates are 1-based, got start {first}")
            start, cls, strand = first - 1, col[2], col[6] if col[6] in ("+", "-") else "."
            ident = [a[3:] for a in (col[8].split(";") if len(col) > 8 else []) if a.startswith("ID=")]
            name = ident[0] if ident else None
        else:
            start, end = _coordinate(col[1], path, line_no), _coordinate(col[2], path, line_no)
            cls = col[3] if len(col) >= 4 else DEFAULT_CLASS
            strand, name = (col[5] if len(col) >= 6 and col[5] in ("+", "-") else "."), None
        if end <= start:
            raise ValueError(f"{path}:{line_no}: end {end} <= start {start} (0-based, half-open)")
        rows.append((line_no, col[0], start, end, cls, strand, name or f"{col[0]}:{start}-{end}"))
    return rows


def select_classes(rows, classes=None, upstream=0) -> list:
    """The class names in plane order: ``classes`` as given, else first appearance among ``rows``; ``upstream`` > 0 appends
    ``UPSTREAM_CLASS``.  ValueError above ``MAX_CLASSES``, with every class and its interval count."""
    counts = {}
    for r in rows:
        counts[r[4]] = counts.get(r[4], 0) + 1
    names = list(classes) if classes is not None else list(counts)
    if upstream:
        if UPSTREAM_CLASS in names:
            raise ValueError(f"--upstream adds the class {UPSTREAM_CLASS!r}, which the annotation already has")
        names.append(UPSTREAM_CLASS)
    if len(names) > MAX_CLASSES:
        listed = ", ".join(f"{n} ({counts.get(n, 0)})" for n in names)
        raise ValueError(f"{len(names)} region classes, at most {MAX_CLASSES} fit: {listed}; select with --classes")
    if not names:
        names = [DEFAULT_CLASS]
    return names


def upstream_of(start: int, end: int, strand: str, length: int, n: int):
    """The ``n`` bases in front of a stranded interval's start in its own direction, clipped to the contig; None when there are none."""
    if strand == "+":
        lo, hi = max(0, start - n), start
    elif strand == "-":
        lo, hi = end, min(length, end + n)
    else:
        return None
    return (lo, hi) if hi > lo else None


def read_regions(path: str, contig_index: dict, contig_len, classes=None, upstream=0, rows=None) -> RegionSet:
    """The annotation ``path`` on the engine's contigs (``contig_index``: engine contig name -> id; ``contig_len``: length per id).
    ``rows``: ``parse_rows(path)`` when the caller has read the file already (the command does, before it opens the engine)."""
    rows = parse_rows(path) if rows is None else rows
    names = select_classes(rows, classes, upstream)
    index = {n: k for k, n in enumerate(names)}
    placements = {}
    for name, i in contig_index.items():
        placements.setdefault(fasta.original_name(name), []).append(int(i))
    out = ([], [], [], [], [], [])
    dropped, dropped_contigs = 0, set()

    def add(i, s, e, c, strand, name):
        for a, v in zip(out, (i, s, e, c, strand, name)):
            a.append(v)
    for line_no, contig, start, end, cls, strand, name in rows:
        if cls not in index:
            continue
        ids = placements.get(contig)
        if not ids:
            dropped += 1
            dropped_contigs.add(contig)
            continue
        for i in ids:
            length = int(contig_len[i])
            if end > length:
                raise ValueError(f"{path}:{line_no}: end {end} is past the {length} positions of contig {contig}")
            add(i, start, end, index[cls], strand, name)
            up = upstream_of(start, end, strand, length, int(upstream)) if upstream else None
            if up is not None:
                add(i, up[0], up[1], index[UPSTREAM_CLASS], strand, name)
    if dropped:
        log.warning(f"{path}: {dropped} intervals on {len(dropped_contigs)} contigs the assembly's bins do not hold; dropped")
    return RegionSet(names, *out, dropped=dropped)


def piece_count(start, end, piece_words: int = PIECE_MAX_WORDS) -> int:
    """The pieces the rasteriser cuts the intervals [start[i], end[i]) into: every interval is cut at multiples of ``piece_words`` plane
    words (32 positions each) from its contig's first word."""
    p = int(piece_words)
    return int(sum((int(e) - 1) // 32 // p - int(s) // 32 // p + 1 for s, e in zip(start, end)))
