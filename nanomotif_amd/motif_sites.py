"""``nanomotif motif_sites``: where every motif of a ``bin-motifs.tsv`` occurs on the contigs of its bin, and whether the occurrence
is methylated, unmethylated or without a call.

The reference keeps this view in memory only — ``motif_model_contig(..., save_motif_positions=True)`` (find_motifs_bin.py:1285-1331)
returns index_meth_fwd / index_nonmeth_fwd / index_meth_rev / index_nonmeth_rev for one motif on one contig — and has no command for
it; the no-call class (occurrences found by ``subseq_indices``, utils.py:44-67, that carry neither call) has no counterpart there.

The pileup goes through the ingest path of ``motif_discovery`` (``loading.load_engine``: same readers, same pre-filters, same
thresholds), so the state planes are the ones the counts of ``bin-motifs.tsv`` were scored on: the summary's ``n_mod`` / ``n_nomod``
summed over a bin's contigs are the row's.  (Under non-default thresholds ``motif_discovery`` scores the motifs its merge stage makes
on a second classification fixed at 0.3 / 0.7, find_motifs_bin.py:569; this command exports the classification of the thresholds it
is given.)

Files: ``motif-sites.bed`` (contig, start, end, motif_modtype_modposition, 0, strand, state, bin — no header, candidates in
``bin-motifs.tsv`` order, within a candidate contigs in bin order, ascending position, '+' before '-') and
``motif-sites-summary.tsv`` (one row per bin, contig, motif, mod_type, mod_position: the six counts and their sums over the strands).
"""
from __future__ import annotations

import csv
import ctypes as C
import os
import time

import numpy as np

from . import _lib, fasta
from .engine import SITE_STATES, ScanEngine
from .export_run import closing, finish, open_candidates, open_run, split_known, table_text, write_texts      # (open_*: also found here)
from .motif import Motif, iupac_to_regex

BED_NAME = "motif-sites.bed"
SUMMARY_NAME = "motif-sites-summary.tsv"
SUMMARY_HEADER = ["bin", "contig", "motif", "mod_type", "mod_position", "n_mod_fwd", "n_nomod_fwd", "n_nocall_fwd", "n_mod_rev", "n_nomod_rev",
                  "n_nocall_rev", "n_mod", "n_nomod", "n_nocall"]
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_sites.json)


def parse_states(text: str) -> tuple:
    """``--states mod,nocall`` -> ("mod", "nocall"), in the canonical order, each once; ValueError names what is not a state."""
    asked = [s.strip() for s in str(text).split(",") if s.strip()]
    bad = [s for s in asked if s not in SITE_STATES]
    if bad or not asked:
        raise ValueError(f"--states takes a comma-separated selection of {', '.join(SITE_STATES)}; got {text!r}")
    return tuple(s for s in SITE_STATES if s in asked)


class SiteCandidate:
    """One exported (bin, motif): ``motif`` in the IUPAC spelling of bin-motifs.tsv, ``name`` = motif_modtype_modposition."""
    __slots__ = ("bin", "motif", "mod_type", "mod_position")

    def __init__(self, bin, motif, mod_type, mod_position):
        self.bin, self.motif, self.mod_type, self.mod_position = bin, motif, mod_type, int(mod_position)

    @property
    def name(self):
        return f"{self.motif}_{self.mod_type}_{self.mod_position}"

    @property
    def key(self):
        return (self.bin, self.motif, self.mod_type, self.mod_position)

    def engine_candidate(self):
        return (Motif(iupac_to_regex(self.motif), self.mod_position), self.mod_type, self.bin)

    def __repr__(self):
        return f"SiteCandidate({self.bin!r}, {self.name!r})"


def candidates_of_bin_motifs(path) -> list:
    """The candidates of a bin-motifs.tsv in file order: every row's motif in the bin of its ``reference`` column, then — when the row
    has a ``motif_complement`` — that complement with ``mod_position_complement``; a (bin, motif, mod_type, position) seen before is
    not repeated."""
    out, seen = [], set()
    with open(path, newline="") as f:
        reader = csv.DictReader(f, delimiter="\t")
        need = {"reference", "motif", "mod_position", "mod_type"}
        if reader.fieldnames is None or not need <= set(reader.fieldnames):
            raise ValueError(f"{path}: not a bin-motifs.tsv (columns {sorted(need)} are required)")
        for row in reader:
            both = [SiteCandidate(row["reference"], row["motif"], row["mod_type"], int(float(row["mod_position"])))]
            comp = (row.get("motif_complement") or "").strip()
            if comp and comp.lower() not in ("nan", "none", "null"):
                both.append(SiteCandidate(row["reference"], comp, row["mod_type"], int(float(row["mod_position_complement"]))))
            for c in both:
                if c.key not in seen:
                    seen.add(c.key)
                    out.append(c)
    return out


def format_sites(contig, pos, code, seg_begin, seg_names, seg_bins, contig_names, symbol="nm_motif_sites_text", seg_partner_offsets=None) -> bytes:
    """The lines of motif-sites.bed for records (contig, pos, code) cut into runs [seg_begin[s], seg_begin[s + 1]) that share a name
    and a bin (nm_motif_sites_text: native, on up to NM_POST_THREADS threads).  ``symbol``: the writer, nm_motif_compare_text for the
    records of ``ScanEngine.motif_compare_sites`` (switched-sites.bed), nm_motif_strands_text with the runs' ``seg_partner_offsets`` for
    those of ``ScanEngine.motif_strand_sites`` (hemi-sites.bed)."""
    lib = _lib.load()
    text = getattr(lib, symbol)
    n = len(contig)
    if n == 0:
        return b""
    contig = np.ascontiguousarray(contig, dtype=np.uint32)
    pos = np.ascontiguousarray(pos, dtype=np.uint32)
    code = np.ascontiguousarray(code, dtype=np.uint8)
    seg_begin = np.ascontiguousarray(seg_begin, dtype=np.uint64)
    parts = [x.encode() for pair in zip(seg_names, seg_bins) for x in pair]
    seg_off = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in parts], out=seg_off[1:])
    cparts = [x.encode() for x in contig_names]
    c_off = np.zeros(len(cparts) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in cparts], out=c_off[1:])
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    extra = ()
    if seg_partner_offsets is not None:
        seg_partner_offsets = np.ascontiguousarray(seg_partner_offsets, dtype=np.int32)
        extra = (p(seg_partner_offsets, C.c_int32),)
    args = (n, p(contig, C.c_uint32), p(pos, C.c_uint32), p(code, C.c_uint8), len(seg_names), p(seg_begin, C.c_uint64), b"".join(parts),
            p(seg_off, C.c_uint64), *extra, len(cparts), b"".join(cparts), p(c_off, C.c_uint64))
    size = C.c_uint64(0)
    _lib.check(text(*args, None, 0, C.byref(size)))
    buf = np.empty(size.value, dtype=np.uint8)
    _lib.check(text(*args, buf.ctypes.data_as(C.c_void_p), size.value, C.byref(size)))
    return buf.tobytes()


def write_site_batches(eng: ScanEngine, batches, cands: list, bed_file, symbol="nm_motif_sites_text", summary=None, partner_offsets=None):
    """The batch-to-BED loop of the per-site exports: ``batches`` (a generator of the engine over ``cands``: ``motif_sites``,
    ``motif_compare_sites``, ``motif_strand_sites``) are written to the open binary file ``bed_file`` by the native writer ``symbol`` as
    they arrive.  ``partner_offsets``: per candidate the partner offset nm_motif_strands_text takes.
    ``summary``: a list that takes the rows (candidate, contig name, its row of the table) of the batches' ``counts`` in candidate,
    contig order.  Returns (records written, seconds spent in the engine, seconds spent on text)."""
    t_eng = t_text = 0.0
    n_records = 0
    contig_names = [fasta.original_name(n) for n in eng.contig_names]
    t0 = time.perf_counter()
    for sb in batches:
        t1 = time.perf_counter()
        t_eng += t1 - t0
        group = cands[sb.first_candidate:sb.first_candidate + sb.n_candidates]
        if summary is not None and sb.counts is not None:
            for c, (names, table) in zip(group, sb.counts):
                summary += [(c, n, table[i]) for i, n in enumerate(names)]
        rec = sb.records
        if len(rec):
            seg_begin = np.searchsorted(rec["candidate"], np.arange(sb.first_candidate, sb.first_candidate + sb.n_candidates + 1))
            bed_file.write(format_sites(rec["contig"], rec["pos"], rec["code"], seg_begin, [c.name for c in group], [c.bin for c in group],
                                        contig_names, symbol=symbol,
                                        seg_partner_offsets=None if partner_offsets is None else partner_offsets[sb.first_candidate:sb.first_candidate + sb.n_candidates]))
            n_records += len(rec)
        t0 = time.perf_counter()
        t_text += t0 - t1
    return n_records, t_eng + time.perf_counter() - t0, t_text


def export_sites(eng: ScanEngine, cands: list, states, bed_file, max_records=None):
    """Write the sites of ``cands`` (SiteCandidate) to the open binary file ``bed_file``; returns the summary rows
    [(candidate, contig name, int64[6])] in candidate, contig order, and the seconds spent in (engine, text)."""
    batches = eng.motif_sites([c.engine_candidate() for c in cands], states=states, max_records=max_records)
    summary = []
    _, t_eng, t_text = write_site_batches(eng, batches, cands, bed_file, summary=summary)
    return summary, (t_eng, t_text)


def format_summary(summary) -> str:
    rows = []
    for c, contig, six in summary:
        six = [int(x) for x in six]
        rows.append([c.bin, fasta.original_name(contig), c.motif, c.mod_type, c.mod_position] + six + [six[0] + six[3], six[1] + six[4], six[2] + six[5]])
    return table_text(SUMMARY_HEADER, rows)


def candidates_of_files(paths) -> list:
    """The candidates of several bin-motifs.tsv in order; a (bin, motif, mod_type, position) seen before is not repeated."""
    out, seen = [], set()
    for path in paths:
        for c in candidates_of_bin_motifs(path):
            if c.key not in seen:
                seen.add(c.key)
                out.append(c)
    return out


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    states = args.states if isinstance(args.states, tuple) else parse_states(args.states)
    eng, cands, status = open_run("motif_sites", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        known = split_known(cands, eng, eng.slot_of_mod)
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, BED_NAME), "wb") as f:
            summary, (t_eng, t_text) = export_sites(eng, known, states, f)
        t1 = time.perf_counter()
        write_texts(args.out, (SUMMARY_NAME,), (format_summary(summary),))
        finish("motif_sites", TIMINGS, t_eng, t_text + time.perf_counter() - t1, candidates=len(known))
    return 0
