"""``nanomotif motif_sites``: where every motif of a ``bin-motifs.tsv`` occurs on the contigs of its bin, and whether the occurrence
is methylated, unmethylated or without a call.

The reference keeps this view in memory only — ``motif_model_contig(..., save_motif_positions=True)`` (find_motifs_bin.py:1285-1331)
returns index_meth_fwd / index_nonmeth_fwd / index_meth_rev / index_nonmeth_rev for one motif on one contig — and has no command for
it; the no-call class (occurrences found by ``subseq_indices``, utils.py:44-67, that carry neither call) has no counterpart there.

The pileup goes through the ingest path of ``motif_discovery`` (same readers, same pre-filters, same thresholds), so the state planes
are the ones the counts of ``bin-motifs.tsv`` were scored on: the summary's ``n_mod`` / ``n_nomod`` summed over a bin's contigs are the
row's.  (Under non-default thresholds ``motif_discovery`` scores the motifs its merge stage makes on a second classification fixed
at 0.3 / 0.7, find_motifs_bin.py:569; this command exports the classification of the thresholds it is given.)

Files: ``motif-sites.bed`` (contig, start, end, motif_modtype_modposition, 0, strand, state, bin — no header, candidates in
``bin-motifs.tsv`` order, within a candidate contigs in bin order, ascending position, '+' before '-') and
``motif-sites-summary.tsv`` (one row per bin, contig, motif, mod_type, mod_position: the six counts and their sums over the strands).
"""
from __future__ import annotations

import csv
import ctypes as C
import logging as log
import os
import time

import numpy as np

from . import _lib, fasta, pileup as pileup_mod
from .engine import SITE_STATES, ScanEngine
from .motif import MOD_TYPE_TO_CANONICAL, Motif, iupac_to_regex

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


def format_sites(contig, pos, code, seg_begin, seg_names, seg_bins, contig_names, symbol="nm_motif_sites_text") -> bytes:
    """The lines of motif-sites.bed for records (contig, pos, code) cut into runs [seg_begin[s], seg_begin[s + 1]) that share a name
    and a bin (nm_motif_sites_text: native, on up to NM_POST_THREADS threads).  ``symbol``: the writer, nm_motif_compare_text for the
    records of ``ScanEngine.motif_compare_sites`` (switched-sites.bed)."""
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
    args = (n, p(contig, C.c_uint32), p(pos, C.c_uint32), p(code, C.c_uint8), len(seg_names), p(seg_begin, C.c_uint64), b"".join(parts),
            p(seg_off, C.c_uint64), len(cparts), b"".join(cparts), p(c_off, C.c_uint64))
    size = C.c_uint64(0)
    _lib.check(text(*args, None, 0, C.byref(size)))
    buf = np.empty(size.value, dtype=np.uint8)
    _lib.check(text(*args, buf.ctypes.data_as(C.c_void_p), size.value, C.byref(size)))
    return buf.tobytes()


def export_sites(eng: ScanEngine, cands: list, states, bed_file, max_records=None):
    """Write the sites of ``cands`` (SiteCandidate) to the open binary file ``bed_file``; returns the summary rows
    [(candidate, contig name, int64[6])] in candidate, contig order, and the seconds spent in (engine, text)."""
    t_eng = t_text = 0.0
    summary = []
    t0 = time.perf_counter()
    for sb in eng.motif_sites([c.engine_candidate() for c in cands], states=states, max_records=max_records):
        t1 = time.perf_counter()
        t_eng += t1 - t0
        group = cands[sb.first_candidate:sb.first_candidate + sb.n_candidates]
        if sb.counts is not None:
            for c, (names, table) in zip(group, sb.counts):
                summary += [(c, n, table[i]) for i, n in enumerate(names)]
        rec = sb.records
        if len(rec):
            seg_begin = np.searchsorted(rec["candidate"], np.arange(sb.first_candidate, sb.first_candidate + sb.n_candidates + 1))
            bed_file.write(format_sites(rec["contig"], rec["pos"], rec["code"], seg_begin, [c.name for c in group], [c.bin for c in group],
                                        [fasta.original_name(n) for n in eng.contig_names]))
        t0 = time.perf_counter()
        t_text += t0 - t1
    return summary, (t_eng + time.perf_counter() - t0, t_text)


def format_summary(summary) -> str:
    lines = ["\t".join(SUMMARY_HEADER)]
    for c, contig, six in summary:
        six = [int(x) for x in six]
        lines.append("\t".join([c.bin, fasta.original_name(contig), c.motif, c.mod_type, str(c.mod_position)] + [str(x) for x in six]
                               + [str(six[0] + six[3]), str(six[1] + six[4]), str(six[2] + six[5])]))
    return "\n".join(lines) + "\n"


def _open_pileup(eng: ScanEngine, path: str, bin_contig: dict, threads: int):
    """The table of one pileup file: the device-side bedMethyl parser, the host reader where it declines; a bgzip pileup through its
    tabix index for the binned contigs."""
    bgzip = path.endswith(".gz")
    if bgzip and not os.path.exists(path + ".tbi"):
        raise FileNotFoundError(f"Tabix index for {path} not found.")
    wanted = list(dict.fromkeys(fasta.original_name(c) for c in bin_contig)) if bgzip else None
    index = path + ".tbi" if bgzip else None
    table = None
    if os.environ.get("NANOMOTIF_HOST_PARSER") != "1" and not any(fasta.ALIAS_SEP in c for c in bin_contig):
        try:
            table = pileup_mod.DevicePileup(eng, path, threads=threads, contigs=wanted, index_path=index)
        except _lib.NmScanError as e:
            if e.code != _lib.NM_EDECLINED:
                raise
            log.info(f"pileup: the device parser declined ({e}); using the host parser")
    if table is None:
        table = pileup_mod.NativePileup(path, contigs=wanted, index_path=index)
    on_device = isinstance(table, pileup_mod.DevicePileup)
    log.info(f"pileup: {len(table):,} rows ({'device' if on_device else 'host'} parser)")
    return table


def _ingest_table(eng: ScanEngine, table, names: list, args, label_of=None) -> dict:
    """Pre-filters and classification of ``motif_discovery`` for one opened pileup on the resident assembly (``names``: the engine's
    contigs); closes the table.  ``label_of``: mod type -> label of its classification (default: the mod type itself).  Returns the
    ingest's result (``kept``: uint32[n_contigs, 8] surviving rows per contig and mod code) — the engine's own ingest tables speak about
    the LAST pileup only."""
    label_of = label_of or (lambda mt: mt)
    t0 = time.perf_counter()
    on_device = isinstance(table, pileup_mod.DevicePileup)
    local_id = {c: i for i, c in enumerate(names)}
    lut = np.array([local_id.get(n, 0xFFFFFFFF) for n in table.contig_names], dtype=np.uint32)
    labels = {i: (label_of(mt), MOD_TYPE_TO_CANONICAL[mt]) for i, mt in enumerate(pileup_mod.MOD_TYPES)}
    low, high = args.methylation_threshold_low, args.methylation_threshold_high
    part_rows = int(os.environ.get("NANOMOTIF_INGEST_PART_ROWS", 250_000_000))
    if on_device:
        res = eng.ingest_device_pileup(table, lut, labels, low=low, high=high, max_part_rows=part_rows)
    else:
        # further placements of a contig listed under several bins: the contig's rows once more per placement
        file_id = {n: i for i, n in enumerate(table.contig_names)}
        placements = [(file_id[fasta.original_name(c)], local_id[c]) for c in names
                      if fasta.ALIAS_SEP in c and fasta.original_name(c) in file_id]
        file_contig = table.file_contig_column().copy() if placements else None
        cols = table.ingest_columns(lut)
        extra = []
        for fid, local in placements:
            sel = np.flatnonzero(file_contig == fid)
            extra.append(dict(contig=np.full(len(sel), local, np.uint32),
                              **{k: cols[k][sel] for k in ("position", "mod_type", "strand", "fraction_mod", "nvalid_cov")}))
        res = eng.ingest_pileup(cols["contig"], cols["position"], cols["mod_type"], cols["strand"], cols["fraction_mod"], cols["nvalid_cov"],
                                labels, low=low, high=high, want_rows=False, max_part_rows=part_rows, extra_parts=extra)
        del cols
    table.close()
    log.info(f"pileup: {res['n_kept']:,} rows after the device-side filters")
    res["seconds"] = time.perf_counter() - t0
    return res


def load_engine(args, device: int, pileups=None) -> ScanEngine:
    """Assembly and pileup of the command line -> an engine whose state planes are ``motif_discovery``'s: the readers, the contig
    selection, the pre-filters and the classification of ``main.find_motifs_bin`` on one GPU (device-side FASTA and bedMethyl
    parsers, the host readers where those decline; a bgzip pileup through its tabix index for the binned contigs).
    ``pileups``: [(path, label_of), ...] to make several pileups resident on the one assembly, each under its own labels (default: the
    one pileup of ``args.pileup`` under the mod types' names); ``eng.pileup_ingests`` holds the result of each ingest in that order
    (``seconds``: reading and ingesting that pileup)."""
    pileups = [(str(args.pileup), None)] if pileups is None else [(str(p), f) for p, f in pileups]
    bin_contig = fasta.generate_contig_bin(args)
    if not bin_contig:
        raise ValueError("No bin contig mapping found")
    threads = max(args.threads, 0) if getattr(args, "threads", 1) > 1 else 0
    eng = ScanEngine(device)
    assembly = None
    try:
        device_fasta = not str(args.assembly).endswith(".gz") and os.environ.get("NANOMOTIF_HOST_FASTA") != "1"
        assembly = fasta.DeviceAssembly(eng, args.assembly, threads=threads) if device_fasta else fasta.load_fasta(args.assembly)
        fasta.add_alias_sequences(assembly, bin_contig)
        bin_contig = {c: b for c, b in bin_contig.items() if c in assembly}
        if not bin_contig:
            raise ValueError("No contigs remain in bin_contig after filtering against the assembly")
        t0 = time.perf_counter()
        table = _open_pileup(eng, pileups[0][0], bin_contig, threads)
        t_open = time.perf_counter() - t0
        names = list(bin_contig)
        all_bins = sorted(set(bin_contig.values()))
        if device_fasta:
            eng.upload_assembly_fasta(assembly, names, [bin_contig[c] for c in names], bin_names=all_bins)
        else:
            eng.upload_assembly(names, [assembly[c] for c in names], [bin_contig[c] for c in names], bin_names=all_bins)
        eng.pileup_ingests = [_ingest_table(eng, table, names, args, pileups[0][1])]
        eng.pileup_ingests[0]["seconds"] += t_open
        for path, label_of in pileups[1:]:
            t0 = time.perf_counter()
            table = _open_pileup(eng, path, bin_contig, threads)
            t_open = time.perf_counter() - t0
            eng.pileup_ingests.append(_ingest_table(eng, table, names, args, label_of))
            eng.pileup_ingests[-1]["seconds"] += t_open
        return eng
    except BaseException:
        eng.close()
        raise
    finally:
        if assembly is not None and hasattr(assembly, "close"):
            assembly.close()


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    TIMINGS.clear()
    if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
        log.error("motif_sites runs on one GPU: start it without a multi-rank launcher (WORLD_SIZE is %s)", os.environ["WORLD_SIZE"])
        return 2
    states = args.states if isinstance(args.states, tuple) else parse_states(args.states)
    cands = candidates_of_bin_motifs(args.bin_motifs)
    log.info(f"{len(cands)} (bin, motif) candidates from {args.bin_motifs}")
    device = args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0") or 0)
    t0 = time.perf_counter()
    try:
        eng = load_engine(args, device)
    except _lib.NmScanError as e:
        raise RuntimeError(f"nanomotif_amd needs an AMD GPU (MI355X); there is no CPU fallback ({e})") from e
    TIMINGS["ingest_s"] = time.perf_counter() - t0
    try:
        known = [c for c in cands if c.bin in eng.bin_index and c.mod_type in eng.slot_of_mod]
        for c in cands:
            if c.bin not in eng.bin_index:
                log.warning(f"{c!r}: the bin has no contig in the assembly; skipped")
            elif c.mod_type not in eng.slot_of_mod:
                log.warning(f"{c!r}: the pileup holds no rows of mod type {c.mod_type}; skipped")
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, BED_NAME), "wb") as f:
            summary, (t_eng, t_text) = export_sites(eng, known, states, f)
        t1 = time.perf_counter()
        with open(os.path.join(args.out, SUMMARY_NAME), "w") as f:
            f.write(format_summary(summary))
        TIMINGS.update(kernels_s=t_eng, text_s=t_text + time.perf_counter() - t1, candidates=len(known))
        log.info(f"motif_sites: ingest {TIMINGS['ingest_s']:.2f}s, engine {t_eng:.2f}s, text {TIMINGS['text_s']:.2f}s")
    finally:
        eng.close()
    return 0
