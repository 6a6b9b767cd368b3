"""Files -> engine: the one path by which a pileup is opened, pre-filtered and classified on a resident assembly.  ``motif_discovery``
(``main.find_motifs_bin``) and the site exports (``load_engine``: motif_sites, motif_coverage, motif_compare) both go through
``open_pileup`` and ``PileupIngest``, so the exports' state planes are the ones the counts of ``bin-motifs.tsv`` were scored on."""
from __future__ import annotations

import logging as log
import os
import threading
import time

import numpy as np

from . import _lib, fasta, pileup as pileup_mod
from .engine import SHIFT_SLOT_B, ScanEngine
from .motif import MOD_TYPE_TO_CANONICAL


def parser_threads(args) -> int:
    """Threads of the native parsers for ``--threads`` (0: the library's default)."""
    threads = getattr(args, "threads", 1)
    return max(threads, 0) if threads > 1 else 0


def wanted_contigs(path: str, contigs):
    """The contigs a bgzip pileup is read for through its tabix index (aliased placements under their contig's name, each once);
    None for a plain file, which is read whole (find_motifs_bin.py:233-246 fetches per bin)."""
    return list(dict.fromkeys(fasta.original_name(c) for c in contigs)) if str(path).endswith(".gz") else None


def open_pileup(eng: ScanEngine, path: str, wanted, bin_contig, threads: int, plan=None):
    """The table of one pileup file.  It is parsed ON THE GPU (``DevicePileup``, nm_bed_parse_device: the host only moves the file
    through pinned slabs — the BGZF blocks of a bgzip file are inflated into them by the copy threads, the tabix subset alike; every
    row equals the host parser's bit for bit); a gzip stream that is not bgzip (the device parser declines), a contig listed under
    several bins (its rows are needed twice) and NANOMOTIF_HOST_PARSER=1 take the host parser (``NativePileup``: raw rows kept in
    native memory).  ``wanted``: ``wanted_contigs`` of the binned contigs the assembly holds.  ``plan``: a ``BedPlan`` made ahead for
    exactly ``wanted``; it is this call's to close — at once when the call fails, else on a thread of its own (closing the plan
    unmaps the pileup: 3.5 million page-table entries at 1 Gbp — off the critical path).  The caller logs what was read."""
    index = path + ".tbi" if path.endswith(".gz") else None
    try:
        if index is not None and not os.path.exists(index):
            raise FileNotFoundError(f"Tabix index for {path} not found.")     # find_motifs_bin.py:383-384
        table = None
        if os.environ.get("NANOMOTIF_HOST_PARSER") != "1" and not any(fasta.ALIAS_SEP in c for c in bin_contig):
            try:
                table = pileup_mod.DevicePileup(eng, path, threads=threads, contigs=wanted, index_path=index, plan=plan)
            except _lib.NmScanError as e:
                if e.code != _lib.NM_EDECLINED:
                    raise
                log.info(f"pileup: the device parser declined ({e}); using the host parser")
        if table is None:
            table = pileup_mod.NativePileup(path, contigs=wanted, index_path=index)
    except BaseException:
        if plan is not None:                     # a final error of the parser: the plan's mapping goes back now
            plan.close()
        raise
    if plan is not None:
        threading.Thread(target=plan.close, name="nm-bed-plan-close", daemon=False).start()
    return table


class PileupIngest:
    """An opened pileup on its way into the resident assembly (``names``: the engine's contigs, in its order): the contig look-up
    table, the host parser's columns and the further placements of a contig listed under several bins are made once; every
    ``classify`` runs the three pre-filters and one classification over them (rows of contigs that are in no bin or on another rank
    are ignored: the reference joins with contig -> bin after filtering, find_motifs_bin.py:416)."""

    def __init__(self, eng: ScanEngine, table, names: list):
        self.eng, self.table = eng, table
        self.on_device = isinstance(table, pileup_mod.DevicePileup)
        local_id = {c: i for i, c in enumerate(names)}
        self.lut = np.array([local_id.get(n, 0xFFFFFFFF) for n in table.contig_names], dtype=np.uint32)
        # further placements of a contig listed under several bins: the contig's rows once more per placement
        file_id = {n: i for i, n in enumerate(table.contig_names)}
        placements = [(file_id[fasta.original_name(c)], local_id[c]) for c in names
                      if fasta.ALIAS_SEP in c and fasta.original_name(c) in file_id]
        file_contig = table.file_contig_column().copy() if placements else None
        self.cols = None if self.on_device else table.ingest_columns(self.lut)    # views in the engine's types; refuses positions >= 4 Gbp
        self.extra = []
        for fid, local in placements:
            sel = np.flatnonzero(file_contig == fid)
            self.extra.append(dict(contig=np.full(len(sel), local, np.uint32),
                                   **{k: self.cols[k][sel] for k in ("position", "mod_type", "strand", "fraction_mod", "nvalid_cov")}))
        # large pileups go to the device in parts of whole contigs (bounds the memory of the raw rows and filter scratch)
        self.part_rows = int(os.environ.get("NANOMOTIF_INGEST_PART_ROWS", 250_000_000))

    def classify(self, label_of, low: float, high: float) -> dict:
        """Pre-filters and classification at ``low`` / ``high``; ``label_of``: mod type -> label its classification is resident
        under.  Returns the ingest's result (``kept``: uint32[n_contigs, 8] surviving rows per contig and mod code) — the engine's own
        ingest tables speak about the LAST classification only."""
        labels = {i: (label_of(mt), MOD_TYPE_TO_CANONICAL[mt]) for i, mt in enumerate(pileup_mod.MOD_TYPES)}
        if self.on_device:
            return self.eng.ingest_device_pileup(self.table, self.lut, labels, low=low, high=high, max_part_rows=self.part_rows)
        c = self.cols
        return self.eng.ingest_pileup(c["contig"], c["position"], c["mod_type"], c["strand"], c["fraction_mod"], c["nvalid_cov"], labels,
                                      low=low, high=high, want_rows=False, max_part_rows=self.part_rows, extra_parts=self.extra)

    def close(self):
        """Releases the table (the columns are views into it)."""
        self.cols, self.extra = None, []
        self.table.close()


def upload_assembly(eng: ScanEngine, assembly, names: list, bins: list, bin_names: list):
    """``names`` of ``assembly`` (a ``fasta.DeviceAssembly``, or the dict of the host reader) become the engine's contigs, each in its
    bin of ``bins``; ``bin_names``: every bin of the run (bin ids must be identical on every rank)."""
    if isinstance(assembly, fasta.DeviceAssembly):
        eng.upload_assembly_fasta(assembly, names, bins, bin_names=bin_names)
    else:
        eng.upload_assembly(names, [assembly[c] for c in names], bins, bin_names=bin_names)


def open_assembly(eng: ScanEngine, args, bin_contig: dict, threads: int):
    """The assembly of the command line, read by the device FASTA parser (a gzip file and NANOMOTIF_HOST_FASTA=1: the host reader), with
    the aliased placements of ``bin_contig`` added.  Returns (assembly, the entries of ``bin_contig`` whose contig the assembly holds);
    the assembly is the caller's to close when it has a ``close``."""
    device_fasta = not str(args.assembly).endswith(".gz") and os.environ.get("NANOMOTIF_HOST_FASTA") != "1"
    assembly = fasta.DeviceAssembly(eng, args.assembly, threads=threads) if device_fasta else fasta.load_fasta(args.assembly)
    try:
        fasta.add_alias_sequences(assembly, bin_contig)
        bin_contig = {c: b for c, b in bin_contig.items() if c in assembly}
        if not bin_contig:
            raise ValueError("No contigs remain in bin_contig after filtering against the assembly")
    except BaseException:
        if hasattr(assembly, "close"):
            assembly.close()
        raise
    return assembly, bin_contig


def load_engine(args, device: int, pileups=None) -> ScanEngine:
    """Assembly and pileup of the command line -> an engine whose state planes are ``motif_discovery``'s on one GPU: the readers
    (device-side FASTA and bedMethyl parsers, the host readers where those decline; a bgzip pileup through its tabix index for the
    binned contigs), the contig selection, the pre-filters and the classification ``main.find_motifs_bin`` goes through.
    ``pileups``: [(path, label_of), ...] to make several pileups resident on the one assembly, each under its own labels (default: the
    one pileup of ``args.pileup`` under the mod types' names); ``eng.pileup_ingests`` holds the result of each ingest in that order
    (``seconds``: reading and ingesting that pileup)."""
    pileups = [(str(args.pileup), None)] if pileups is None else [(str(p), f) for p, f in pileups]
    bin_contig = fasta.generate_contig_bin(args)
    if not bin_contig:
        raise ValueError("No bin contig mapping found")
    threads = parser_threads(args)
    eng = ScanEngine(device)
    assembly = None
    try:
        assembly, bin_contig = open_assembly(eng, args, bin_contig, threads)
        names = list(bin_contig)
        eng.pileup_ingests = []
        for path, label_of in pileups:
            t0 = time.perf_counter()
            table = open_pileup(eng, path, wanted_contigs(path, bin_contig), bin_contig, threads)
            log.info(f"pileup: {len(table):,} rows ({'device' if isinstance(table, pileup_mod.DevicePileup) else 'host'} parser)")
            t_open = time.perf_counter() - t0
            if not eng.pileup_ingests:           # (the first pileup is opened beside the parsed assembly, before its planes are packed)
                upload_assembly(eng, assembly, names, [bin_contig[c] for c in names], sorted(set(bin_contig.values())))
            t0 = time.perf_counter()
            ingest = PileupIngest(eng, table, names)
            res = ingest.classify(label_of or (lambda mt: mt), args.methylation_threshold_low, args.methylation_threshold_high)
            ingest.close()
            log.info(f"pileup: {res['n_kept']:,} rows after the device-side filters")
            res["seconds"] = time.perf_counter() - t0 + t_open
            eng.pileup_ingests.append(res)
        return eng
    except BaseException:
        eng.close()
        raise
    finally:
        if assembly is not None and hasattr(assembly, "close"):
            assembly.close()


def kept_mod_types(eng: ScanEngine) -> list:
    """The mod types of which at least one ingest of ``eng.pileup_ingests`` kept a pileup row on a resident contig, in slot order
    (``load_engine`` gives every known mod code a slot; a slot no row went into is not a mod type of these pileups)."""
    kept = [np.asarray(r["kept"]) for r in eng.pileup_ingests]
    present = {mt for code, mt in enumerate(pileup_mod.MOD_TYPES) if any(k[:, code].any() for k in kept)}
    return [mt for mt in sorted((m for m in pileup_mod.MOD_TYPES if m in eng.slot_of_mod), key=eng.slot_of_mod.get) if mt in present]


class AliasedContigs(ValueError):
    """A contig is listed under several bins where the command cannot serve that (``load_readstats_engine``)."""


def load_readstats_engine(args, device: int, mod_types, pileups=None) -> ScanEngine:
    """Assembly and pileup of the command line -> an engine that holds the BINNED assembly exactly as ``load_engine`` puts it (same
    readers, the binned contigs the assembly holds, the run's bins) and the READ STATISTICS of ``mod_types`` (the mod codes wanted) in
    place of the state planes: every pileup record with ``n_valid_cov >= args.min_valid_read_coverage`` and ``n_valid_cov / (n_valid_cov
    + n_diff) >= args.min_valid_cov_to_diff_fraction`` keeps its (n_valid_cov, n_modified).  The pileup goes through
    ``contig_methylation.read_statistics_device`` (parsed on the device, one upload per mod code from the parser's columns), or
    ``read_statistics_host`` when the device parser declines or NANOMOTIF_HOST_PARSER=1; pileup contigs outside the bins are ignored.
    ``eng.readstats_kept``: mod code -> records kept.  ``pileups``: the paths to read, default the one of ``args.pileup``; a second path
    (sample B of ``motif_shift``) goes to the slots from ``engine.SHIFT_SLOT_B`` on the same assembly and its records kept to
    ``eng.readstats_kept_b``, ``eng.readstats_kept`` stays sample A's.  A contig listed under several bins would need its rows twice in one
    upload: ``AliasedContigs`` names it before any device is touched."""
    from . import contig_methylation as cm
    bin_contig = fasta.generate_contig_bin(args)
    if not bin_contig:
        raise ValueError("No bin contig mapping found")
    aliased = sorted({fasta.original_name(c) for c in bin_contig if fasta.ALIAS_SEP in c})
    if aliased:
        raise AliasedContigs(f"{len(aliased)} contig(s) are listed under several bins (e.g. {aliased[0]}): the read statistics hold a pileup row once, "
                             "so a contig cannot be read in two bins of one run; list it under one bin")
    threads = parser_threads(args)
    eng = ScanEngine(device)
    assembly = None
    try:
        assembly, bin_contig = open_assembly(eng, args, bin_contig, threads)
        names = list(bin_contig)
        upload_assembly(eng, assembly, names, [bin_contig[c] for c in names], sorted(set(bin_contig.values())))
        if hasattr(assembly, "close"):
            assembly.close()
        assembly = None
        local = {c: i for i, c in enumerate(names)}
        wanted = set(mod_types)
        filters = (int(args.min_valid_read_coverage), float(args.min_valid_cov_to_diff_fraction))
        paths = [args.pileup] if pileups is None else list(pileups)
        if not 1 <= len(paths) <= 2:
            raise ValueError("the read statistics hold one or two pileups")
        both = []
        for path, base in zip(paths, (0, SHIFT_SLOT_B)):
            kept, more = None, ({"slot_base": base} if base else {})       # (the first pileup is read exactly as ever)
            if os.environ.get("NANOMOTIF_HOST_PARSER") != "1":
                try:
                    kept = cm.read_statistics_device(eng, eng.lib, path, threads, local, wanted, True, *filters, **more)
                    log.info("pileup: read statistics from the device parser's columns")
                except _lib.NmScanError as e:
                    if e.code != _lib.NM_EDECLINED:
                        raise
                    log.info(f"pileup: the device parser declined ({e}); using the host parser")
            if kept is None:
                kept = cm.read_statistics_host(eng, eng.lib, path, getattr(args, "threads", 1), local, wanted, True, *filters, **more)
                log.info("pileup: read statistics from the host parser's rows")
            both.append(kept)
        eng.readstats_kept = both[0]
        if len(both) == 2:
            eng.readstats_kept_b = both[1]
        return eng
    except BaseException:
        eng.close()
        raise
    finally:
        if assembly is not None and hasattr(assembly, "close"):
            assembly.close()
