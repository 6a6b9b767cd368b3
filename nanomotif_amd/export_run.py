"""What the ``run(args)`` of the export commands (``motif_sites`` ... ``motif_pileup``) have in common, once: how a command opens
(the refusal of a multi-rank launch, the candidates of ``--bin_motifs``, the loaded engine, ``ingest_s``), the split of the candidates
into known and skipped with its two warnings, the one-letter background candidates, the tail (files, ``TIMINGS``, the log line) and the
small text helpers of the tables.  A command keeps its file names, headers, ``format_files``, statistics and its ``TIMINGS`` dict."""
from __future__ import annotations

import logging as log
import os
import time
from contextlib import closing                      # ``with closing(eng):`` — the engine is closed on every path out of a command

from . import _lib
from .loading import AliasedContigs, load_engine, load_readstats_engine
from .motif import MOD_TYPE_TO_CANONICAL, Motif

READ_FILTER_SUFFIX = " that pass the read filters"  # the second warning of the commands that read the read statistics


# ------------------------------------------------------------------------------------------------ text helpers
def table_text(header, rows) -> str:
    """A tab-separated table as text: the header line, then one line per row."""
    return "\n".join(["\t".join(header)] + ["\t".join(str(x) for x in r) for r in rows]) + "\n"


def frac_text(n_mod: int, n_nomod: int) -> str:
    """n_mod / (n_mod + n_nomod) as ``%.6f``; empty when nothing is called."""
    called = int(n_mod) + int(n_nomod)
    return "%.6f" % (int(n_mod) / called) if called else ""


def share_text(n: int, total: int) -> str:
    """n / total as ``%.6f``; empty when the total is 0."""
    return "%.6f" % (int(n) / int(total)) if int(total) else ""


def parse_int_in(option: str, value, low: int, high=None, what=None, step=1) -> int:
    """An integer option in [low, high] (no upper end: ``high`` None) that is a multiple of ``step``; ValueError "<option> takes <what>;
    got <value>" otherwise.  ``what``: default "an integer in low..high" / "an integer of at least low"."""
    try:
        v = int(str(value).strip())
        if v >= low and (high is None or v <= high) and v % step == 0:
            return v
    except ValueError:
        pass
    what = what or (f"an integer in {low}..{high}" if high is not None else f"an integer of at least {low}")
    raise ValueError(f"{option} takes {what}; got {value!r}")


# ------------------------------------------------------------------------------------------------ the opening
def run_device(args) -> int:
    """The GPU of a run: ``--device``, else LOCAL_RANK, else 0."""
    return args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0") or 0)


def open_candidates(command: str, args, timings: dict):
    """How every export command opens, before anything is loaded: the refusal of a multi-rank launch and the candidates of
    ``--bin_motifs`` (one file or several).  Returns (candidates, the GPU to use, 0), or (None, None, the exit status) when the command
    does not run."""
    from .motif_sites import candidates_of_files                          # (motif_sites imports this module: the reader is about sites)
    timings.clear()
    if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
        log.error("%s runs on one GPU: start it without a multi-rank launcher (WORLD_SIZE is %s)", command, os.environ["WORLD_SIZE"])
        return None, None, 2
    files = [args.bin_motifs] if isinstance(args.bin_motifs, str) else list(args.bin_motifs)
    cands = candidates_of_files(files)
    log.info(f"{len(cands)} (bin, motif) candidates from {', '.join(files)}")
    return cands, run_device(args), 0


def _open(command: str, args, timings: dict, load, with_candidates=True):
    """``open_candidates`` (unless ``with_candidates`` is False: no refusal, no candidates), then ``load(candidates, device)`` -> the
    engine, timed as ``timings["ingest_s"]``.  Returns (engine, candidates, 0) or (None, None, the exit status)."""
    if with_candidates:
        cands, device, status = open_candidates(command, args, timings)
        if cands is None:
            return None, None, status
    else:
        timings.clear()
        cands, device = None, run_device(args)
    t0 = time.perf_counter()
    try:
        eng = load(cands, device)
    except AliasedContigs as e:
        log.error(f"{command}: {e}")
        return None, None, 2
    except _lib.NmScanError as e:
        raise RuntimeError(f"nanomotif_amd needs an AMD GPU (MI355X); there is no CPU fallback ({e})") from e
    timings["ingest_s"] = time.perf_counter() - t0
    return eng, cands, 0


def open_run(command: str, args, timings: dict, pileups=None, with_candidates=True):
    """How the export commands that read the state planes open: ``open_candidates``, the loaded engine (``loading.load_engine`` with
    ``pileups``) and ``timings["ingest_s"]``.  Returns (engine, candidates, 0), or (None, None, the exit status) when the command does
    not run.  ``with_candidates`` False (``motif_kmers`` without ``--bin_motifs``): the engine alone — and, as nothing is opened before
    it, no refusal of a multi-rank launch."""
    return _open(command, args, timings, lambda cands, device: load_engine(args, device, pileups), with_candidates)


def open_readstats_run(command: str, args, timings: dict, pileups=None):
    """``open_run`` for the commands that read the READ STATISTICS (``loading.load_readstats_engine`` of the candidates' mod codes, with
    ``pileups``: default the one of ``args.pileup``); a contig listed under several bins is logged as an error of ``command`` and ends it
    with status 2."""
    from .contig_methylation import MOD_CODES
    return _open(command, args, timings,
                 lambda cands, device: load_readstats_engine(args, device, sorted({c.mod_type for c in cands if c.mod_type in MOD_CODES}),
                                                            **({} if pileups is None else {"pileups": pileups})))


# ------------------------------------------------------------------------------------------------ known and skipped
def readstats_mod_types(eng) -> set:
    """The mod types of which the read statistics kept a record."""
    return {mt for mt, n in eng.readstats_kept.items() if n}


def split_known(cands, eng, mod_types, suffix="", wording="the pileup holds no rows") -> list:
    """The candidates of ``cands`` whose bin has a contig in the assembly and whose mod type is among ``mod_types``, in file order; every
    other one is named in a warning.  ``suffix`` / ``wording``: how the second warning reads for the command."""
    known = []
    for c in cands:
        if c.bin not in eng.bin_index:
            log.warning(f"{c!r}: the bin has no contig in the assembly; skipped")
        elif c.mod_type not in mod_types:
            log.warning(f"{c!r}: {wording} of mod type {c.mod_type}{suffix}; skipped")
        else:
            known.append(c)
    return known


# ------------------------------------------------------------------------------------------------ background
def resident_bins(eng) -> list:
    """The bins with a contig in the assembly, sorted."""
    return sorted(b for b in eng.bin_index if eng.bin_contigs(b))


def bin_mod_keys(eng, mod_types) -> list:
    """[(bin, mod type)]: every bin with a contig, sorted, x ``mod_types`` in the order given."""
    return [(b, mt) for b in resident_bins(eng) for mt in mod_types]


def background_keys(cands) -> list:
    """[(bin, mod type)] of the background candidates: per bin in order of first appearance, the mod types present among its candidates."""
    keys = []
    for c in cands:
        if (c.bin, c.mod_type) not in keys:
            keys.append((c.bin, c.mod_type))
    return keys


def background_candidates(keys) -> list:
    """The one-letter engine candidates "canonical base at position 0" of (bin, mod type) ``keys``: every position that can carry the
    modification, the background a motif is read against."""
    return [(Motif(MOD_TYPE_TO_CANONICAL[mt], 0), mt, b) for b, mt in keys]


# ------------------------------------------------------------------------------------------------ the tail
def write_texts(out: str, names, texts):
    """``texts`` into the files ``names`` of the folder ``out``; a text that is None has no file."""
    for name, text in zip(names, texts):
        if text is not None:
            with open(os.path.join(out, name), "w") as f:
                f.write(text)


def finish(command: str, timings: dict, t_eng: float, t_text: float, label="text", ingest="", **counts):
    """The end of a run: ``kernels_s``, ``text_s`` and the command's ``counts`` into ``timings``, and the log line.  ``label``: what the
    second phase is called; ``ingest``: text behind the ingest's seconds."""
    timings.update(kernels_s=t_eng, text_s=t_text, **counts)
    log.info(f"{command}: ingest {timings['ingest_s']:.2f}s{ingest}, engine {t_eng:.2f}s, {label} {t_text:.2f}s")
