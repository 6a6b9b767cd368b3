"""``nanomotif motif_discovery`` on the MI355X engine (reference: nanomotif/main.py:18-104, 298-321).

Single GPU:   python -m nanomotif_amd motif_discovery ASSEMBLY PILEUP -c CONTIG_BIN --out OUT
Several GPUs: python -m torch.distributed.run --nproc-per-node N -m nanomotif_amd motif_discovery ...
              (contigs are sharded over the ranks, count tables are all-reduced over RCCL, rank 0 writes the output)
"""
from __future__ import annotations

import json
import logging as log
import os
import random
import sys
import threading
import time
import warnings
from pathlib import Path

import numpy as np

from . import _lib, fasta, pileup as pileup_mod, postprocess
from .argparser import __version__, create_parser
from .find_motifs_bin import FilteredPileup, ProcessorConfig, allreduce_counts, discover, engine_scorer, use_native_allreduce
from .engine import MAX_DEVICE_WINDOW_WIDTH, ScanEngine
from .loading import PileupIngest, open_pileup, parser_threads, upload_assembly, wanted_contigs
from .motif import MOD_TYPE_TO_CANONICAL
from .shard import assign_bins, assign_contigs

HEADER = "\t".join(postprocess.HEADER) + "\n"


def set_seed(seed=42):
    random.seed(seed)
    np.random.seed(seed)


def shared_setup(args, working_dir, rank=0):
    """main.py:18-43: output directory, logs/, args.<command>.json, seeds."""
    if not os.path.exists(args.out):
        os.makedirs(args.out, exist_ok=True)
    elif rank == 0:
        log.warning(f"Output directory {args.out} already exists")
    log_dir = working_dir + "/logs"
    Path(log_dir).mkdir(parents=True, exist_ok=True)
    handlers = [log.StreamHandler(sys.stdout)]
    if rank == 0:
        handlers.append(log.FileHandler(log_dir + f"/{args.command}.main.log"))
    log.basicConfig(level=log.DEBUG if args.verbose else log.INFO, handlers=handlers, force=True,
                    format="%(asctime)s - %(levelname)s - %(message)s")
    warnings.filterwarnings("ignore")
    log.info(f"nanomotif (MI355X build) version: {__version__}")
    if rank == 0:
        with open(working_dir + f"/args.{args.command}.json", "w") as f:
            json.dump(vars(args), f, indent=2)
    set_seed(args.seed)


TIMINGS = {}          # seconds per phase of the last find_motifs_bin call in this process (written to OUT/logs/timings.*.json)


class _Laps:
    """``lap(name)`` adds the time since the lap before (or ``start``) to ``TIMINGS[key.format(name)]``."""

    def __init__(self, key="{}", start=None):
        self.key, self.t = key, time.perf_counter() if start is None else start

    def __call__(self, name):
        now = time.perf_counter()
        key = self.key.format(name)
        TIMINGS[key] = TIMINGS.get(key, 0.0) + now - self.t
        self.t = now


def _start_distributed(device):
    """The process group of a multi-rank run; returns torch.distributed.  torch is plumbing for the multi-rank run only (process
    group, RCCL); a single-GPU run never imports it."""
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise RuntimeError("nanomotif_amd needs an AMD GPU (MI355X); there is no CPU fallback")
    torch.cuda.set_device(device)
    if not dist.is_initialized():
        # RCCL unless NANOMOTIF_DIST_BACKEND=gloo (debugging aid: lets several ranks share one GPU with --device)
        backend = os.environ.get("NANOMOTIF_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group(backend)
    return dist


class _EngineStart:
    """The HIP runtime takes 0.1-0.3 s to come up in a fresh process: it does so on a side thread while the main one reads the
    contig-bin table and parses the assembly (native code, the interpreter lock is released).  Fails loudly without a GPU: there is
    no CPU fallback."""

    def __init__(self, device):
        self.device, self.eng, self.error = device, None, None
        self.thread = threading.Thread(target=self._start, name="nm-engine-start")
        self.thread.start()

    def _start(self):
        try:
            # large device blocks stay with the process when the library frees them (nm_block_cache: memory another process used is
            # scrubbed by the driver on its way back in — the pre-filters' state planes waited 0.19 s for that at 1 Gbp — and hipFree
            # synchronises the device); NANOMOTIF_BLOCK_CACHE_GB=0 turns it off
            early = None
            if _lib.early_engine_thread is not None:     # (__main__.py: the context may exist already, made beside the imports)
                _lib.early_engine_thread.join()
                _lib.early_engine_thread, early, _lib.early_engine = None, _lib.early_engine, None
                if _lib.early_pin_thread is not None:
                    _lib.early_pin_thread.join()
                    _lib.early_pin_thread = None
            cache_gb = float(os.environ.get("NANOMOTIF_BLOCK_CACHE_GB", "16"))
            if early is not None and early[0] != self.device:
                _lib.load().nm_ctx_destroy(early[1])     # (another --device than the command line showed at a glance)
                early = None
            if cache_gb > 0 and not (early is not None and early[2]):
                _lib.use_block_cache(int(cache_gb * (1 << 30)))
            self.eng = ScanEngine(self.device, ctx=early[1]) if early is not None else ScanEngine(self.device)
            TIMINGS["engine_context_made_beside_the_imports"] = early is not None
        except BaseException as e:               # re-raised on the main thread by engine()
            self.error = e

    def engine(self) -> ScanEngine:
        self.thread.join()
        if self.error is not None:
            if isinstance(self.error, _lib.NmScanError):
                raise RuntimeError(f"nanomotif_amd needs an AMD GPU (MI355X); there is no CPU fallback ({self.error})") from self.error
            raise self.error
        return self.eng

    def abandon(self):
        """An error before the engine was put to use: whatever came up is closed."""
        self.thread.join()
        if self.eng is not None:
            self.eng.close()


class _PlanAhead:
    """A bgzip pileup: the host-only half of its indexed parse (tabix index, the walk over the BGZF blocks: half a second at 1 Gbp)
    starts NOW on a thread, for the contigs the bin table names — beside the HIP runtime coming up and the assembly being parsed.
    ``take(wanted)`` hands the plan out when the assembly turns out to hold them all (else it is closed: ``open_pileup`` plans again
    for the ones it holds)."""

    def __init__(self, path: str, bin_contig: dict, threads: int):
        self.thread = self.plan = self.error = None
        if path.endswith(".gz") and os.path.exists(path + ".tbi") and os.environ.get("NANOMOTIF_HOST_PARSER") != "1" \
                and not any(fasta.ALIAS_SEP in c for c in bin_contig) and os.environ.get("NANOMOTIF_NO_PREPLAN") != "1":
            guess = wanted_contigs(path, bin_contig)

            def make_plan():
                try:
                    self.plan = pileup_mod.BedPlan(path, path + ".tbi", guess, threads=threads)
                except BaseException as e:       # (the regular path will meet the same problem and report it)
                    self.error = e
            self.thread = threading.Thread(target=make_plan, name="nm-bed-plan")
            self.thread.start()

    def take(self, wanted):
        """The plan when it was made for exactly ``wanted``, else None; the thread is waited for (it is not a daemon: the process
        would wait for its half-second walk at exit anyway) and a plan not handed out releases its mapping of the pileup now, not by
        a finaliser."""
        if self.thread is not None:
            self.thread.join()
        plan, self.thread, self.plan = self.plan, None, None
        if self.error is not None:
            log.debug(f"the pre-planned indexed parse failed (the regular path reports the cause): {self.error!r}")
            self.error = None
        if plan is not None and (wanted is None or list(plan.contigs) != list(wanted)):
            plan.close()                         # the assembly lacks some of the binned contigs: plan again for the ones it holds
            plan = None
        return plan

    def drop(self):
        """An error path between the plan thread's start and its use."""
        self.take(None)


def _native_communicator_up(eng, dist, rank, world, device) -> bool:
    """Whether EVERY rank has the C ABI's own RCCL communicator up, so that the per-round count tables can travel through it
    (nm_allreduce_counts_host); torch.distributed only carries the 128-byte id to the ranks.  Every rank must end up on the SAME path.
    What is guaranteed: a rank on which librccl does not load says so BEFORE anybody enters ncclCommInitRank (every rank makes a unique
    id as a probe; MIN all-reduce), and a rank whose ncclCommInitRank RETURNS an error says so after it (second MIN all-reduce) — the
    run then falls back to torch.distributed as a whole.  What no agreement can cover is a rank that never arrives inside the
    collective init (it died, or hangs): the others would wait there for ever, so the init runs under a watchdog that ends this
    process with a message (NANOMOTIF_COMM_TIMEOUT seconds, default 300)."""
    import torch

    def comm_init_watched(uid):
        limit = float(os.environ.get("NANOMOTIF_COMM_TIMEOUT", "300"))
        done = threading.Event()

        def watchdog():
            if not done.wait(limit):
                sys.stderr.write(f"rank {rank}: nm_comm_init did not return within {limit:.0f} s (a rank missing from ncclCommInitRank?): "
                                 "giving up; NANOMOTIF_ALLREDUCE=torch takes torch.distributed instead\n")
                sys.stderr.flush()
                os._exit(3)
        threading.Thread(target=watchdog, name="nm-comm-watchdog", daemon=True).start()
        try:
            eng.comm_init(rank, world, uid)
        finally:
            done.set()

    def agreed(ok_here: int) -> bool:
        flag = torch.tensor([ok_here], dtype=torch.int32, device=torch.device("cuda", device))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return int(flag[0]) == 1

    ok = 1
    uid = [None]
    try:
        probe = eng.comm_unique_id()             # EVERY rank: proves that librccl loads here before anybody waits in CommInitRank
        uid = [probe if rank == 0 else None]
    except _lib.NmScanError as e:
        ok = 0
        log.warning(f"rank {rank}: nm_comm_unique_id failed ({e})")
    if agreed(ok):
        dist.broadcast_object_list(uid, src=0)
        try:
            comm_init_watched(uid[0])
        except _lib.NmScanError as e:
            ok = 0
            log.warning(f"rank {rank}: nm_comm_init failed ({e})")
    else:
        ok = 0
    if agreed(ok):
        log.info(f"rank {rank}: count tables all-reduced by nm_allreduce_counts (RCCL, {eng.comm_info()['world']} ranks)")
        return True
    log.warning(f"rank {rank}: the C ABI's communicator is not up on every rank: count tables go through torch.distributed")
    return False


def _filter_stage(eng, cfg, assembly, table, names, shard, world, lap):
    """This rank's contigs of ``names`` (shard ``shard`` of ``world``) and the opened pileup ``table`` -> the engine's planes: upload,
    the pre-filters and the classification, the window pipeline, the merge stage's classification.  Closes ``table`` (and a device
    assembly once its packed bases have served).  Returns (this rank's FilteredPileup, window store, extractor)."""
    parts = assign_contigs([fasta.assembly_length(assembly, c) for c in names], world, bins=[cfg.bin_contig[c] for c in names])
    mine = [names[i] for i in parts[shard]]
    all_bins = sorted(set(cfg.bin_contig[c] for c in names))         # bin ids must be identical on every rank
    upload_assembly(eng, assembly, mine, [cfg.bin_contig[c] for c in mine], all_bins)
    part = _Laps("filters_{}_s", start=lap.t)    # (what upload_filter_s is made of, from the end of the phase before: the pileup parse)
    part("upload_assembly")
    ingest = PileupIngest(eng, table, mine)
    part("tables")
    t0 = time.perf_counter()
    low, high = cfg.methylation_threshold_low, cfg.methylation_threshold_high
    res = ingest.classify(lambda mt: mt, low, high)
    part("ingest")
    if 2 * cfg.padding + 1 > MAX_DEVICE_WINDOW_WIDTH:
        # a search frame beyond the device's window planes (default 40; nobody runs such frames): windows are extracted and
        # filtered on the host (search.HostWindowStore), candidates scored on the device (far-reaching ones by the plain kernel)
        log.info(f"search frame {cfg.search_frame_size}: windows of {2 * cfg.padding + 1} positions stay on the host")
        store, extractor = None, None
    else:
        store, extractor = device_window_pipeline(eng, {c: fasta.assembly_length(assembly, c) for c in names}, mine, cfg.padding, world)
    if isinstance(assembly, fasta.DeviceAssembly) and extractor is not None:
        assembly.close()                         # the packed bases have served; (host windows would read contigs back from them)
    # (confident_rows speaks about the LAST classification: before the merge stage's)
    rows = eng.confident_rows() if extractor is None else tuple(np.zeros(0, dt) for dt in (np.uint32, np.uint32, np.uint8, np.int8))
    if (low, high) == (0.3, 0.7):
        for mt in pileup_mod.MOD_TYPES:
            eng.alias_label((mt, "merge"), mt)
    else:                 # the merge stage always runs at 0.3 / 0.7 (find_motifs_bin.py:569, 1436): a second classification
        ingest.classify(lambda mt: (mt, "merge"), 0.3, 0.7)
    log.info(f"pileup: {res['n_kept']:,} rows after the device-side filters ({time.perf_counter() - t0:.1f}s)")
    part("window_pipeline")
    ingest.close()
    part("table_close")
    lap("upload_filter_s")
    return FilteredPileup(mine, *rows, res["kept"]), store, extractor


def _load_assembly(args, starting, plans, bin_contig, threads, lap):
    """(engine, assembly with the aliased placements of ``bin_contig``); on an error the engine that came up and the plan go."""
    log.info("Loading assembly")
    # A plain-text assembly is parsed ON THE GPU (nm_fasta_parse_device: the host only moves the file through pinned slabs; the
    # bases never become a host array, the planes are packed from the parser's device buffer); a .gz assembly and
    # NANOMOTIF_HOST_FASTA=1 take the native host reader, which runs while the HIP runtime comes up.
    device_fasta = not str(args.assembly).endswith(".gz") and os.environ.get("NANOMOTIF_HOST_FASTA") != "1"
    try:
        if device_fasta:
            eng = starting.engine()
            lap("engine_start_s")
            assembly = fasta.DeviceAssembly(eng, args.assembly, threads=threads)
            TIMINGS["assembly_reading_s"] = assembly.seconds_reading
        else:
            assembly = fasta.load_fasta(args.assembly)
        fasta.add_alias_sequences(assembly, bin_contig)          # a contig listed under several bins is a member of each
    except BaseException:
        starting.abandon()
        plans.drop()
        raise
    lap("assembly_s")
    TIMINGS["assembly_parser"] = "device" if device_fasta else "host"
    if not device_fasta:
        eng = starting.engine()
        lap("engine_start_s")                    # what the assembly did not hide
    return eng, assembly


def _open_table(eng, path, names, bin_contig, plans, threads, lap):
    """The pileup's table for ``names`` (the binned contigs the assembly holds), through the plan made ahead when it is still the right
    one; logs what was read and records the ``pileup_*`` timings."""
    t0 = time.perf_counter()
    wanted = wanted_contigs(path, names)
    plan = plans.take(wanted)
    if plan is not None:
        TIMINGS["pileup_plan_s_on_a_thread"] = plan.seconds
    table = open_pileup(eng, path, wanted, bin_contig, threads, plan=plan)
    on_device = isinstance(table, pileup_mod.DevicePileup)
    how = f", tabix-indexed: {table.bytes_inflated / 1e6:.1f} MB inflated for {len(wanted)} contigs" if table.indexed else ""
    if on_device:
        log.info(f"pileup: {len(table):,} rows parsed on the device ({time.perf_counter() - t0:.1f}s, {table.seconds_reading:.1f}s of it "
                 f"moving the file{how})")
    else:
        log.info(f"pileup: {len(table):,} rows read ({time.perf_counter() - t0:.1f}s{how})")
    lap("pileup_parse_s")
    TIMINGS["pileup_parser"] = "device" if on_device else "host"
    if on_device:
        TIMINGS.update(pileup_reading_s=table.seconds_reading, pileup_inflating_s=table.seconds_inflating, pileup_parsing_s=table.seconds_parsing,
                       pileup_in_parser_s=table.seconds)       # (the rest of pileup_parse_s: the tabix index, the walk over the BGZF blocks, the tables)
    TIMINGS["pileup_rows"] = len(table)
    return table


def find_motifs_bin(args):
    """main.py:46-104."""
    TIMINGS.clear()
    lap = _Laps()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    device = args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
    dist = _start_distributed(device) if world > 1 else None
    starting = _EngineStart(device)
    log.info("Starting nanomotif motif finder")
    bin_contig = fasta.generate_contig_bin(args)
    if not bin_contig:
        log.error("No bin contig mapping found")
        starting.engine().close()
        return None
    threads = parser_threads(args)
    plans = _PlanAhead(str(args.pileup), bin_contig, threads)

    eng, assembly = _load_assembly(args, starting, plans, bin_contig, threads, lap)
    log.info("Identifying motifs")
    cfg = ProcessorConfig(assembly=assembly, pileup_path=args.pileup, bin_contig=bin_contig, threads=args.threads,
                          search_frame_size=args.search_frame_size, methylation_threshold_low=args.methylation_threshold_low,
                          methylation_threshold_high=args.methylation_threshold_high,
                          minimum_kl_divergence=args.minimum_kl_divergence, score_threshold=args.min_motif_score,
                          verbose=args.verbose, log_dir=args.out + "/logs", seed=args.seed, output_dir=args.out)
    names = [c for c in cfg.bin_contig if c in assembly]             # the binned contigs the assembly holds
    table = _open_table(eng, cfg.pileup_path, names, cfg.bin_contig, plans, threads, lap)

    # engine: this rank's contigs (all contigs that belong to a bin).  Several GPUs: whole bins per GPU when they
    # balance (independent searches, no collective until the rows are gathered), else the contigs of every bin are
    # sharded and the count tables all-reduced every round.
    bin_order = list(dict.fromkeys(cfg.bin_contig.values()))         # task order of the reference (:152-171)
    by_bins = None
    if world > 1 and args.shard != "contigs":
        sizes = {}
        for c in names:
            sizes[cfg.bin_contig[c]] = sizes.get(cfg.bin_contig[c], 0) + fasta.assembly_length(assembly, c)
        by_bins = assign_bins(sizes, world, tolerance=0.15 if args.shard == "auto" else float("inf"))
    if by_bins is not None:
        my_bins = set(by_bins[rank])
        log.info(f"rank {rank}: {len(my_bins)} of {len(sizes)} bins (whole bins per GPU)")
        cfg.bin_contig = {c: b for c, b in cfg.bin_contig.items() if b in my_bins}
        names = [c for c in names if cfg.bin_contig.get(c) in my_bins]
        gather_world, world = world, 1                               # the data path below is a single-GPU run
        if not names:                                                # more GPUs than bins
            return _gather_rows(args, [], rank, gather_world, bin_order)
    else:
        gather_world = 1
    if world > 1 and dist.get_backend() == "nccl" and os.environ.get("NANOMOTIF_ALLREDUCE", "native") == "native" \
            and _native_communicator_up(eng, dist, rank, world, device):
        use_native_allreduce(eng)
    try:
        filtered, store, extractor = _filter_stage(eng, cfg, assembly, table, names, rank if gather_world == 1 else 0, world, lap)
        if world > 1:                            # (contigs sharded over the ranks: every rank searches on the rows of all)
            gathered = [None] * world
            dist.all_gather_object(gathered, filtered)
            filtered = FilteredPileup.merge(gathered)
        if filtered.kept.sum() == 0:
            log.info("No pileup data after filtering, skipping")
            return _gather_rows(args, [], rank, gather_world, bin_order) if gather_world > 1 else None
        scorer = engine_scorer(eng, cfg.methylation_threshold_low, cfg.methylation_threshold_high, use_dist=world > 1)
        rows, scorer = discover(cfg, filtered, scorer, rank=0 if gather_world > 1 else rank, bgzip_order=cfg.pileup_path.endswith(".gz"),
                                window_store=store, extractor=extractor)
        if getattr(eng, "wide_scored", 0):
            log.info(f"{eng.wide_scored} candidates reaching further than 95 positions from the modified base scored by nm_score_batch_wide")
        lap("search_s")
        TIMINGS.update({"search_" + k: v for k, v in getattr(scorer, "timings", {}).items()})
        out = _gather_rows(args, rows, rank, gather_world, bin_order)
        lap("write_s")
        return out
    finally:
        # also on the early returns and on exceptions: the module-global reducer must not outlive its engine
        use_native_allreduce(None)
        if isinstance(assembly, fasta.DeviceAssembly):
            assembly.close()
        eng.close()


def _gather_rows(args, rows, rank, gather_world, bin_order):
    """Collect the motif rows (whole-bin sharding: from every rank, back into the reference's bin order), apply the
    bin-level filter and let rank 0 write bin-motifs.tsv."""
    if gather_world > 1:
        import torch.distributed as dist
        gathered = [None] * gather_world
        dist.all_gather_object(gathered, rows)
        by_bin = {}
        for part in gathered:
            for r in part:
                by_bin.setdefault(r.reference, []).append(r)
        rows = [r for b in bin_order for r in by_bin.get(b, [])]
    if not rows:
        log.info("No motifs were identified")
        return None
    rows = [r for r in rows if r.n_mod + r.n_nomod >= args.min_motifs_bin]      # main.py:96
    if not rows:
        log.info("Motif frequency of all motifs too low")
        return None
    if rank == 0:
        log.info("Writing motifs")
        postprocess.write_motif_formatted(rows, args.out + "/bin-motifs.tsv")
    log.info(f"Identified {len(rows)} motifs in {len({r.reference for r in rows})} bins")
    return rows


def device_window_pipeline(eng, lengths: dict, mine: list, padding: int, world: int = 1):
    """(window store, extractor) for ``discover``: windows are gathered and the background is counted on the device,
    every rank for its own contigs, with the per-request counts summed over the ranks.  An assembly with letters
    other than A C G T N keeps window extraction on the host (the reference raises KeyError when a window meets one,
    seq.py:474-478, and so does the host path); then every rank holds all windows."""
    from .engine import DeviceWindowExtractor, DeviceWindowStore
    if world > 1:
        import torch.distributed as dist
    other = np.array([eng.other_letters()], dtype=np.int64)
    if world > 1:
        other = allreduce_counts(other)
    if int(other[0]):
        log.info(f"{int(other[0])} assembly letters outside ACGTN: window extraction stays on the host")
        return DeviceWindowStore(eng), None

    def everywhere(local: dict) -> dict:
        if world == 1:
            return local
        gathered = [None] * world
        dist.all_gather_object(gathered, local)
        return {k: v for g in gathered for k, v in g.items()}

    # valid sample starts per contig (seq.py:202-225), counted on the device; confident rows per contig and strand (the windows
    # themselves are read from the methylated-state planes).  One GPU: the native plan (nm_plan_windows) counts both itself, so the
    # tables are made only when the task-by-task path asks for them (NANOMOTIF_PLAN_PER_TASK=1): four device round trips and four
    # dictionaries over every contig otherwise — 4 ms of a 1 Gbp run.
    bases = sorted({MOD_TYPE_TO_CANONICAL[mt] for mt in pileup_mod.MOD_TYPES})
    mods = [mt for mt in pileup_mod.MOD_TYPES if mt in eng.slot_of_mod]
    if world == 1:
        n_valid = _LazyTables(bases, lambda base: dict(zip(mine, eng.contig_base_counts(base, padding).tolist())))
        row_counts = _LazyTables(mods, lambda mt: dict(zip(mine, eng.methylated_row_counts(mt, padding).tolist())))
    else:
        n_valid = {base: everywhere(dict(zip(mine, eng.contig_base_counts(base, padding).tolist()))) for base in bases}
        row_counts = {mt: everywhere(dict(zip(mine, eng.methylated_row_counts(mt, padding).tolist()))) for mt in mods}
    reduce = allreduce_counts if world > 1 else None
    store = DeviceWindowStore(eng, allreduce=reduce)
    return store, DeviceWindowExtractor(eng, store, lengths, n_valid, padding, resident=eng.contig_index, allreduce_i64=reduce,
                                        row_counts=row_counts)


class _LazyTables:
    """``tables[key]`` made by ``make(key)`` on first use (the keys are known up front: ``in`` and iteration work without making any)."""

    def __init__(self, keys, make):
        self._keys, self._make, self._made = list(keys), make, {}

    def __getitem__(self, key):
        if key not in self._made:
            if key not in self._keys:
                raise KeyError(key)
            self._made[key] = self._make(key)
        return self._made[key]

    def __contains__(self, key):
        return key in self._keys

    def __iter__(self):
        return iter(self._keys)

    def __len__(self):
        return len(self._keys)


def binnary(args):
    """main.py:114-281: the read-methylation table (computed on the device, or read back from OUT when it exists and --force is
    not given), the methylation filter, then contamination detection and / or contig inclusion and their files."""
    import pandas as pd
    from . import binnary as bn
    from .contig_methylation import COLUMNS, methylation_pattern
    log.info(f"Starting Binnary {args.command} analysis...")
    contig_bins = bn.load_contig_bins(args.contig_bins)
    motifs = bn.motif_mods_of_bin_motifs(args.bin_motifs)
    # the reference's choice is spelled weighted_mean but compared with "weighted-mean" (main.py:144-148): both mean the weighted mean
    output_type = "weighted-mean" if args.methylation_output_type == "weighted_mean" else args.methylation_output_type
    table_path = os.path.join(args.out, f"motifs-scored-read-methylation_{args.methylation_output_type}.tsv")
    if os.path.isfile(table_path) and not args.force:
        log.info(f"{os.path.basename(table_path)} exists. Using existing file! Use --force to override this.")
        table = pd.read_csv(table_path, sep="\t", dtype={"contig": str, "motif": str, "mod_type": str, "mod_position": np.int64,
                                                          "methylation_value": np.float64, "mean_read_cov": np.float64, "n_motif_obs": np.int64},
                            keep_default_na=False)
    else:
        log.info(f"Computing {os.path.basename(table_path)}")
        device = args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0") or 0)
        rows = methylation_pattern(pileup=args.pileup, assembly=args.assembly, motifs=motifs, threads=args.threads,
                                   min_valid_read_coverage=args.min_valid_read_coverage, batch_size=1000, min_valid_cov_to_diff_fraction=0.8,
                                   output=table_path, allow_assembly_pileup_mismatch=True, output_type=output_type, device=device)
        if not rows:
            log.warning("the read-methylation table is empty")
            sys.exit(1)
        table = pd.DataFrame(rows, columns=COLUMNS)
    log.info("Loading assembly file...")
    assembly = bn.read_fasta(args.assembly)
    lengths = bn.contig_lengths(assembly)
    table = bn.filter_methylation(table, args.methylation_threshold)
    contamination = None
    if args.command == "detect_contamination" and args.contamination_file:
        contamination = bn.load_contamination_file(args.contamination_file)
    if (args.command == "detect_contamination" and not args.contamination_file) or (args.command == "include_contigs" and args.run_detect_contamination):
        contamination = bn.detect_contamination(bn.add_bin(table, contig_bins), lengths, args.num_consensus, args.threads)
        bn.generate_output(contamination, args.out, "bin_contamination.tsv")
    if args.command == "detect_contamination":
        new_contig_bins = bn.create_contig_bin_file(contig_bins, contamination)
        bn.generate_output(new_contig_bins, args.out, "decontaminated_contig_bin.tsv")
    else:
        if args.contamination_file:
            log.info("Loading contamination file...")
            contamination = bn.load_contamination_file(args.contamination_file)
        if contamination is None:
            contamination = pd.DataFrame({"contig": []}, dtype=str)
        log.info("Removing contaminants from bins")
        contig_bins = contig_bins[~contig_bins["contig"].isin(contamination["contig"])]
        included = bn.include_contigs(bn.add_bin(table, contig_bins), lengths, mean_probability=args.mean_model_confidence)
        bn.generate_output(included, args.out, "include_contigs.tsv")
        unique = (included[included["confidence"] == "high_confidence"][["contig", "assigned_bin"]].rename(columns={"assigned_bin": "bin"})
                  .drop_duplicates())
        new_contig_bins = bn.create_contig_bin_file(contig_bins, contamination, include=unique)
        bn.generate_output(new_contig_bins, args.out, "new_contig_bin.tsv")
    if args.write_bins:
        log.info("Write bins flag is set. Writing bins to file...")
        bn.write_bins_from_contigs(new_contig_bins, assembly, os.path.join(args.out, args.command + "_bins"))
    log.info(f"Analysis Completed. Results are saved to: {args.out}")


def check_installation():
    """main.py:330-346 runs motif_discovery on the packaged geobacillus data; its pileup is not distributable, so
    this build runs the same command on a small synthetic data set with the same planted motifs."""
    import shutil
    import subprocess
    import tempfile
    from . import synth
    tmp = tempfile.mkdtemp(prefix="nanomotif_check_installation_")
    mg = synth.make_metagenome(synth.SynthSpec(
        n_contigs=2, total_bp=200_000, n_bins=1, mod_types=("a",), seed=43, min_contig_bp=80_000,
        fixed_motifs=(("GATC", 1, "a"), ("ACCCA", 4, "a"), ("CCAAAT", 4, "a"), ("GRNGAAGY", 5, "a"))))
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_bed(tmp + "/pileup.bed")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    out = tmp + "/out"
    cmd = [sys.executable, "-m", "nanomotif_amd", "motif_discovery", "-t", "1", tmp + "/assembly.fasta", tmp + "/pileup.bed",
           "-c", tmp + "/contig_bin.tsv", "--out", out]
    rc = subprocess.run(cmd).returncode
    if rc == 0 and os.path.exists(out + "/bin-motifs.tsv"):
        print(open(out + "/bin-motifs.tsv").read())
    shutil.rmtree(tmp, ignore_errors=True)
    return rc


def main(argv=None):
    parser = create_parser()
    args = parser.parse_args(argv)
    if args.command == "motif_discovery":
        rank = int(os.environ.get("RANK", "0"))
        shared_setup(args, args.out, rank=rank)
        t_main = time.perf_counter()
        result = find_motifs_bin(args)
        if rank == 0:
            try:
                TIMINGS["find_motifs_bin_s"] = time.perf_counter() - t_main
                with open(os.path.join(args.out, "logs", "timings.motif_discovery.json"), "w") as f:
                    json.dump(TIMINGS, f, indent=1)
            except OSError:
                pass
        if result is None and rank == 0:
            with open(os.path.join(args.out, "bin-motifs.tsv"), "w") as f:     # main.py:317-321
                f.write(HEADER)
    elif args.command in ("motif_sites", "motif_coverage", "motif_compare", "motif_strands", "motif_profile", "motif_tracks", "motif_fractions", "motif_pileup", "motif_shift", "motif_context", "motif_gc", "motif_overlap", "motif_regions", "motif_runs", "motif_kmers"):
        import importlib
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            sys.stderr.write(f"nanomotif {args.command} runs on one GPU: start it without a multi-rank launcher\n")
            sys.exit(2)
        command = importlib.import_module("." + args.command, __package__)
        shared_setup(args, args.out)
        status = command.run(args)
        try:
            with open(os.path.join(args.out, "logs", f"timings.{args.command}.json"), "w") as f:
                json.dump(command.TIMINGS, f, indent=1)
        except OSError:
            pass
        if status:
            sys.exit(status)
    elif args.command in ("detect_contamination", "include_contigs"):
        args.verbose = False                    # main.py:310-312: binnary runs with seed 1
        args.seed = 1
        shared_setup(args, args.out)
        binnary(args)
    elif args.command == "check_installation":
        sys.exit(check_installation())
    else:
        parser.print_help()
        sys.exit()


if __name__ == "__main__":
    main()
