"""Python host of the HIP scan engine: owns an ``nm_ctx`` and speaks in the reference's vocabulary
(contigs, bins, pileup rows, motifs).  Thin by design — packing, classification, scanning and counting all
happen on the GPU inside libnmscan.so; this file only marshals numpy buffers through ctypes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .motif import MOD_TYPE_TO_CANONICAL, Motif


MAX_MOTIF_LEN = 191        # include/nmscan.h NM_MAX_MOTIF_LEN: stripped length of a candidate on the fast scoring kernels ...
MAX_REACH = 95             # ... and its furthest position from the modified base; beyond: nm_score_batch_wide
MAX_DEVICE_WINDOW_WIDTH = 191      # NM_WIN_MAX_WIDTH 192 columns: wider search frames keep their windows on the host


def _ptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


SITE_STATES = ("mod", "nomod", "nocall")       # include/nmscan.h: NM_SITES_MOD / NM_SITES_NOMOD / NM_SITES_NOCALL, the state of a record's code
SITE_MINUS = 4                                 # NM_SITES_MINUS: the strand bit of a record's code
SITE_RECORD_BYTES = 9                          # a record on the device: contig (4), position (4), code (1)
SITE_BUDGET_BYTES = 256 << 20                  # default size of one batch of records (ScanEngine.motif_sites)
SITE_DTYPE = np.dtype([("candidate", np.uint32), ("contig", np.uint32), ("pos", np.uint32), ("code", np.uint8)])
COMPARE_MINUS = 16                             # NM_COMPARE_MINUS: the strand bit of a record of nm_motif_compare_sites; the rest is the transition
TRANSITIONS = tuple(f"{a}>{b}" for a in SITE_STATES for b in SITE_STATES)      # transition t = 3 * state in sample A + state in sample B
SWITCHED = ("mod>nomod", "nomod>mod")          # NM_COMPARE_SWITCHED: the two discordant called transitions
STRANDS_MINUS = 16                             # NM_STRANDS_MINUS: the strand bit of a record of nm_motif_strands_sites; the rest is the pair
PAIRS = tuple(f"{a}-{b}" for a in SITE_STATES for b in SITE_STATES)            # pair t = 3 * state of the own base + state of the partner's
HEMI = ("mod-nomod", "nomod-mod")              # NM_STRANDS_HEMI: the two hemimethylated pairs
PROFILE_MAX_RADIUS = 31                        # NM_PROFILE_MAX_RADIUS: offsets a profile reaches either side of the modified base
PROFILE_CLASSES = ("mod", "nomod", "nocall", "other")                           # the last axis of ScanEngine.motif_profile's table
CONTEXT_MAX_RADIUS = 31                        # NM_CONTEXT_MAX_RADIUS: offsets a context table reaches either side of the modified base
CONTEXT_LETTERS = ("A", "C", "G", "T", "other")                                 # the last axis of ScanEngine.motif_context's table
TRACKS_MIN_WINDOW = 128                        # NM_TRACKS_MIN_WINDOW: one lane's span of a wave-chunk; a window is a multiple of it ...
TRACKS_MAX_WINDOW = 1 << 30                    # ... up to NM_TRACKS_MAX_WINDOW
TRACK_ROW_BYTES = 24                           # a row of ScanEngine.motif_tracks on the device: six uint32
TRACK_BUDGET_BYTES = 256 << 20                 # default size of the tables of one library call of ScanEngine.motif_tracks
FRACTIONS_MIN_BINS, FRACTIONS_MAX_BINS = 2, 64 # NM_FRACTIONS_MIN_BINS / NM_FRACTIONS_MAX_BINS: histogram bins of ScanEngine.motif_fractions
FRACTIONS_EXTRA = 3                            # NM_FRACTIONS_EXTRA: occurrences, sum_valid, sum_mod behind a strand's histogram
FRACTIONS_BUDGET_BYTES = 256 << 20             # default size of the table of one library call of ScanEngine.motif_fractions
UNEXPLAINED_DTYPE =np.dtype([("set", np.uint32), ("contig", np.uint32), ("pos", np.uint32), ("code", np.uint8)])   # ScanEngine.unexplained_sites


PILEUP_SELECT = ("site", "bare")                 # NM_PILEUP_SITE / NM_PILEUP_BARE: occurrences with / without a kept record
PILEUP_MINUS = 4                                 # NM_PILEUP_MINUS: the strand bit of a record of nm_motif_pileup_sites ...
PILEUP_BARE = 1                                  # ... and NM_PILEUP_CODE_BARE: a bare occurrence (n_valid = n_mod = 0)
PILEUP_RECORD_BYTES = 17                         # a record on the device: contig (4), position (4), code (1), n_valid_cov (4), n_modified (4)
PILEUP_DTYPE = np.dtype([("candidate", np.uint32), ("contig", np.uint32), ("pos", np.uint32), ("code", np.uint8), ("n_valid", np.uint32),
                         ("n_mod", np.uint32)])
SHIFT_MIN_BINS, SHIFT_MAX_BINS = 2, 16            # NM_SHIFT_MIN_BINS / NM_SHIFT_MAX_BINS: bins per axis of the joint histogram of ScanEngine.motif_shift_counts
SHIFT_EXTRA = 12                                 # NM_SHIFT_EXTRA: the sums behind a strand's joint histogram, in the order of SHIFT_SUMS
SHIFT_SUMS = ("occurrences", "n_paired", "n_only_a", "n_only_b", "sum_valid_a", "sum_mod_a", "sum_valid_b", "sum_mod_b", "n_up", "n_down", "n_shift_up",
              "n_shift_down")
SHIFT_BUDGET_BYTES = 256 << 20                   # default size of the table of one library call of ScanEngine.motif_shift_counts
SHIFT_SELECT = ("up", "down")                    # NM_SHIFT_UP / NM_SHIFT_DOWN: the read fraction is higher / lower in sample B
SHIFT_MINUS = 4                                  # NM_SHIFT_MINUS: the strand bit of a record of nm_motif_shift_sites ...
SHIFT_DOWN = 1                                   # ... and NM_SHIFT_CODE_DOWN: the site goes down
SHIFT_RECORD_BYTES = 25                          # a record on the device: contig (4), position (4), code (1), n_valid / n_mod of A and of B (4 x 4)
SHIFT_SLOT_B = 3                                 # read-statistics slot of sample B = SHIFT_SLOT_B + the mod code's index (loading: the second pileup's base)
SHIFT_DTYPE = np.dtype([("candidate", np.uint32), ("contig", np.uint32), ("pos", np.uint32), ("code", np.uint8), ("n_valid_a", np.uint32),
                        ("n_mod_a", np.uint32), ("n_valid_b", np.uint32), ("n_mod_b", np.uint32)])
GC_MAX_HALF = 31                            # NM_GC_MAX_HALF: positions a GC window reaches either side of the modified base
GC_BUDGET_BYTES = 256 << 20                    # default size of the table of one library call of ScanEngine.motif_gc
REGION_MAX_CLASSES = 8                         # NM_REGION_MAX_CLASSES: one byte of class mask per record and per chunk
REGIONS_BUDGET_BYTES = 256 << 20               # default size of the table of one library call of ScanEngine.motif_regions_counts
REGION_RECORD_BYTES = 10                       # a record on the device: contig (4), position (4), code (1), classes (1)
REGION_DTYPE = np.dtype(SITE_DTYPE.descr + [("classes", np.uint8)])
REGION_OUTSIDE = "outside"                     # the cell behind the classes, and its name in a selection
RUNS_MIN_MAX_RUN, RUNS_MAX_MAX_RUN = 2, 64     # NM_RUNS_MIN_MAX_RUN / NM_RUNS_MAX_MAX_RUN: the run-length buckets R of ScanEngine.motif_run_counts
RUNS_BUDGET_BYTES = 256 << 20                  # default size of the table of one library call of ScanEngine.motif_run_counts
RUN_RECORD_BYTES = 17                          # a record on the device: contig (4), start (4), state (1), last (4), n_sites (4)
RUN_DTYPE = np.dtype(SITE_DTYPE.descr + [("last", np.uint32), ("n_sites", np.uint32)])
OVERLAP_MAX_PARTNERS = 4095                   # NM_OVERLAP_MAX_PARTNERS: partner motifs of one candidate of ScanEngine.motif_overlap
OVERLAP_ROW_BYTES = 48                         # one (block, contig) row of nm_motif_overlap_count: 2 strands x 3 states, int64
OVERLAP_BUDGET_BYTES = 256 << 20               # default size of the table of one library call of ScanEngine.motif_overlap
KMER_MAX_FLANKS = 10                           # NM_KMER_MAX_FLANKS: counted positions of a k-mer shape ...
KMER_MAX_OFFSET = 31                           # ... each within NM_KMER_MAX_OFFSET of the modified base
KMER_BUDGET_BYTES = 256 << 20                  # default size of the tables of one library call of ScanEngine.kmer_methylation
KMER_LETTERS = "ACGT"                          # the digits 0..3 of a row index


def kmer_shape(shape) -> tuple:
    """The counted offsets of a k-mer shape, ascending: ``shape`` is a shape string — ``N`` a counted position, ``.`` a skipped one,
    exactly one ``*`` for the modified base, e.g. ``NNN*......NNN`` — or a sequence of distinct non-zero offsets.  At most
    ``KMER_MAX_FLANKS`` offsets, each within ``KMER_MAX_OFFSET`` of the modified base; ValueError otherwise."""
    if isinstance(shape, str):
        bad = sorted(set(shape) - set("N.*"))
        if bad:
            raise ValueError(f"shape {shape!r}: only N, . and * are expected, got {''.join(bad)!r}")
        if shape.count("*") != 1:
            raise ValueError(f"shape {shape!r}: exactly one * (the modified base) is expected, got {shape.count('*')}")
        centre = shape.index("*")
        offsets = [j - centre for j, ch in enumerate(shape) if ch == "N"]
    else:
        offsets = sorted(int(o) for o in shape)
        if len(set(offsets)) != len(offsets) or 0 in offsets:
            raise ValueError(f"shape {list(shape)!r}: distinct non-zero offsets are expected")
    if len(offsets) > KMER_MAX_FLANKS:
        raise ValueError(f"shape {shape!r}: {len(offsets)} counted positions, at most {KMER_MAX_FLANKS} are possible")
    if any(abs(o) > KMER_MAX_OFFSET for o in offsets):
        raise ValueError(f"shape {shape!r}: a counted position lies more than {KMER_MAX_OFFSET} from the modified base")
    return tuple(offsets)


def kmer_text(shape, canonical: str, row: int) -> str:
    """The k-mer of table row ``row`` under ``shape``: its letters at the counted positions (the first offset is the most significant
    base-4 digit, A C G T = 0 1 2 3), the canonical base at the modified position, ``.`` in the gaps — from the lowest offset (or the
    modified base) to the highest."""
    offsets = kmer_shape(shape)
    row = int(row)
    if not 0 <= row < 4 ** len(offsets):
        raise ValueError(f"row {row} outside 0..{4 ** len(offsets) - 1}")
    lo, hi = min(offsets + (0,)), max(offsets + (0,))
    text = ["."] * (hi - lo + 1)
    text[-lo] = canonical
    for f, o in enumerate(offsets):
        text[o - lo] = KMER_LETTERS[(row >> 2 * (len(offsets) - 1 - f)) & 3]
    return "".join(text)


def kmer_row(shape, text: str) -> int:
    """The table row of a k-mer text of ``kmer_text`` (the letters at the skipped positions and at the modified base play no part)."""
    offsets = kmer_shape(shape)
    lo = min(offsets + (0,))
    row = 0
    for o in offsets:
        row = row * 4 + KMER_LETTERS.index(text[o - lo])
    return row


def kmer_motif(shape, canonical: str, row: int) -> Motif:
    """The ``Motif`` whose strand-summed ``motif_site_counts`` row is table row ``row``: ``kmer_text`` with its modified position."""
    offsets = kmer_shape(shape)
    return Motif(kmer_text(offsets, canonical, row), -min(offsets + (0,)))


def site_state_set(states) -> int:
    """("mod", "nocall") -> the state_set bits of nm_motif_sites."""
    states = tuple(states)
    bad = [s for s in states if s not in SITE_STATES]
    if bad or not states:
        raise ValueError(f"states must be a non-empty selection of {SITE_STATES}, got {states!r}")
    return sum(1 << SITE_STATES.index(s) for s in set(states))


def run_state_set(states, nocall_breaks=False) -> int:
    """("nomod",) -> the state_set bits of nm_motif_runs_sites: ``site_state_set``, and ValueError for "nocall" without
    ``nocall_breaks`` — a nocall site is transparent then, runs of them do not exist."""
    bits = site_state_set(states)
    if bits & 4 and not nocall_breaks:
        raise ValueError(f"states {tuple(states)!r}: runs of nocall sites exist with nocall_breaks only")
    return bits


def run_length_limit(max_run) -> int:
    """The R of ``ScanEngine.motif_run_counts``: an integer in 2..64, else ValueError."""
    r = int(max_run)
    if r != max_run or not RUNS_MIN_MAX_RUN <= r <= RUNS_MAX_MAX_RUN:
        raise ValueError(f"max_run {max_run!r} outside {RUNS_MIN_MAX_RUN}..{RUNS_MAX_MAX_RUN}")
    return r


def region_class_set(names, selection) -> tuple:
    """(class_set, want_outside) of nm_motif_regions_sites for ``selection``, a sequence of class names of ``names`` (the uploaded
    classes in order) and / or "outside"; None selects every class and not the outside.  ValueError for an unknown name and for an empty
    selection."""
    names = list(names)
    if selection is None:
        return (1 << len(names)) - 1, False
    selection = [selection] if isinstance(selection, str) else list(selection)
    unknown = [s for s in selection if s != REGION_OUTSIDE and s not in names]
    if unknown or not selection:
        raise ValueError(f"classes: a non-empty selection of {', '.join(names + [REGION_OUTSIDE])} is expected, got {selection!r}")
    return sum(1 << names.index(s) for s in set(selection) if s != REGION_OUTSIDE), REGION_OUTSIDE in selection


def pileup_select(select) -> int:
    """("site", "bare") -> NM_PILEUP_SITE | NM_PILEUP_BARE; ValueError for an unknown name or an empty selection."""
    bits = 0
    for s in select:
        if s not in PILEUP_SELECT:
            raise ValueError(f"unknown selection {s!r} (expected a selection of {PILEUP_SELECT})")
        bits |= 1 << PILEUP_SELECT.index(s)
    if bits == 0:
        raise ValueError("no selection given")
    return bits


def shift_select(select) -> int:
    """("up", "down") -> NM_SHIFT_UP | NM_SHIFT_DOWN; ValueError for an unknown name or an empty selection."""
    bits = 0
    for s in select:
        if s not in SHIFT_SELECT:
            raise ValueError(f"unknown direction {s!r} (expected a selection of {SHIFT_SELECT})")
        bits |= 1 << SHIFT_SELECT.index(s)
    if bits == 0:
        raise ValueError("no direction given")
    return bits


def shift_permille(min_delta_permille) -> int:
    """The threshold of ``ScanEngine.motif_shift*`` as the library takes it: an integer in 0..1000, else ValueError."""
    t = int(min_delta_permille)
    if t != min_delta_permille or not 0 <= t <= 1000:
        raise ValueError(f"min_delta_permille {min_delta_permille!r} is not an integer in 0..1000")
    return t


def transition_set(transitions) -> int:
    """("mod>nomod", "nomod>mod") -> the transition_set bits of nm_motif_compare_*."""
    transitions = tuple(transitions)
    bad = [t for t in transitions if t not in TRANSITIONS]
    if bad or not transitions:
        raise ValueError(f"transitions must be a non-empty selection of {TRANSITIONS}, got {transitions!r}")
    return sum(1 << TRANSITIONS.index(t) for t in set(transitions))


def pair_set(pairs) -> int:
    """("mod-nomod", "nomod-mod") -> the pair_set bits of nm_motif_strands_*."""
    pairs = tuple(pairs)
    bad = [t for t in pairs if t not in PAIRS]
    if bad or not pairs:
        raise ValueError(f"pairs must be a non-empty selection of {PAIRS}, got {pairs!r}")
    return sum(1 << PAIRS.index(t) for t in set(pairs))


def track_window(window) -> int:
    """A window size of ``ScanEngine.motif_tracks``: a multiple of 128 in [128, 2^30]; ValueError otherwise."""
    w = int(window)
    if not TRACKS_MIN_WINDOW <= w <= TRACKS_MAX_WINDOW or w % TRACKS_MIN_WINDOW:
        raise ValueError(f"window {window!r}: a multiple of {TRACKS_MIN_WINDOW} in [{TRACKS_MIN_WINDOW}, 2^30]")
    return w


def window_prefix(lengths, window) -> np.ndarray:
    """int64[n + 1]: the prefix of the window counts max(1, ceil(L / window)) of contigs of the given lengths — the layout of
    nm_tracks_windows restated on the host (``ScanEngine.track_windows`` asks the library)."""
    w = track_window(window)
    out = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum([max(1, -(-int(n) // w)) for n in lengths], out=out[1:])
    return out


def partner_offset(motif: Motif, partner_position: int) -> int:
    """d = L - 1 - i - j of include/nmscan.h: ``motif`` (L tokens, unstripped) has its modified base at i, its partner's modified base
    is at ``partner_position`` = j of the motif's reverse complement.  Stripping dots from both ends of both leaves d unchanged."""
    return len(motif.tokens) - 1 - int(motif.mod_position) - int(partner_position)


class SiteBatch:
    """One delivery of ``ScanEngine.motif_sites``: the records [first_record, first_record + len(records)) of the candidates
    [first_candidate, first_candidate + n_candidates), which hold ``batch_records`` in all; ``counts`` (first delivery of a group of
    candidates only, else None): per candidate (contig names, int64[n_contigs, 6]) as ``motif_site_counts`` returns."""

    def __init__(self, first_candidate, n_candidates, first_record, batch_records, records, counts):
        self.first_candidate, self.n_candidates, self.first_record, self.batch_records = first_candidate, n_candidates, first_record, batch_records
        self.records, self.counts = records, counts


class CandidateBatch:
    """Flat SoA form of a list of candidates (include/nmscan.h: nm_score_batch arguments)."""

    def __init__(self, bins, slots, lens, modpos, offsets, masks):
        self.bins, self.slots, self.lens, self.modpos, self.offsets, self.masks = bins, slots, lens, modpos, offsets, masks

    def __len__(self):
        return len(self.bins)

    def slice(self, k, e):
        """The candidates [k, e): views of the per-candidate arrays, the mask pool shared."""
        return CandidateBatch(self.bins[k:e], self.slots[k:e], self.lens[k:e], self.modpos[k:e], self.offsets[k:e], self.masks)


def _budget_groups(costs, limit):
    """Consecutive owners grouped while the sum of their ``costs`` fits ``limit``; a group holds at least one owner.  Yields (k, e, sum
    of the costs of the owners [k, e))."""
    n, k = len(costs), 0
    while k < n:
        e, held = k + 1, int(costs[k])
        while e < n and held + int(costs[e]) <= limit:
            held += int(costs[e])
            e += 1
        yield k, e, held
        k = e


def _byte_limit(max_bytes, default: int) -> int:
    """The ``max_bytes`` of a generator over tables: ``default`` when None; ValueError below 1."""
    limit = default if max_bytes is None else int(max_bytes)
    if limit < 1:
        raise ValueError("max_bytes must be at least 1")
    return limit


def _table_groups(b: CandidateBatch, names: dict, n_rows, row_bytes: int, limit: int, shape: tuple, dtype, call):
    """The table loop of the generators over per-candidate tables (``ScanEngine.motif_tracks`` / ``motif_fractions`` / ``motif_gc`` /
    ``motif_overlap``).  Candidate j of ``b`` owns ``n_rows[j]`` rows of ``row_bytes`` bytes; consecutive candidates [k, e) share one
    zeroed table ``dtype[max(rows, 1), *shape]`` while their rows fit ``limit`` bytes (a group holds at least one candidate), filled by
    ``call(k, e, b.slice(k, e), rows, table)`` with ``rows`` the uint64 row prefix of the group.  Yields (j, the contig names
    ``names[bin id]`` of j's bin, j's rows of the table) in candidate order — the same under every ``limit``."""
    bins = [int(x) for x in b.bins]
    for k, e, _ in _budget_groups([int(n) * row_bytes for n in n_rows], limit):
        rows = np.zeros(e - k + 1, dtype=np.uint64)
        np.cumsum([int(n) for n in n_rows[k:e]], out=rows[1:])
        table = np.zeros((max(int(rows[-1]), 1), *shape), dtype=dtype)
        call(k, e, b.slice(k, e), rows, table)
        for j in range(k, e):
            yield j, names[bins[j]], table[int(rows[j - k]):int(rows[j - k + 1])]


class DeviceWindowStore:
    """Window requests of the lock-step search served by the engine's window kernels (nm_win_*): same interface as
    search.HostWindowStore.  Windows are bit planes over windows in HBM; a ``pssm`` request returns integer counts,
    a ``remove`` request clears the matching windows from the task's alive mask."""

    def __init__(self, engine, allreduce=None):
        """``allreduce``: callable summing an int32 numpy array over the ranks of a multi-GPU run, in which every rank
        holds only the windows of its own contigs (tasks added with ``add_task_rows``)."""
        self.engine = engine
        self.allreduce = allreduce
        self.task_id = {}
        self.totals = {}
        self.width = {}
        _lib.check(engine.lib.nm_win_clear(engine.ctx))

    def add_task_rows(self, key, contig, position, minus, pad, total=None):
        """Windows gathered on the device from the resident sequence planes (nm_win_add_task_rows): rows are
        (engine contig index, position, minus flag), already edge-filtered.  ``total``: number of windows of the task
        over all ranks (default: the rows given)."""
        contig = np.ascontiguousarray(contig, dtype=np.uint32)
        position = np.ascontiguousarray(position, dtype=np.uint32)
        minus = np.ascontiguousarray(minus, dtype=np.uint8)
        tid = C.c_uint32(0)
        _lib.check(self.engine.lib.nm_win_add_task_rows(self.engine.ctx, len(contig), _ptr(contig, C.c_uint32),
                                                        _ptr(position, C.c_uint32), _ptr(minus, C.c_uint8), int(pad), C.byref(tid)))
        self.task_id[key], self.width[key] = int(tid.value), 2 * int(pad) + 1
        self.totals[key] = int(len(contig) if total is None else total)

    def add_task(self, key, sets: np.ndarray):
        sets = np.ascontiguousarray(sets, dtype=np.uint8)
        tid = C.c_uint32(0)
        _lib.check(self.engine.lib.nm_win_add_task(self.engine.ctx, sets.shape[0], sets.shape[1], _ptr(sets, C.c_uint8), C.byref(tid)))
        self.task_id[key], self.totals[key], self.width[key] = int(tid.value), int(sets.shape[0]), int(sets.shape[1])

    def add_task_contigs(self, key, label, contigs, pad, total=None):
        """Windows around every confidently methylated row (pad < pos < len - pad) of the listed resident contigs,
        taken from the methylated-state planes of the classification ``label`` (nm_win_add_task_contigs)."""
        contigs = np.ascontiguousarray(contigs, dtype=np.uint32)
        tid, n = C.c_uint32(0), C.c_uint64(0)
        _lib.check(self.engine.lib.nm_win_add_task_contigs(self.engine.ctx, self.engine.slot_of_mod[label], len(contigs),
                                                           _ptr(contigs, C.c_uint32), int(pad), C.byref(tid), C.byref(n)))
        self.task_id[key], self.width[key] = int(tid.value), 2 * int(pad) + 1
        self.totals[key] = int(n.value if total is None else total)
        return int(n.value)

    def execute(self, batch):
        out = [None] * len(batch)
        dev = [(i, key, req) for i, (key, req) in enumerate(batch) if req.kind != "total"]
        for i, (key, req) in enumerate(batch):
            if req.kind == "total":
                out[i] = self.totals[key]
        if dev:
            n = len(dev)
            task = np.fromiter((self.task_id[k] for _, k, _ in dev), dtype=np.uint32, count=n)
            kind = np.fromiter((1 if r.kind == "remove" else 0 for _, _, r in dev), dtype=np.uint8, count=n)
            ws = (max(self.width[k] for _, k, _ in dev) + 63) // 64 * 64        # columns per row of sets / counts (nm_win_batch_w)
            sets = np.full((n, ws), 15, dtype=np.uint8)
            for j, (_, k, r) in enumerate(dev):
                sets[j, :self.width[k]] = r.motif.sets
            res = np.zeros((n, 2 + 4 * ws), dtype=np.int32)
            _lib.check(self.engine.lib.nm_win_batch_w(self.engine.ctx, n, _ptr(task, C.c_uint32), _ptr(kind, C.c_uint8),
                                                      _ptr(sets, C.c_uint8), ws, res.ctypes.data_as(C.POINTER(C.c_int32))))
            if self.allreduce is not None:
                res = self.allreduce(res)
            for j, (i, k, r) in enumerate(dev):
                if r.kind == "remove":
                    out[i] = (int(res[j, 0]), int(res[j, 1]))
                else:
                    w = self.width[k]
                    out[i] = (int(res[j, 0]), res[j, 2:].reshape(4, ws)[:, :w].astype(np.int64))
        return out


class DeviceWindowExtractor:
    """``extract_windows`` (find_motifs_bin.py:625-686) with the window gather and the background letter counts on the
    device: the host only draws the sample indices (``random.sample`` order and consumption are the reference's) and
    applies the edge filter to the row positions; sequences are read from the resident bit planes.

    ``lengths`` / ``n_valid[base]``: contig name -> length / number of valid sample starts (``contig_base_counts``),
    for EVERY contig of the data set; ``resident``: name -> engine contig index for the contigs this rank holds (all of
    them on one GPU).  Samples and rows of other contigs are left to their rank; ``allreduce_i64`` sums the counts."""

    MAX_SAMPLES_PER_CALL = 4 << 20

    def __init__(self, engine, store: DeviceWindowStore, lengths, n_valid, padding, resident=None, allreduce_i64=None,
                 background_sampling_frequency=0.01, row_counts=None):
        """``row_counts[mod type]``: contig name -> (plus, minus) confident rows inside the edge padding
        (``methylated_row_counts``), over all ranks — needed by ``plan_contigs`` only."""
        self.engine, self.store, self.lengths, self.n_valid, self.pad = engine, store, lengths, n_valid, int(padding)
        self.row_counts = row_counts
        self.resident = engine.contig_index if resident is None else resident
        self.allreduce_i64 = allreduce_i64
        self.freq = background_sampling_frequency
        self.tasks = []           # (key, base, n_bg, [sample contig arrays], [sample rank arrays])
        self._groups = []         # deferred draws: [(MT19937 state at the group's start, [(task index or None, nv, n_samples, keep)])]

    def _draw(self, rng, name, base, s_contig, s_rank) -> int:
        """The background sample of one contig (seq.py:202-225): draws its start ranks from ``rng`` (consumed on every
        rank alike), keeps them if the contig is resident here, returns the number of samples."""
        import math
        length = int(self.lengths[name])
        n_samples = int(max(math.ceil(length * self.freq), 50))
        if n_samples > length - (2 * self.pad + 1) + 1:
            raise ValueError("Too many samples requested for unique subsequences")
        nv = int(self.n_valid[base][name])
        if nv < n_samples:
            raise ValueError(f"Not enough subsequences with '{base}' in the middle (found {nv}, need {n_samples})")
        ranks = rng.sample(nv, n_samples)
        ci = self.resident.get(name)
        if ci is not None:
            s_contig.append(np.full(n_samples, ci, dtype=np.uint32))
            s_rank.append(ranks.astype(np.uint32))
        return n_samples

    def plan(self, key, plus_pos: dict, minus_pos: dict, mod_type: str) -> bool:
        """One task from explicit row positions (name -> ascending positions of the confident rows per strand);
        consumes the interpreter's RNG exactly like extract_windows.  False = no methylation windows."""
        from .search import NativeRandom
        base, pad = MOD_TYPE_TO_CANONICAL[mod_type], self.pad
        s_contig, s_rank, rows_c, rows_p, rows_m = [], [], [], [], []
        n_bg = total = 0
        empty = np.zeros(0, np.int64)
        with NativeRandom() as rng:
            for name in sorted(plus_pos.keys() | minus_pos.keys()):
                n_bg += self._draw(rng, name, base, s_contig, s_rank)
                length = int(self.lengths[name])
                p, m = plus_pos.get(name, empty), minus_pos.get(name, empty)
                p = p[(p > pad) & (p < length - pad)]
                m = m[(m > pad) & (m < length - pad)]
                if len(p) + len(m) == 0:
                    return False                         # find_motifs_bin.py:662-664
                total += len(p) + len(m)
                ci = self.resident.get(name)
                if ci is not None:
                    rows_c.append(np.full(len(p) + len(m), ci, dtype=np.uint32))
                    rows_p += [p, m]
                    rows_m.append(np.concatenate([np.zeros(len(p), np.uint8), np.ones(len(m), np.uint8)]))
        if total == 0 or n_bg == 0:
            return False
        cat = lambda xs, dt: np.concatenate(xs).astype(dt, copy=False) if xs else np.zeros(0, dt)
        self.store.add_task_rows(key, cat(rows_c, np.uint32), cat(rows_p, np.uint32), cat(rows_m, np.uint8), pad, total=total)
        self.tasks.append((key, base, n_bg, cat(s_contig, np.uint32), cat(s_rank, np.uint32)))
        return True

    def begin_group(self, seed=None):
        """Called right after the caller (re)seeded ``random`` for the next task(s): the ``plan_contigs`` calls that follow
        form one generator stream whose draws are DEFERRED to ``finish`` — where the streams of all tasks are drawn on
        several host threads at once (a thousand tasks x 1 % of a Gbp is 1e7 sequential Mersenne-Twister draws).
        ``seed``: what ``random.seed`` was just called with — every task of a plain-pileup run starts from the same
        generator state (find_motifs_bin.py:152-171), read from the interpreter once."""
        import random
        cache = self.__dict__.setdefault("_seed_state", {})
        state = cache.get(seed) if seed is not None else None
        if state is None:
            state = np.array(random.getstate()[1], dtype=np.uint32)
            if seed is not None:
                cache[seed] = state
        self._groups.append((state, []))

    def plan_contigs(self, key, names, mod_type: str) -> bool:
        """``plan`` without row lists: the task's windows are all confident rows of the contigs ``names`` (those present
        in the filtered pileup of this mod type), read on the device from the methylated-state planes.  The background
        samples of all its contigs are drawn by ONE native call (same draws, same order as contig-by-contig)."""
        import math
        from .search import NativeRandom
        base, counts = MOD_TYPE_TO_CANONICAL[mod_type], self.row_counts[mod_type]
        names = sorted(names)
        W = 2 * self.pad + 1
        lengths = [int(self.lengths[n]) for n in names]
        n_samples = [int(max(math.ceil(L * self.freq), 50)) for L in lengths]
        nv = [int(self.n_valid[base][n]) for n in names]
        # the reference draws contig by contig and stops at the first contig without rows (find_motifs_bin.py:662-664):
        # only the contigs before it consume random numbers
        stop = next((i for i, n in enumerate(names) if int(counts[n][0]) + int(counts[n][1]) == 0), len(names))
        for i in range(min(stop + 1, len(names))):
            if n_samples[i] > lengths[i] - W + 1:
                raise ValueError("Too many samples requested for unique subsequences")
            if nv[i] < n_samples[i]:
                raise ValueError(f"Not enough subsequences with '{base}' in the middle (found {nv[i]}, need {n_samples[i]})")
        drawn = min(stop + 1, len(names))
        deferred = bool(self._groups)
        if deferred:
            ranks = None
        else:
            with NativeRandom() as rng:
                ranks = rng.sample_many(nv[:drawn], n_samples[:drawn])
        if stop < len(names):
            if deferred:
                self._groups[-1][1].append((None, nv[:drawn], n_samples[:drawn], None))      # consumes numbers, keeps none
            return False
        total = sum(int(counts[n][0]) + int(counts[n][1]) for n in names)
        n_bg = sum(n_samples)
        if total == 0 or n_bg == 0:
            return False
        res = [self.resident.get(n) for n in names]
        mine = [ci for ci in res if ci is not None]
        if deferred:
            keep = [i for i, ci in enumerate(res) if ci is not None]
            # the samples stay RUNS (contig, count) — nm_bg_counts_runs writes the per-sample contig column on the device
            runs = (np.asarray(mine, dtype=np.uint32), np.asarray([n_samples[i] for i in keep], dtype=np.uint32))
            self._groups[-1][1].append((len(self.tasks), nv, n_samples, keep))
            self.store.add_task_contigs(key, mod_type, mine, self.pad, total=total)
            self.tasks.append([key, base, n_bg, runs, None])
            return True
        if len(mine) == len(names):
            s_contig = np.repeat(np.asarray(mine, dtype=np.uint32), n_samples)
            s_rank = ranks
        else:
            off = np.concatenate([[0], np.cumsum(n_samples)])
            keep = [i for i, ci in enumerate(res) if ci is not None]
            s_contig = np.repeat(np.asarray([res[i] for i in keep], dtype=np.uint32), [n_samples[i] for i in keep]) if keep else np.zeros(0, np.uint32)
            s_rank = np.concatenate([ranks[off[i]:off[i + 1]] for i in keep]) if keep else np.zeros(0, np.uint32)
        self.store.add_task_contigs(key, mod_type, mine, self.pad, total=total)
        self.tasks.append((key, base, n_bg, s_contig, np.ascontiguousarray(s_rank, dtype=np.uint32)))
        return True

    def _draw_deferred(self):
        _draw_deferred_impl(self)

    def plan_all(self, tasks, seed, one_stream_per_bin=False) -> dict:
        """Every task of a single-GPU run in ONE native call (nm_plan_windows): ``tasks`` = [(key, contig names present in
        the filtered pileup of the task's mod type — or their engine indices, a uint32 array in the order of the sorted names —,
        mod_type)] in task order; ``seed``: what the reference seeds ``random``
        with before a task (plain pileup, find_motifs_bin.py:152-171) or before a bin's tasks (``one_stream_per_bin``: the
        bgzip path, :219-248 — consecutive tasks of one bin share a stream).  Windows are gathered, backgrounds drawn and
        counted on the device / on native threads; the interpreter's generator ends where the sequential run would leave it.
        Returns {key: background PSSM float64[4, W]} for the tasks that have methylation windows (the others are the
        reference's "No methylation sequences found")."""
        import random
        if not tasks:
            return {}
        n = len(tasks)
        slot = np.fromiter((self.engine.slot_of_mod[t[2]] for t in tasks), dtype=np.uint32, count=n)
        base = np.fromiter((ord(MOD_TYPE_TO_CANONICAL[t[2]]) for t in tasks), dtype=np.uint8, count=n)
        begin = np.zeros(n + 1, dtype=np.uint32)
        res = self.resident
        parts = [t[1] if isinstance(t[1], np.ndarray) else np.fromiter((res[x] for x in sorted(t[1])), dtype=np.uint32, count=len(t[1]))
                 for t in tasks]
        np.cumsum(np.fromiter((len(x) for x in parts), dtype=np.uint32, count=n), out=begin[1:])
        ids = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint32)
        if one_stream_per_bin:
            group = np.zeros(n, dtype=np.uint32)
            g, last_bin = -1, object()
            for k, (key, _, _) in enumerate(tasks):
                if key[0] != last_bin:
                    g, last_bin = g + 1, key[0]
                group[k] = g
            n_groups = g + 1
        else:
            group, n_groups = np.arange(n, dtype=np.uint32), n
        version, _, gauss = random.getstate()
        random.seed(seed)
        init = np.array(random.getstate()[1], dtype=np.uint32)
        W = 2 * self.pad + 1
        status = np.zeros(n, dtype=np.uint8)
        window = np.zeros(n, dtype=np.uint32)
        n_win, n_bg = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        counts = np.zeros((n, 4, W), dtype=np.int64)
        final = np.zeros(625, dtype=np.uint32)
        rc = self.engine.lib.nm_plan_windows(self.engine.ctx, n, _ptr(slot, C.c_uint32), _ptr(base, C.c_uint8), _ptr(group, C.c_uint32),
                                             _ptr(begin, C.c_uint32), _ptr(ids, C.c_uint32), self.pad, float(self.freq), n_groups,
                                             _ptr(init, C.c_uint32), 1, _ptr(status, C.c_uint8), _ptr(window, C.c_uint32),
                                             _ptr(n_win, C.c_uint64), _ptr(n_bg, C.c_uint64), _ptr(counts, C.c_int64), _ptr(final, C.c_uint32))
        if rc:
            msg = self.engine.lib.nm_last_error().decode()
            if msg.startswith("Too many samples") or msg.startswith("Not enough subsequences"):
                raise ValueError(msg)                       # seq.py:208-219 raises these
            _lib.check(rc)
        random.setstate((version, tuple(final.tolist()), gauss))
        out = {}
        # (one division for all tasks: a thousand small numpy calls cost more than the arithmetic; true division of int64 by
        #  float64 like the per-task expression counts[k] / float(n_bg[k]))
        pssm = counts / np.where(n_bg == 0, 1, n_bg).astype(np.float64)[:, None, None]
        ok, win, nw = (status == 0).tolist(), window.tolist(), n_win.tolist()
        task_id, width, totals = self.store.task_id, self.store.width, self.store.totals
        for k, (key, _, _) in enumerate(tasks):
            if not ok[k]:
                continue
            task_id[key], width[key], totals[key] = win[k], W, nw[k]
            out[key] = pssm[k]
        return out

    def finish(self) -> dict:
        """Background PSSM (``background_sequences.pssm()``, float64[4, W]) of every planned task."""
        W = 2 * self.pad + 1
        if self._groups:
            self._draw_deferred()
        counts = np.zeros((len(self.tasks), 4, W), dtype=np.int64)
        n_of = [len(t[4]) for t in self.tasks]                 # samples this rank holds of every task
        for base in sorted({t[1] for t in self.tasks}):
            idx = [i for i, t in enumerate(self.tasks) if t[1] == base]
            lo = 0
            while lo < len(idx):
                hi, n = lo, 0
                while hi < len(idx) and (hi == lo or n + n_of[idx[hi]] <= self.MAX_SAMPLES_PER_CALL):
                    n += n_of[idx[hi]]
                    hi += 1
                part = idx[lo:hi]
                sr = np.concatenate([self.tasks[i][4] for i in part]) if n else np.zeros(0, np.uint32)
                out = np.zeros((len(part), 4, W), dtype=np.int64)
                if all(isinstance(self.tasks[i][3], tuple) for i in part):
                    run_begin = np.zeros(len(part) + 1, dtype=np.uint32)
                    np.cumsum([len(self.tasks[i][3][0]) for i in part], out=run_begin[1:])
                    rc = np.ascontiguousarray(np.concatenate([self.tasks[i][3][0] for i in part]), dtype=np.uint32)
                    rn = np.ascontiguousarray(np.concatenate([self.tasks[i][3][1] for i in part]), dtype=np.uint32)
                    _lib.check(self.engine.lib.nm_bg_counts_runs(self.engine.ctx, ord(base), self.pad, len(rc), _ptr(rc, C.c_uint32),
                                                                 _ptr(rn, C.c_uint32), _ptr(sr, C.c_uint32), len(part),
                                                                 _ptr(run_begin, C.c_uint32), _ptr(out, C.c_int64)))
                else:
                    begin = np.zeros(len(part) + 1, dtype=np.uint64)
                    np.cumsum([n_of[i] for i in part], out=begin[1:])
                    sc = np.concatenate([self.tasks[i][3] if not isinstance(self.tasks[i][3], tuple) else np.repeat(*self.tasks[i][3])
                                         for i in part]) if n else np.zeros(0, np.uint32)
                    _lib.check(self.engine.lib.nm_bg_counts(self.engine.ctx, ord(base), self.pad, n, _ptr(sc, C.c_uint32), _ptr(sr, C.c_uint32),
                                                            len(part), _ptr(begin, C.c_uint64), _ptr(out, C.c_int64)))
                counts[part] = out
                lo = hi
        if self.allreduce_i64 is not None:
            counts = self.allreduce_i64(counts)
        res = {t[0]: counts[i] / t[2] for i, t in enumerate(self.tasks)}
        self.tasks = []
        return res


def _draw_deferred_impl(extractor):
    import random
    groups = extractor._groups
    calls = [c for _, cs in groups for c in cs]
    group_off = np.zeros(len(groups) + 1, dtype=np.uint64)
    np.cumsum([sum(len(c[1]) for c in cs) for _, cs in groups], out=group_off[1:])
    ns = np.ascontiguousarray(np.concatenate([np.asarray(c[1], dtype=np.uint64) for c in calls]) if calls else np.zeros(0, np.uint64))
    ks = np.ascontiguousarray(np.concatenate([np.asarray(c[2], dtype=np.uint64) for c in calls]) if calls else np.zeros(0, np.uint64))
    init = np.ascontiguousarray(np.stack([st for st, _ in groups]))
    out = np.empty(max(int(ks.sum()), 1), dtype=np.uint32)
    final = np.zeros(625, dtype=np.uint32)
    _lib.check(extractor.engine.lib.nm_py_random_sample_groups(len(groups), _ptr(init, C.c_uint32), _ptr(group_off, C.c_uint64), _ptr(ns, C.c_uint64),
                                                               _ptr(ks, C.c_uint64), _ptr(out, C.c_uint32), _ptr(final, C.c_uint32)))
    off = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
    at = 0
    for task, nv, n_samples, keep in calls:
        m = len(nv)
        if task is not None:
            if len(keep) == m:
                ranks = out[off[at]:off[at + m]]
            else:
                ranks = np.concatenate([out[off[at + i]:off[at + i + 1]] for i in keep]) if keep else np.zeros(0, np.uint32)
            extractor.tasks[task][4] = np.ascontiguousarray(ranks, dtype=np.uint32)
        at += m
    version, _, gauss = random.getstate()
    random.setstate((version, tuple(final.tolist()), gauss))       # where a sequential run would have left the interpreter
    extractor._groups = []


class ScanEngine:
    """One engine per GPU / process.  Mirrors what ``motif_model_bin`` needs (find_motifs_bin.py:1265-1283):
    the bin's contig sequences and the (bin, mod_type) pileup, but resident in HBM across calls."""

    def __init__(self, device: int = 0, ctx=None):
        """``ctx``: an ``nm_ctx *`` (ctypes.c_void_p) on ``device`` that somebody else created — the engine takes it over and destroys it
        in ``close`` (the command line makes it on a thread while the interpreter still imports, __main__.py)."""
        self.lib = _lib.load()
        if ctx is not None:
            self.ctx = ctx
        else:
            self.ctx = C.c_void_p()
            _lib.check(self.lib.nm_ctx_create(int(device), C.byref(self.ctx)))
        self.device = int(device)
        self.contig_index = {}
        self.contig_names = []
        self.contig_lengths = None
        self.contig_bin = None
        self.bin_index = {}
        self.bin_names = []
        self.slot_of_mod = {}
        self.readstats_mods = set()      # mod codes whose read statistics are resident (contig_methylation.upload_read_statistics)
        self.comm_world = 0
        self.regions = C.c_void_p()      # nm_regions * of ``upload_regions``, bound to the resident assembly
        self.region_classes = []

    def close(self):
        self.clear_regions()
        if self.ctx:
            self.lib.nm_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def use_stream(self, hip_stream_handle: int | None):
        """Run engine work on another HIP stream (e.g. a ``torch.cuda.Stream().cuda_stream``); None restores the
        engine's own stream.  The legacy default stream (handle 0) cannot be expressed through nm_set_stream —
        create a side stream and make it torch's current stream instead (see bench.py)."""
        if hip_stream_handle == 0:
            raise ValueError("handle 0 is the legacy default stream: pass a side stream's handle, or None")
        _lib.check(self.lib.nm_set_stream(self.ctx, C.c_void_p(hip_stream_handle or 0)))

    # ------------------------------------------------------------------ assembly
    def upload_assembly(self, names, sequences, bin_of_contig, bin_names=None):
        """names: contig names; sequences: str / bytes / uint8 arrays (any case, IUPAC letters);
        bin_of_contig: bin name per contig.  Bin ids are assigned in sorted bin-name order, or follow
        ``bin_names`` when given (a multi-GPU shard may hold no contig of some bins but must number them alike)."""
        names = list(names)
        if not names and bin_names is None:
            raise ValueError("assembly is empty")
        bufs = []
        for s in sequences:
            if isinstance(s, str):
                s = s.encode("ascii")
            bufs.append(np.frombuffer(s, dtype=np.uint8) if not isinstance(s, np.ndarray) else s.astype(np.uint8, copy=False))
        lengths = np.array([len(b) for b in bufs], dtype=np.uint64)
        offsets = np.zeros(len(bufs) + 1, dtype=np.uint64)
        np.cumsum(lengths, out=offsets[1:])
        # no contig at all = the shard of a rank that received nothing (more GPUs than pieces): it keeps the bin
        # numbering, scores everything to zero and joins every collective (nm_upload_contigs accepts n_contigs = 0)
        ascii_all = np.concatenate(bufs) if len(bufs) > 1 else (np.ascontiguousarray(bufs[0]) if bufs else np.zeros(1, np.uint8))
        self.bin_names = sorted(set(bin_of_contig)) if bin_names is None else list(bin_names)
        self.bin_index = {b: i for i, b in enumerate(self.bin_names)}
        bin_ids = np.array([self.bin_index[b] for b in bin_of_contig], dtype=np.uint32) if names else np.zeros(1, np.uint32)
        self.clear_regions()                   # the planes of a region set are laid out for the assembly they were made on
        _lib.check(self.lib.nm_upload_contigs(self.ctx, len(names), _ptr(offsets, C.c_uint64), _ptr(bin_ids, C.c_uint32),
                                              len(self.bin_names), _ptr(ascii_all, C.c_uint8)))
        self.contig_names = names
        self.contig_index = {n: i for i, n in enumerate(names)}
        self.contig_lengths = lengths.astype(np.int64)
        self.contig_bin = bin_ids
        self.slot_of_mod = {}
        self.readstats_mods = set()      # mod codes whose read statistics are resident (contig_methylation.upload_read_statistics)

    def upload_assembly_device(self, names, lengths, bin_of_contig, device_ptr: int, bin_names=None):
        """``upload_assembly`` for sequences that are already in device memory: ``device_ptr`` addresses the contigs'
        ASCII bytes back to back in the order of ``names`` (nm_upload_contigs_device), e.g. a torch uint8 tensor's
        ``data_ptr()``."""
        names = list(names)
        lengths = np.asarray(lengths, dtype=np.uint64)
        offsets = np.zeros(len(names) + 1, dtype=np.uint64)
        np.cumsum(lengths, out=offsets[1:])
        self.bin_names = sorted(set(bin_of_contig)) if bin_names is None else list(bin_names)
        self.bin_index = {b: i for i, b in enumerate(self.bin_names)}
        bin_ids = np.array([self.bin_index[b] for b in bin_of_contig], dtype=np.uint32)
        self.clear_regions()                   # the planes of a region set are laid out for the assembly they were made on
        _lib.check(self.lib.nm_upload_contigs_device(self.ctx, len(names), _ptr(offsets, C.c_uint64), _ptr(bin_ids, C.c_uint32),
                                                     len(self.bin_names), C.c_void_p(int(device_ptr))))
        self.contig_names = names
        self.contig_index = {n: i for i, n in enumerate(names)}
        self.contig_lengths = lengths.astype(np.int64)
        self.contig_bin = bin_ids
        self.slot_of_mod = {}
        self.readstats_mods = set()      # mod codes whose read statistics are resident (contig_methylation.upload_read_statistics)

    def upload_assembly_fasta(self, assembly, names, bin_of_contig, bin_names=None):
        """``upload_assembly`` for a ``fasta.DeviceAssembly`` (the FASTA was parsed on this device): contig ``names[i]`` is the
        record of that name; the planes are packed straight from the parser's device buffer (nm_upload_contigs_fasta)."""
        names = list(names)
        records = np.array([assembly.record[n] for n in names], dtype=np.uint32)
        self.bin_names = sorted(set(bin_of_contig)) if bin_names is None else list(bin_names)
        self.bin_index = {b: i for i, b in enumerate(self.bin_names)}
        bin_ids = np.array([self.bin_index[b] for b in bin_of_contig], dtype=np.uint32)
        self.clear_regions()                   # the planes of a region set are laid out for the assembly they were made on
        _lib.check(self.lib.nm_upload_contigs_fasta(self.ctx, assembly._h, len(names), _ptr(records, C.c_uint32), _ptr(bin_ids, C.c_uint32),
                                                    len(self.bin_names)))
        self.contig_names = names
        self.contig_index = {n: i for i, n in enumerate(names)}
        self.contig_lengths = np.array([assembly.length(n) for n in names], dtype=np.int64)
        self.contig_bin = bin_ids
        self.slot_of_mod = {}
        self.readstats_mods = set()      # mod codes whose read statistics are resident (contig_methylation.upload_read_statistics)

    def contig_base_counts(self, base: str, padding: int) -> np.ndarray:
        """Per resident contig: positions p in [padding, len - padding) whose base is ``base`` — the number of valid
        starts ``sample_n_subsequences`` draws from (seq.py:202-225)."""
        out = np.zeros(len(self.contig_names), dtype=np.uint64)
        _lib.check(self.lib.nm_contig_base_counts(self.ctx, ord(base), int(padding), _ptr(out, C.c_uint64)))
        return out

    def other_letters(self) -> int:
        """Assembly letters that are none of A C G T N (the reference's window code raises KeyError on them)."""
        n = C.c_uint64(0)
        _lib.check(self.lib.nm_assembly_other_letters(self.ctx, C.byref(n)))
        return int(n.value)

    # ------------------------------------------------------------------ pileup
    def upload_pileup(self, mod_type, contig_id, position, strand, fraction_mod, low=0.3, high=0.7, append=False,
                      label=None):
        """Rows of one mod type after the pre-filters (SoA).  strand: uint8 ASCII '+'/'-'.  ``label`` names the
        resident classification (default: the mod type); a second label of the same mod type holds another
        threshold pair (find_motifs_bin.state_label)."""
        label = mod_type if label is None else label
        if label not in self.slot_of_mod:
            n_slots = len(set(self.slot_of_mod.values()))
            if n_slots >= 8:
                raise ValueError("at most 8 pileup classifications resident")
            self.slot_of_mod[label] = n_slots
        slot = self.slot_of_mod[label]
        cid = np.ascontiguousarray(contig_id, dtype=np.uint32)
        pos = np.ascontiguousarray(position, dtype=np.uint32)
        st = np.ascontiguousarray(strand, dtype=np.uint8)
        fr = np.ascontiguousarray(fraction_mod, dtype=np.float64)
        if not (len(cid) == len(pos) == len(st) == len(fr)):
            raise ValueError("pileup columns differ in length")
        _lib.check(self.lib.nm_upload_pileup(self.ctx, slot, ord(MOD_TYPE_TO_CANONICAL[mod_type]), float(low), float(high),
                                             len(cid), _ptr(cid, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(st, C.c_uint8),
                                             _ptr(fr, C.c_double), 1 if append else 0))

    def ingest_pileup(self, contig_local, position, mod_code, strand, fraction_mod, nvalid_cov, labels, low=0.3, high=0.7,
                      want_rows=True, max_part_rows=None, extra_parts=()):
        """RAW pileup rows -> device-side pre-filters (dataload.py:191-247) -> state planes.
        contig_local: engine contig index per row, 0xFFFFFFFF for contigs this engine does not hold;
        mod_code: int8 ids as numbered by the reader (0 = m, 1 = a, 2 = 21839, 3.. = others, which only take part in
        the filters); labels: {mod code id: (label, canonical base)} for the codes to classify.
        Returns dict(n_kept, n_confident, confident=(contig_local, position, strand, mod_code) of the surviving rows
        with fraction_mod >= high (None unless ``want_rows``: the device keeps them as the methylated-state planes, see
        ``methylated_row_counts`` / ``DeviceWindowStore.add_task_contigs``; ``confident_rows()`` fetches them later),
        kept=uint32[n_contigs, 8] surviving rows per (contig, mod code)).
        ``max_part_rows``: ingest a pileup whose rows are grouped by contig (modkit output is) in parts of about that many
        rows, cut at contig boundaries (nm_ingest_pileup_part) — bounds the device memory of the raw rows and of the
        dense adjacency arrays; the result is the same.  ``extra_parts``: further parts as dicts of the six columns
        (contig, position, mod_type, strand, fraction_mod, nvalid_cov), each holding whole contigs that appear in no other
        part (the rows of a contig that is a member of a second bin, under that placement's contig index)."""
        cid = np.ascontiguousarray(contig_local, dtype=np.uint32)
        pos = np.ascontiguousarray(position, dtype=np.uint32)
        mod = np.ascontiguousarray(mod_code, dtype=np.int8)
        st = np.ascontiguousarray(strand, dtype=np.uint8)
        fr = np.ascontiguousarray(fraction_mod, dtype=np.float64)
        nv = nvalid_cov if getattr(nvalid_cov, "dtype", None) == np.int32 else np.clip(nvalid_cov, -2**31, 2**31 - 1)
        nv = np.ascontiguousarray(nv, dtype=np.int32)
        n = len(cid)
        if not (len(pos) == len(mod) == len(st) == len(fr) == len(nv) == n):
            raise ValueError("pileup columns differ in length")
        slot_of = (C.c_int32 * 8)(*([-1] * 8))
        canon = (C.c_uint8 * 8)(*([0] * 8))
        for code, (label, base) in labels.items():
            if label not in self.slot_of_mod:
                n_slots = len(set(self.slot_of_mod.values()))
                if n_slots >= 8:
                    raise ValueError("at most 8 pileup classifications resident")
                self.slot_of_mod[label] = n_slots
            slot_of[int(code)] = self.slot_of_mod[label]
            canon[int(code)] = ord(base)
        n_kept, n_conf = C.c_uint64(0), C.c_uint64(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        # always ingest in PARTS of whole contigs listing the contigs that have rows (nm_ingest_pileup_part): the dense
        # adjacency scratch (16 B per bp) then covers those contigs only, not the whole resident assembly — a multi-Gbp
        # assembly with a modest pileup would otherwise ask for tens of GB it does not need
        parts = self._pileup_parts(cid, max_part_rows if (max_part_rows and n > max_part_rows) else max(n, 1)) if n else []
        if parts is None:                 # some contig's rows are not contiguous: one part with every contig present
            parts = [(0, n)]
        if n == 0:
            _lib.check(self.lib.nm_ingest_pileup(self.ctx, 0, None, None, None, None, None, None, slot_of, canon,
                                                 float(low), float(high), 0, C.byref(n_kept), C.byref(n_conf)))
        for k, (a, b) in enumerate(parts):
            seg = cid[a:b]
            edge = np.concatenate([[0], np.flatnonzero(seg[1:] != seg[:-1]) + 1]) if b > a else np.zeros(0, np.int64)
            ids = np.unique(seg[edge])
            ids = np.ascontiguousarray(ids[ids != 0xFFFFFFFF], dtype=np.uint32)
            sl = lambda x: vp(x[a:b]) if b > a else None
            _lib.check(self.lib.nm_ingest_pileup_part(self.ctx, b - a, sl(cid), sl(pos), sl(mod), sl(st), sl(fr), sl(nv), slot_of, canon,
                                                      float(low), float(high), 0, 1 if k == 0 else 0, len(ids), _ptr(ids, C.c_uint32),
                                                      C.byref(n_kept), C.byref(n_conf)))
        for x in extra_parts:
            xc = np.ascontiguousarray(x["contig"], dtype=np.uint32)
            cols_x = [xc, np.ascontiguousarray(x["position"], dtype=np.uint32), np.ascontiguousarray(x["mod_type"], dtype=np.int8),
                      np.ascontiguousarray(x["strand"], dtype=np.uint8), np.ascontiguousarray(x["fraction_mod"], dtype=np.float64),
                      np.ascontiguousarray(x["nvalid_cov"], dtype=np.int32)]
            ids = np.ascontiguousarray(np.unique(xc[xc != 0xFFFFFFFF]), dtype=np.uint32)
            if len(xc) == 0:
                continue
            _lib.check(self.lib.nm_ingest_pileup_part(self.ctx, len(xc), *[vp(a) for a in cols_x], slot_of, canon, float(low), float(high), 0,
                                                      0, len(ids), _ptr(ids, C.c_uint32), C.byref(n_kept), C.byref(n_conf)))
        self._n_confident = int(n_conf.value)
        kept = np.zeros((len(self.contig_names), 8), dtype=np.uint32)
        _lib.check(self.lib.nm_ingest_results(self.ctx, None, None, None, None, 0, _ptr(kept, C.c_uint32)))
        return dict(n_kept=int(n_kept.value), n_confident=self._n_confident,
                    confident=self.confident_rows() if want_rows else None, kept=kept)

    def ingest_device_pileup(self, table, lut, labels, low=0.3, high=0.7, max_part_rows=None):
        """``ingest_pileup`` for a ``pileup.DevicePileup`` (columns already in device memory, parsed there): ``lut`` maps
        the file's contig ids to engine contig indices (0xFFFFFFFF: not held here).  Parts are cut at the runs of equal
        contig names the parser reports.  Returns dict(n_kept, n_confident, kept)."""
        lut = np.ascontiguousarray(lut, dtype=np.uint32)
        table.map_contigs(lut)
        ptr = table.device_pointers()
        esz = {"contig": 4, "position": 4, "mod_type": 1, "strand": 1, "fraction_mod": 8, "nvalid_cov": 4}
        slot_of = (C.c_int32 * 8)(*([-1] * 8))
        canon = (C.c_uint8 * 8)(*([0] * 8))
        for code, (label, base) in labels.items():
            if label not in self.slot_of_mod:
                n_slots = len(set(self.slot_of_mod.values()))
                if n_slots >= 8:
                    raise ValueError("at most 8 pileup classifications resident")
                self.slot_of_mod[label] = n_slots
            slot_of[int(code)] = self.slot_of_mod[label]
            canon[int(code)] = ord(base)
        run_eng = lut[table.run_contig]                                   # engine contig of every run
        n = len(table)
        bounds = [0]
        if max_part_rows and n > max_part_rows:
            # a part must hold whole contigs: a run boundary is a cut when every contig seen so far has had its LAST run
            # (a modkit file has one run per contig: every boundary is one; a file that comes back to a contig later is cut
            # behind that contig's last run, so its parts can be larger than asked for — said below, never silently whole)
            last_run = {}
            for r, c in enumerate(run_eng.tolist()):
                if c != 0xFFFFFFFF:
                    last_run[c] = r
            at, open_until = 0, -1
            for r, (c, e) in enumerate(zip(run_eng.tolist(), table.run_row[1:].tolist())):
                if c != 0xFFFFFFFF:
                    open_until = max(open_until, last_run[c])
                if open_until <= r and e - at >= max_part_rows:
                    bounds.append(int(e))
                    at = e
        if bounds[-1] != n:
            bounds.append(n)
        part_rows = [b - a for a, b in zip(bounds, bounds[1:])]          # empty for a table without rows
        if max_part_rows and part_rows and max(part_rows) > 2 * max_part_rows:
            import logging
            logging.warning(f"pileup rows are not grouped by contig: ingestion parts of up to {max(part_rows):,} rows "
                            f"instead of {max_part_rows:,} (device memory for the raw rows and the adjacency scratch grows with them)")
        n_kept, n_conf = C.c_uint64(0), C.c_uint64(0)
        for k in range(len(bounds) - 1):
            a, b = bounds[k], bounds[k + 1]
            in_part = (table.run_row[:-1] >= a) & (table.run_row[:-1] < b)
            ids = np.unique(run_eng[in_part])
            ids = np.ascontiguousarray(ids[ids != 0xFFFFFFFF], dtype=np.uint32)
            col = lambda name: C.c_void_p(ptr[name] + a * esz[name])
            _lib.check(self.lib.nm_ingest_pileup_part(self.ctx, b - a, col("contig"), col("position"), col("mod_type"), col("strand"),
                                                      col("fraction_mod"), col("nvalid_cov"), slot_of, canon, float(low), float(high), 1,
                                                      1 if k == 0 else 0, len(ids), _ptr(ids, C.c_uint32), C.byref(n_kept), C.byref(n_conf)))
        self._n_confident = int(n_conf.value)
        kept = np.zeros((len(self.contig_names), 8), dtype=np.uint32)
        _lib.check(self.lib.nm_ingest_results(self.ctx, None, None, None, None, 0, _ptr(kept, C.c_uint32)))
        return dict(n_kept=int(n_kept.value), n_confident=self._n_confident, confident=None, kept=kept)

    @staticmethod
    def _pileup_parts(cid: np.ndarray, max_rows: int):
        """[(begin, end)] row ranges of about ``max_rows`` rows cut where the contig id changes, or None when some contig's
        rows are not contiguous (then the pileup has to be ingested in one piece)."""
        change = np.flatnonzero(cid[1:] != cid[:-1]) + 1
        starts = np.concatenate([[0], change])
        ids = cid[starts]
        real = ids[ids != 0xFFFFFFFF]
        if len(np.unique(real)) != len(real):
            return None
        ends = np.concatenate([change, [len(cid)]])
        parts, a = [], 0
        for e in ends.tolist():
            if e - a >= max_rows:
                parts.append((a, e))
                a = e
        if a < len(cid):
            parts.append((a, len(cid)))
        return parts

    def confident_rows(self):
        """(contig_local, position, strand, mod_code) of the rows the last ``ingest_pileup`` kept with
        fraction_mod >= high, copied from the device."""
        k = getattr(self, "_n_confident", 0)
        cc, cp = np.empty(k, np.uint32), np.empty(k, np.uint32)
        cs, cm = np.empty(k, np.uint8), np.empty(k, np.int8)
        if k:
            _lib.check(self.lib.nm_ingest_results(self.ctx, _ptr(cc, C.c_uint32), _ptr(cp, C.c_uint32), _ptr(cs, C.c_uint8),
                                                  cm.ctypes.data_as(C.POINTER(C.c_int8)), k, None))
        return cc, cp, cs, cm

    def methylated_row_counts(self, label, padding: int) -> np.ndarray:
        """uint64[n_contigs, 2]: confidently methylated rows (plus, minus) of the classification ``label`` per resident
        contig with padding < position < len - padding — the rows window extraction uses."""
        out = np.zeros((len(self.contig_names), 2), dtype=np.uint64)
        _lib.check(self.lib.nm_methylated_row_counts(self.ctx, self.slot_of_mod[label], int(padding), _ptr(out, C.c_uint64)))
        return out

    def alias_label(self, label, existing):
        """Make ``label`` refer to the classification already resident as ``existing``."""
        self.slot_of_mod[label] = self.slot_of_mod[existing]

    # ------------------------------------------------------------------ scoring
    def make_batch(self, candidates, slot_of=None) -> CandidateBatch:
        """candidates: sequence of (Motif, mod_type, bin name or id).  Parsing / stripping is done natively
        (nm_parse_motifs); Python only joins the strings.  ``slot_of``: mod type -> slot number, default the resident
        classifications (``slot_of_mod``)."""
        n = len(candidates)
        strings = [c[0].string for c in candidates]
        text = "".join(strings).encode("ascii")
        offsets = np.zeros(n + 1, dtype=np.uint32)
        np.cumsum(np.fromiter((len(s) for s in strings), dtype=np.uint32, count=n), out=offsets[1:])
        modpos_in = np.fromiter((c[0].mod_position for c in candidates), dtype=np.int32, count=n)
        bi, so = self.bin_index, self.slot_of_mod
        bins = np.fromiter((bi[c[2]] if isinstance(c[2], str) else c[2] for c in candidates), dtype=np.uint32, count=n)
        slots = np.fromiter(((so[c[1]] if slot_of is None else slot_of(c[1])) for c in candidates), dtype=np.uint8, count=n)
        lens = np.empty(n, dtype=np.uint8)
        modpos = np.empty(n, dtype=np.uint8)
        moff = np.empty(n, dtype=np.uint32)
        masks = np.empty(max(len(text), 1), dtype=np.uint8)
        used = C.c_uint64(0)
        _lib.check(self.lib.nm_parse_motifs(n, text, _ptr(offsets, C.c_uint32), _ptr(modpos_in, C.c_int32),
                                            _ptr(lens, C.c_uint8), _ptr(modpos, C.c_uint8), _ptr(moff, C.c_uint32),
                                            _ptr(masks, C.c_uint8), len(masks), C.byref(used)))
        return CandidateBatch(bins, slots, lens, modpos, moff, masks[:used.value])

    def _batch_args(self, b: CandidateBatch):
        args = getattr(b, "_args", None)            # the ctypes views are reusable as long as the arrays live
        if args is None:
            args = (len(b), _ptr(b.bins, C.c_uint32), _ptr(b.slots, C.c_uint8), _ptr(b.lens, C.c_uint8),
                    _ptr(b.modpos, C.c_uint8), _ptr(b.offsets, C.c_uint32), _ptr(b.masks, C.c_uint8))
            b._args = args
        return args

    def _as_batch(self, candidates, slot_of=None) -> CandidateBatch:
        """``candidates`` as a CandidateBatch: itself if it is one, else ``make_batch`` of the sequence."""
        return candidates if isinstance(candidates, CandidateBatch) else self.make_batch(list(candidates), slot_of=slot_of)

    def score(self, candidates) -> np.ndarray:
        """int64[n, 2] = (n_mod, n_nomod) per candidate — what ``model.update`` receives (find_motifs_bin.py:1320)."""
        if not isinstance(candidates, CandidateBatch) and any(len(c[0].tokens) > MAX_REACH + 1 for c in candidates):
            return self._score_with_wide(candidates)
        b = self._as_batch(candidates)
        out = np.zeros((len(b), 2), dtype=np.int64)
        if len(b):
            _lib.check(self.lib.nm_score_batch(self.ctx, *self._batch_args(b), out.ctypes.data_as(C.c_void_p)))
        return out

    def _score_with_wide(self, candidates) -> np.ndarray:
        """A search frame above 191 (find_motifs_bin.py:110-130 takes any): candidates that stay within 95 positions of the
        modified base once stripped go the usual way, the others through nm_score_batch_wide (plain kernel, any reach)."""
        stripped = [c[0].stripped_sets() for c in candidates]
        wide = [k for k, (sets, mp) in enumerate(stripped) if max(mp, len(sets) - 1 - mp) > MAX_REACH or len(sets) > MAX_MOTIF_LEN]
        is_wide = set(wide)
        narrow = [k for k in range(len(candidates)) if k not in is_wide]
        out = np.zeros((len(candidates), 2), dtype=np.int64)
        if narrow:
            out[narrow] = self.score(self.make_batch([candidates[k] for k in narrow]))
        if wide:
            n = len(wide)
            bi, so = self.bin_index, self.slot_of_mod
            bins = np.fromiter((bi[candidates[k][2]] if isinstance(candidates[k][2], str) else candidates[k][2] for k in wide), dtype=np.uint32, count=n)
            slots = np.fromiter((so[candidates[k][1]] for k in wide), dtype=np.uint8, count=n)
            lens = np.fromiter((len(stripped[k][0]) for k in wide), dtype=np.uint16, count=n)
            modpos = np.fromiter((stripped[k][1] for k in wide), dtype=np.uint16, count=n)
            moff = np.zeros(n, dtype=np.uint32)
            np.cumsum(lens[:-1], out=moff[1:])
            masks = np.concatenate([stripped[k][0] for k in wide]).astype(np.uint8)
            res = np.zeros((n, 2), dtype=np.int64)
            _lib.check(self.lib.nm_score_batch_wide(self.ctx, n, _ptr(bins, C.c_uint32), _ptr(slots, C.c_uint8), _ptr(lens, C.c_uint16),
                                                    _ptr(modpos, C.c_uint16), _ptr(moff, C.c_uint32), _ptr(masks, C.c_uint8), _ptr(res, C.c_int64)))
            out[wide] = res
            self.wide_scored = getattr(self, "wide_scored", 0) + n
        return out

    def bin_contigs(self, bin_name) -> list:
        """Resident contig names of a bin in the row order of ``score_per_contig`` (nm_bin_contigs)."""
        b = self.bin_index[bin_name] if isinstance(bin_name, str) else int(bin_name)
        n = C.c_uint32(0)
        _lib.check(self.lib.nm_bin_contigs(self.ctx, b, None, 0, C.byref(n)))
        ids = np.zeros(max(n.value, 1), dtype=np.uint32)
        _lib.check(self.lib.nm_bin_contigs(self.ctx, b, _ptr(ids, C.c_uint32), n.value, C.byref(n)))
        return [self.contig_names[i] for i in ids[:n.value].tolist()]

    def score_per_contig(self, candidates):
        """Per-contig (n_mod, n_nomod): ``motif_model_contig`` (find_motifs_bin.py:1285-1331) for every resident contig of
        each candidate's bin in one launch (nm_score_batch_per_contig).  Returns a list, per candidate, of
        (contig names, int64[n_contigs, 2])."""
        b = self._as_batch(candidates)
        names = {}
        for bid in np.unique(b.bins).tolist():
            names[bid] = self.bin_contigs(int(bid))
        rows = np.zeros(len(b) + 1, dtype=np.uint64)
        np.cumsum([len(names[int(x)]) for x in b.bins], out=rows[1:])
        out = np.zeros((max(int(rows[-1]), 1), 2), dtype=np.int64)
        if len(b):
            _lib.check(self.lib.nm_score_batch_per_contig(self.ctx, *self._batch_args(b), _ptr(rows, C.c_uint64), _ptr(out, C.c_int64)))
        return [(names[int(b.bins[k])], out[int(rows[k]):int(rows[k + 1])]) for k in range(len(b))]

    # ------------------------------------------------------------------ per-site export (nm_motif_sites*)
    def _site_rows(self, b: CandidateBatch):
        names = {int(bid): self.bin_contigs(int(bid)) for bid in np.unique(b.bins).tolist()}
        rows = np.zeros(len(b) + 1, dtype=np.uint64)
        np.cumsum([len(names[int(x)]) for x in b.bins], out=rows[1:])
        return names, rows

    def _count_table(self, call, args, b: CandidateBatch, selection: int, width: int):
        """(contig names per bin, row prefix, totals under ``selection``, int64[rows, width]) of one count call of the per-candidate
        exports (nm_motif_sites_count, nm_motif_compare_count, nm_motif_strands_count); ``args``: the call's candidate arguments."""
        names, rows = self._site_rows(b)
        table = np.zeros((max(int(rows[-1]), 1), width), dtype=np.int64)
        totals = np.zeros(max(len(b), 1), dtype=np.uint64)
        if len(b):
            _lib.check(call(self.ctx, *args, int(selection), _ptr(rows, C.c_uint64), _ptr(totals, C.c_uint64), _ptr(table, C.c_int64)))
        return names, rows, totals[:len(b)], table[:int(rows[-1])]

    @staticmethod
    def _record_limit(max_records, record_bytes=SITE_RECORD_BYTES) -> int:
        limit = SITE_BUDGET_BYTES // record_bytes if max_records is None else int(max_records)
        if limit < 1:
            raise ValueError("max_records must be at least 1")
        return limit

    def _record_windows(self, call, group_args, totals, limit: int, dtype, owner: str, unit: str, values=()):
        """The window loop of the record exports: consecutive owners (candidates, sets) are grouped while their ``totals`` fit
        ``limit``, and every group is fetched in windows of at most ``limit`` records — one, unless a single owner exceeds the limit.
        ``call``: the library's *_sites function; ``group_args(k, e)``: its arguments before first_record for the owners [k, e);
        ``dtype``: the records' type, whose ``owner`` field is filled in here; ``unit``: what the library's message calls a group;
        ``values``: the fields of ``dtype`` the call writes after the code, in the call's order — a name (a uint32 column;
        nm_motif_pileup_sites: n_valid, n_mod) or (name, numpy type) (nm_motif_regions_sites: the class byte).
        The ctypes pointers of those arguments keep their arrays alive.  Yields (k, e, first_record, records of the group, the window's
        records)."""
        columns = [(v, np.uint32) if isinstance(v, str) else v for v in values]
        for k, e, held in _budget_groups(totals, limit):
            args = group_args(k, e)
            first = 0
            while True:
                cap = min(limit, held - first) if held else 0
                rec = np.zeros(cap, dtype=dtype)
                contig, pos, code = (np.zeros(max(cap, 1), dtype=t) for t in (np.uint32, np.uint32, np.uint8))
                more = [np.zeros(max(cap, 1), dtype=t) for _, t in columns]
                off = np.zeros(e - k + 1, dtype=np.uint64)
                written = C.c_uint64(0)
                _lib.check(call(*args, first, cap, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8),
                                *(_ptr(m, np.ctypeslib.as_ctypes_type(m.dtype)) for m in more), _ptr(off, C.c_uint64), C.byref(written)))
                if int(off[-1]) != held or written.value != cap:
                    raise _lib.NmScanError(f"{call.__name__} delivered {written.value} of {cap} records ({int(off[-1])} in the {unit}, {held} counted)")
                rec["contig"], rec["pos"], rec["code"] = contig[:cap], pos[:cap], code[:cap]
                for (name, _), m in zip(columns, more):
                    rec[name] = m[:cap]
                # the owner of every record of the window: the prefix of the group, cut to [first, first + cap)
                cut = np.clip(off.astype(np.int64) - first, 0, cap)
                rec[owner] = np.repeat(np.arange(k, e, dtype=np.uint32), np.diff(cut))
                yield k, e, first, held, rec
                first += cap
                if first >= held:
                    break

    def _site_batches(self, windows, b: CandidateBatch, names, rows, table):
        """The windows of ``_record_windows`` over the candidates ``b`` as ``SiteBatch`` objects."""
        for k, e, first, held, rec in windows:
            counts = [(names[int(b.bins[j])], table[int(rows[j]):int(rows[j + 1])]) for j in range(k, e)] if first == 0 else None
            yield SiteBatch(first_candidate=k, n_candidates=e - k, first_record=first, batch_records=held, records=rec, counts=counts)

    def _site_counts(self, b: CandidateBatch, state_set: int):
        return self._count_table(self.lib.nm_motif_sites_count, self._batch_args(b), b, state_set, 6)

    def motif_site_counts(self, candidates):
        """Per (candidate, contig) the six site counts (fwd mod, fwd nomod, fwd nocall, rev mod, rev nomod, rev nocall) of every
        resident contig of the candidate's bin (nm_motif_sites_count): ``score_per_contig`` split by strand, plus the occurrences
        that carry no call.  Returns a list, per candidate, of (contig names, int64[n_contigs, 6])."""
        b = self._as_batch(candidates)
        names, rows, _, table = self._site_counts(b, 7)
        return [(names[int(b.bins[k])], table[int(rows[k]):int(rows[k + 1])]) for k in range(len(b))]

    def motif_sites(self, candidates, states=SITE_STATES, max_records=None):
        """Generator over the sites of ``candidates`` (sequence of (Motif, mod_type, bin), or a CandidateBatch): what
        ``motif_model_contig(..., save_motif_positions=True)`` returns per motif and contig (find_motifs_bin.py:1285-1331), for the
        whole list, plus the occurrences without a call.  Yields ``SiteBatch`` objects in candidate order; their ``records``
        (fields candidate, contig, pos, code; code = 4 for the '-' strand | 0 mod / 1 nomod / 2 nocall) concatenated are the sites
        in the order candidate, contig (``bin_contigs`` order), position, '+' before '-'.  No batch holds more than ``max_records``
        records (default: ``SITE_BUDGET_BYTES`` = 256 MiB of device records, 9 bytes each); a candidate with more is delivered in
        several windows.  The concatenation does not depend on ``max_records``."""
        b = self._as_batch(candidates)
        state_set = site_state_set(states)
        limit = self._record_limit(max_records)
        names, rows, totals, table = self._site_counts(b, state_set)

        def group_args(k, e):
            sub = b.slice(k, e)
            return (self.ctx, *self._batch_args(sub), state_set)
        windows = self._record_windows(self.lib.nm_motif_sites, group_args, totals, limit, SITE_DTYPE, "candidate", "batch")
        yield from self._site_batches(windows, b, names, rows, table)

    # ------------------------------------------------------------------ two-sample comparison (nm_motif_compare_*)
    def _compare_batch(self, candidates, labels_a_b):
        """(CandidateBatch whose slots are sample A's, uint8 slots of sample B).  ``labels_a_b``: the classifications of the two
        samples — a pair (label or slot number of A, of B) for every candidate, or a mapping / callable from a candidate's mod type to
        such a pair."""
        if isinstance(labels_a_b, (tuple, list)):
            pair_of = lambda mt: labels_a_b
        elif callable(labels_a_b):
            pair_of = labels_a_b
        else:
            pair_of = labels_a_b.__getitem__
        so = self.slot_of_mod
        slot = lambda x: so[x] if isinstance(x, str) else int(x)
        candidates = list(candidates)
        b = self.make_batch(candidates, slot_of=lambda mt: slot(pair_of(mt)[0]))
        slots_b = np.fromiter((slot(pair_of(c[1])[1]) for c in candidates), dtype=np.uint8, count=len(candidates))
        return b, slots_b

    @staticmethod
    def _compare_args(b: CandidateBatch, slots_b):
        return (len(b), _ptr(b.bins, C.c_uint32), _ptr(b.slots, C.c_uint8), _ptr(slots_b, C.c_uint8), _ptr(b.lens, C.c_uint8),
                _ptr(b.modpos, C.c_uint8), _ptr(b.offsets, C.c_uint32), _ptr(b.masks, C.c_uint8))

    def _compare_counts(self, b: CandidateBatch, slots_b, tset: int):
        return self._count_table(self.lib.nm_motif_compare_count, self._compare_args(b, slots_b), b, tset, 18)

    def motif_compare_counts(self, candidates, labels_a_b):
        """Per (candidate, contig) the eighteen transition counts of every resident contig of the candidate's bin between two resident
        classifications (nm_motif_compare_count): column 3 * state_a + state_b of the forward strand, then 9 + that of the reverse
        strand; states 0 mod, 1 nomod, 2 nocall.  ``candidates``: sequence of (Motif, mod_type, bin); ``labels_a_b``: see
        ``_compare_batch``.  Returns a list, per candidate, of (contig names, int64[n_contigs, 18])."""
        b, slots_b = self._compare_batch(candidates, labels_a_b)
        names, rows, _, table = self._compare_counts(b, slots_b, 0x1FF)
        return [(names[int(b.bins[k])], table[int(rows[k]):int(rows[k + 1])]) for k in range(len(b))]

    def motif_compare_sites(self, candidates, labels_a_b, transitions=SWITCHED, max_records=None):
        """Generator over the occurrences of ``candidates`` whose transition between the two samples is one of ``transitions``
        (``TRANSITIONS`` spellings; default the two discordant called ones).  Yields ``SiteBatch`` objects as ``motif_sites`` does
        (``counts``: the int64[n_contigs, 18] tables); a record's code = 16 for the '-' strand | transition 0..8.  Order: candidate,
        contig (``bin_contigs`` order), position, '+' before '-'.  No batch holds more than ``max_records`` records; the concatenation
        does not depend on ``max_records``."""
        b, slots_b = self._compare_batch(candidates, labels_a_b)
        tset = transition_set(transitions)
        limit = self._record_limit(max_records)
        names, rows, totals, table = self._compare_counts(b, slots_b, tset)

        def group_args(k, e):
            sub = b.slice(k, e)
            return (self.ctx, *self._compare_args(sub, np.ascontiguousarray(slots_b[k:e])), tset)
        windows = self._record_windows(self.lib.nm_motif_compare_sites, group_args, totals, limit, SITE_DTYPE, "candidate", "batch")
        yield from self._site_batches(windows, b, names, rows, table)

    # ------------------------------------------------------------------ both strands of a site (nm_motif_strands_*)
    def _strands_batch(self, candidates):
        """(CandidateBatch, int8 partner offsets) of ``candidates`` = sequence of (Motif, mod_type, bin, partner_position).  An offset
        beyond int8 is clipped: it lies outside every motif within the reach limit, and the library refuses it by name."""
        candidates = list(candidates)
        b = self.make_batch([c[:3] for c in candidates])
        d = np.fromiter((max(-128, min(127, partner_offset(c[0], c[3]))) for c in candidates), dtype=np.int8, count=len(candidates))
        return b, d

    @staticmethod
    def _strands_args(b: CandidateBatch, d):
        return (len(b), _ptr(b.bins, C.c_uint32), _ptr(b.slots, C.c_uint8), _ptr(d, C.c_int8), _ptr(b.lens, C.c_uint8), _ptr(b.modpos, C.c_uint8),
                _ptr(b.offsets, C.c_uint32), _ptr(b.masks, C.c_uint8))

    def _strands_counts(self, b: CandidateBatch, d, pset: int):
        return self._count_table(self.lib.nm_motif_strands_count, self._strands_args(b, d), b, pset, 18)

    def motif_strand_counts(self, candidates):
        """Per (candidate, contig) the eighteen pair counts of every resident contig of the candidate's bin (nm_motif_strands_count):
        column 3 * own state + partner state of the occurrences on '+', then 9 + that of the occurrences on '-'; states 0 mod, 1 nomod,
        2 nocall.  ``candidates``: sequence of (Motif, mod_type, bin, partner_position) — the partner's modified base is at
        ``partner_position`` of the motif's reverse complement, on the opposite strand (``partner_offset``).  Returns a list, per
        candidate, of (contig names, int64[n_contigs, 18])."""
        b, d = self._strands_batch(candidates)
        names, rows, _, table = self._strands_counts(b, d, 0x1FF)
        return [(names[int(b.bins[k])], table[int(rows[k]):int(rows[k + 1])]) for k in range(len(b))]

    def motif_strand_sites(self, candidates, pairs=HEMI, max_records=None):
        """Generator over the occurrences of ``candidates`` whose (own, partner) pair is one of ``pairs`` (``PAIRS`` spellings; default
        the two hemimethylated ones).  Yields ``SiteBatch`` objects as ``motif_sites`` does (``counts``: the int64[n_contigs, 18]
        tables); a record's position is that of the OWN base, its code = 16 for an occurrence on '-' | pair 0..8.  Order: candidate,
        contig (``bin_contigs`` order), position, '+' before '-'.  No batch holds more than ``max_records`` records; the concatenation
        does not depend on ``max_records``."""
        b, d = self._strands_batch(candidates)
        pset = pair_set(pairs)
        limit = self._record_limit(max_records)
        names, rows, totals, table = self._strands_counts(b, d, pset)

        def group_args(k, e):
            sub = b.slice(k, e)
            return (self.ctx, *self._strands_args(sub, np.ascontiguousarray(d[k:e])), pset)
        windows = self._record_windows(self.lib.nm_motif_strands_sites, group_args, totals, limit, SITE_DTYPE, "candidate", "batch")
        yield from self._site_batches(windows, b, names, rows, table)

    # ------------------------------------------------------------------ profile around a motif's sites (nm_motif_profile_count)
    def _profile_targets(self, targets):
        """(labels, uint8 slots) of ``targets`` = labels or slot numbers; None: every resident classification in slot order (a slot that
        several labels name appears once, under the label that came first)."""
        so = self.slot_of_mod
        if targets is None:
            first = {}
            for label, slot in so.items():
                first.setdefault(int(slot), label)
            targets = [first[s] for s in sorted(first)]
        targets = list(targets)
        if not targets:
            raise ValueError("motif_profile needs at least one target classification")
        label_of_slot = {}
        for label, slot in so.items():
            label_of_slot.setdefault(int(slot), label)
        labels, slots = [], []
        for t in targets:
            if isinstance(t, str):
                if t not in so:
                    raise ValueError(f"target {t!r} is not a resident classification ({', '.join(map(str, so)) or 'none'})")
                labels.append(t)
                slots.append(int(so[t]))
            else:
                labels.append(label_of_slot.get(int(t), str(int(t))))
                slots.append(int(t))
        return labels, np.asarray(slots, dtype=np.uint8)

    def motif_profile(self, candidates, targets=None, radius=10):
        """The methylation of every position around the sites of ``candidates`` (sequence of (Motif, mod_type, bin), or a
        CandidateBatch; a candidate's mod type plays no part: occurrences depend on the sequence only) under the classifications
        ``targets`` (labels or slot numbers; default every resident one in slot order), nm_motif_profile_count.  An occurrence has its
        modified base at p on occurrence strand s (0 '+', 1 '-'); offset o counts in the motif's reading direction, relative strand r is
        0 for the occurrence's strand and 1 for the opposite one; the probe is (p + o, s ^ r) for s = 0 and (p - o, s ^ r) for s = 1.
        Returns (target labels, sites int64[n, 2] = occurrences per occurrence strand, table int64[n, n_targets, 2 radius + 1, 2 (s),
        2 (r), 4]) with the classes mod, nomod, nocall (no call, and the letter read on the probed strand is the target's canonical
        base) and other (the rest); offset o is at index o + radius; the four classes sum to ``sites[:, s]``.  Counts are summed over
        the contigs of the candidate's bin."""
        radius = int(radius)
        if not 0 <= radius <= PROFILE_MAX_RADIUS:
            raise ValueError(f"radius {radius} outside 0..{PROFILE_MAX_RADIUS}")
        labels, slots = self._profile_targets(targets)
        b = self._as_batch(candidates, slot_of=lambda mt: 0)
        n, nt, width = len(b), len(slots), 2 * radius + 1
        sites = np.zeros((n, 2), dtype=np.uint64)
        three = np.zeros((n, nt, width, 2, 2, 3), dtype=np.int64)
        if n:
            _lib.check(self.lib.nm_motif_profile_count(self.ctx, n, _ptr(b.bins, C.c_uint32), _ptr(b.lens, C.c_uint8), _ptr(b.modpos, C.c_uint8),
                                                       _ptr(b.offsets, C.c_uint32), _ptr(b.masks, C.c_uint8), nt, _ptr(slots, C.c_uint8), radius,
                                                       _ptr(sites, C.c_uint64), _ptr(three, C.c_int64)))
        sites = sites.astype(np.int64)
        table = np.empty((n, nt, width, 2, 2, 4), dtype=np.int64)
        table[..., :3] = three
        table[..., 3] = sites[:, None, None, :, None] - three.sum(axis=-1)
        return labels, sites, table

    # ------------------------------------------------------------------ sequence context of a motif's sites (nm_motif_context_count)
    def motif_context(self, candidates, radius=10):
        """The contig's letter at every offset around the sites of ``candidates`` (sequence of (Motif, mod_type, bin), or a
        CandidateBatch with slots from ``slot_of_mod``, as ``motif_site_counts`` takes them), counted apart by the state of the site
        itself (nm_motif_context_count).  An occurrence has its modified base at p on occurrence strand s (0 '+', 1 '-') and the state
        ``motif_site_counts`` gives it; offset o counts in the motif's reading direction: the probe is p + o for s = 0 and p - o for
        s = 1, its letter the contig's read on strand s.  Returns (states int64[n, 2 (s), 3 (mod, nomod, nocall)], table int64[n,
        2 radius + 1, 2 (s), 3 (state), 5 (A, C, G, T, other)]); ``other`` is N, any other character and a position outside the
        contig; offset o is at index o + radius; every (offset, s, state) row sums to ``states[:, s, state]``.  The cell (o, X) is the
        ``states`` of the candidate narrowed to X at o.  Counts are summed over the contigs of the candidate's bin."""
        radius = int(radius)
        if not 0 <= radius <= CONTEXT_MAX_RADIUS:
            raise ValueError(f"radius {radius} outside 0..{CONTEXT_MAX_RADIUS}")
        b = self._as_batch(candidates)
        n, width = len(b), 2 * radius + 1
        states = np.zeros((n, 2, 3), dtype=np.uint64)
        four = np.zeros((n, width, 2, 3, 4), dtype=np.int64)
        if n:
            _lib.check(self.lib.nm_motif_context_count(self.ctx, *self._batch_args(b), radius, _ptr(states, C.c_uint64), _ptr(four, C.c_int64)))
        states = states.astype(np.int64)
        table = np.empty((n, width, 2, 3, 5), dtype=np.int64)
        table[..., :4] = four
        table[..., 4] = states[:, None, :, :] - four.sum(axis=-1)
        return states, table

    # ------------------------------------------------------------------ methylation of every k-mer context (nm_kmer_methylation)
    def kmer_methylation(self, requests, shape, max_bytes=None):
        """The methylation of EVERY sequence context of a shape around the A (or C) of a bin, without a motif (nm_kmer_methylation).
        ``requests``: sequence of (mod type or slot number, bin name or id); ``shape``: see ``kmer_shape``, F counted offsets in the
        reading direction of the site's strand.  Sites are the positions that hold the slot's canonical base X ('+') or its complement
        (a site on '-'); the state of a site is ``motif_site_counts``'.  Returns (totals int64[n, 2 (strand), 3 (mod, nomod, nocall)]:
        all sites = ``motif_site_counts`` of the one-letter motif X summed over the bin's contigs; table int64[n, 4^F, 3]: the sites
        whose F probed positions all lie inside the contig and hold A, C, G or T, summed over strands and contigs, row = the base-4
        number of the letters (``kmer_text`` / ``kmer_motif`` spell a row).  Consecutive requests share one library call while their
        tables fit ``max_bytes`` (default ``KMER_BUDGET_BYTES``; a request is 24 x 4^F bytes); a call holds at least one request.  The
        result does not depend on ``max_bytes``."""
        offsets = np.asarray(kmer_shape(shape), dtype=np.int8)
        limit = _byte_limit(max_bytes, KMER_BUDGET_BYTES)
        requests = list(requests)
        n, rows = len(requests), 4 ** len(offsets)
        bi, so = self.bin_index, self.slot_of_mod
        slots = np.fromiter((so[r[0]] if isinstance(r[0], str) else int(r[0]) for r in requests), dtype=np.uint8, count=n)
        bins = np.fromiter((bi[r[1]] if isinstance(r[1], str) else int(r[1]) for r in requests), dtype=np.uint32, count=n)
        totals = np.zeros((n, 2, 3), dtype=np.uint64)
        table = np.zeros((n, rows, 3), dtype=np.uint64)
        off = np.ascontiguousarray(offsets) if len(offsets) else np.zeros(1, dtype=np.int8)
        for k, e, _ in _budget_groups([rows * 24 + 48] * n, limit):
            b, s = np.ascontiguousarray(bins[k:e]), np.ascontiguousarray(slots[k:e])
            _lib.check(self.lib.nm_kmer_methylation(self.ctx, e - k, _ptr(b, C.c_uint32), _ptr(s, C.c_uint8), len(offsets), _ptr(off, C.c_int8),
                                                    _ptr(totals[k:e], C.c_uint64), _ptr(table[k:e], C.c_uint64)))
        return totals.astype(np.int64), table.astype(np.int64)

    # ------------------------------------------------------------------ methylation along contigs (nm_tracks_windows, nm_motif_tracks_count)
    def track_windows(self, bin, window) -> np.ndarray:
        """int64[n_contigs + 1]: the prefix of the window counts over the resident contigs of ``bin`` in ``bin_contigs`` order at window
        size ``window`` (nm_tracks_windows, the one definition of the row layout of ``motif_tracks``): a contig of length L has
        max(1, ceil(L / window)) windows, window i covers [i window, min((i + 1) window, L))."""
        w = track_window(window)
        b = self.bin_index[bin] if isinstance(bin, str) else int(bin)
        n = C.c_uint32(0)
        _lib.check(self.lib.nm_tracks_windows(self.ctx, b, w, None, 0, C.byref(n)))
        off = np.zeros(n.value + 1, dtype=np.uint64)
        _lib.check(self.lib.nm_tracks_windows(self.ctx, b, w, _ptr(off, C.c_uint64), n.value, C.byref(n)))
        return off.astype(np.int64)

    def motif_tracks(self, candidates, window=4096, max_bytes=None):
        """Generator over the methylation of ``candidates`` (sequence of (Motif, mod_type, bin), or a CandidateBatch) ALONG the contigs of
        their bins (nm_motif_tracks_count).  Yields one item per candidate, in candidate order: (contig names in ``bin_contigs`` order,
        the window prefix int64[n_contigs + 1] of ``track_windows``, uint32[n_windows, 6]) — per window the six counts of
        ``motif_site_counts`` (fwd mod, fwd nomod, fwd nocall, rev mod, rev nomod, rev nocall) of the occurrences whose modified base
        lies in it, contigs in order, windows ascending.  ``window``: a multiple of 128 in [128, 2^30].  Consecutive candidates share
        one library call while their tables fit ``max_bytes`` (default ``TRACK_BUDGET_BYTES`` = 256 MiB at 24 bytes a row); a group
        always holds at least one candidate.  What is yielded does not depend on ``max_bytes``."""
        w = track_window(window)
        limit = _byte_limit(max_bytes, TRACK_BUDGET_BYTES)
        return self._track_groups(self._as_batch(candidates), w, limit)

    def _bin_names(self, b: CandidateBatch) -> dict:
        """{bin id: the names of its resident contigs} of the bins of a batch."""
        return {bid: self.bin_contigs(bid) for bid in sorted({int(x) for x in b.bins})}

    def _track_groups(self, b: CandidateBatch, w: int, limit: int):
        names = self._bin_names(b)
        prefix = {bid: self.track_windows(bid, w) for bid in names}

        def call(k, e, sub, rows, table):
            _lib.check(self.lib.nm_motif_tracks_count(self.ctx, *self._batch_args(sub), w, _ptr(rows, C.c_uint64), _ptr(table, C.c_uint32)))
        n_rows = [int(prefix[int(bid)][-1]) for bid in b.bins]
        for j, contigs, table in _table_groups(b, names, n_rows, TRACK_ROW_BYTES, limit, (6,), np.uint32, call):
            yield contigs, prefix[int(b.bins[j])], table

    # ------------------------------------------------------------------ read-fraction histograms at motif sites (nm_motif_fractions_count)
    def motif_fractions(self, candidates, bins=20, max_bytes=None):
        """Generator over the read-fraction histograms of ``candidates`` (sequence of (Motif, mod_type, bin)) on the contigs of their
        bins, read against the READ STATISTICS of the candidate's mod code (``contig_methylation.upload_read_statistics`` /
        ``read_statistics_device``), nm_motif_fractions_count.  Yields one item per candidate, in call order: (the candidate, contig names
        in ``bin_contigs`` order, uint64[n_contigs, 2, bins + 3]) — per strand (0: the motif on '+' against '+' records, 1: its reverse
        complement on '-' against '-' records) the histogram of the sites' n_modified / n_valid_cov over ``bins`` equal bins (a site's bin
        is min(bins - 1, n_modified * bins // n_valid_cov)), then the occurrences (with or without a record), the sum of n_valid_cov and
        the sum of n_modified over the sites.  ``bins``: 2..64.  A candidate of a mod code without resident read statistics is a
        ValueError.  Consecutive candidates share one library call while their table fits ``max_bytes`` (default
        ``FRACTIONS_BUDGET_BYTES``); a group always holds at least one candidate.  What is yielded does not depend on ``max_bytes``."""
        bins = int(bins)
        if not FRACTIONS_MIN_BINS <= bins <= FRACTIONS_MAX_BINS:
            raise ValueError(f"bins {bins} outside {FRACTIONS_MIN_BINS}..{FRACTIONS_MAX_BINS}")
        limit = _byte_limit(max_bytes, FRACTIONS_BUDGET_BYTES)
        candidates = list(candidates)
        return self._fraction_groups(candidates, self._readstats_batch(candidates), bins, limit)

    def _readstats_batch(self, candidates: list) -> CandidateBatch:
        """``candidates`` with their slots naming READ-STATISTICS slots; a mod code without resident read statistics is a ValueError."""
        from .contig_methylation import MOD_CODES
        missing = sorted({str(c[1]) for c in candidates if c[1] not in self.readstats_mods})
        if missing:
            raise ValueError(f"no read statistics are resident for mod type(s) {', '.join(missing)} (resident: {', '.join(sorted(self.readstats_mods)) or 'none'})")
        return self.make_batch(candidates, slot_of=lambda mt: MOD_CODES.index(mt))

    def _fraction_groups(self, candidates, b: CandidateBatch, nb: int, limit: int):
        names = self._bin_names(b)
        width = nb + FRACTIONS_EXTRA

        def call(k, e, sub, rows, table):                                 # (the library lays the rows out itself: no row prefix goes in)
            _lib.check(self.lib.nm_motif_fractions_count(self.ctx, *self._batch_args(sub), nb, _ptr(table, C.c_uint64)))
        n_rows = [len(names[int(bid)]) for bid in b.bins]
        for j, contigs, table in _table_groups(b, names, n_rows, 2 * width * 8, limit, (2, width), np.uint64, call):
            yield candidates[j], contigs, table

    # ------------------------------------------------------------------ per-site read counts at motif sites (nm_motif_pileup_*)
    def _pileup_counts(self, b: CandidateBatch, select: int):
        return self._count_table(self.lib.nm_motif_pileup_count, self._batch_args(b), b, select, 4)

    def motif_pileup_counts(self, candidates):
        """Per (candidate, contig) the four occurrence counts (fwd site, fwd bare, rev site, rev bare) of every resident contig of the
        candidate's bin (nm_motif_pileup_count), read against the READ STATISTICS of the candidate's mod code as ``motif_fractions`` reads
        them: a site is an occurrence whose modified base carries a kept record, a bare occurrence one without.  Returns a list, per
        candidate, of (contig names, int64[n_contigs, 4]).  A mod code without resident read statistics is a ValueError."""
        b = self._readstats_batch(list(candidates))
        names, rows, _, table = self._pileup_counts(b, 3)
        return [(names[int(b.bins[k])], table[int(rows[k]):int(rows[k + 1])]) for k in range(len(b))]

    def motif_pileup(self, candidates, select=("site",), max_records=None):
        """Generator over the per-site read counts of ``candidates`` (sequence of (Motif, mod_type, bin)): for every occurrence under
        ``select`` (a selection of "site", "bare") the n_valid_cov and n_modified of the kept pileup record under its modified base
        (nm_motif_pileup_sites).  Yields ``SiteBatch`` objects in candidate order; their ``records`` (fields candidate, contig, pos, code,
        n_valid, n_mod; code = 4 for the '-' strand | 1 for a bare occurrence, which carries 0 / 0) concatenated are the occurrences in the
        order candidate, contig (``bin_contigs`` order), position, '+' before '-'; ``counts`` as ``motif_pileup_counts`` returns them.  No
        batch holds more than ``max_records`` records (default: ``SITE_BUDGET_BYTES`` of device records, 17 bytes each).  The
        concatenation does not depend on ``max_records``.  A mod code without resident read statistics is a ValueError."""
        b = self._readstats_batch(list(candidates))
        sel = pileup_select(select)
        limit = self._record_limit(max_records, PILEUP_RECORD_BYTES)
        return self._pileup_windows(b, sel, limit)

    def _pileup_windows(self, b: CandidateBatch, sel: int, limit: int):
        names, rows, totals, table = self._pileup_counts(b, sel)

        def group_args(k, e):
            sub = b.slice(k, e)
            return (self.ctx, *self._batch_args(sub), sel)
        windows = self._record_windows(self.lib.nm_motif_pileup_sites, group_args, totals, limit, PILEUP_DTYPE, "candidate", "batch", values=("n_valid", "n_mod"))
        yield from self._site_batches(windows, b, names, rows, table)

    # ------------------------------------------------------------------ read-fraction change between two pileups (nm_motif_shift_*)
    def _shift_slots(self, candidates: list, slot_b) -> np.ndarray:
        """uint8 read-statistics slots of sample B.  ``slot_b``: None (``SHIFT_SLOT_B`` + the mod code's index: the second pileup of
        ``upload_read_statistics(..., slot=)``), a base number (0: sample A against itself) or a callable from a mod type to a slot."""
        from .contig_methylation import MOD_CODES
        of = slot_b if callable(slot_b) else (lambda mt, base=SHIFT_SLOT_B if slot_b is None else int(slot_b): base + MOD_CODES.index(mt))
        return np.fromiter((of(c[1]) for c in candidates), dtype=np.uint8, count=len(candidates))

    def motif_shift_counts(self, candidates, bins=10, min_delta_permille=250, slot_b=None, max_bytes=None):
        """Generator over the JOIN of two pileups at the sites of ``candidates`` (sequence of (Motif, mod_type, bin)),
        nm_motif_shift_count: sample A is the read statistics of the candidate's mod code as ``motif_fractions`` reads them, sample B the
        slot ``slot_b`` names (``_shift_slots``).  Yields one item per candidate, in call order: (the candidate, contig names in
        ``bin_contigs`` order, uint64[n_contigs, 2, bins * bins + 12]) — per strand the joint histogram over the PAIRED sites (a kept
        record in both samples; cell = bin in A * bins + bin in B, a bin as in ``motif_fractions``), then the twelve sums ``SHIFT_SUMS``.
        A paired site goes up when n_mod_b / n_valid_b > n_mod_a / n_valid_a and is shifted when the two differ by at least
        ``min_delta_permille`` / 1000, both decided in exact integers.  ``bins``: 2..16.  Consecutive candidates share one library call
        while their table fits ``max_bytes`` (default ``SHIFT_BUDGET_BYTES``); what is yielded does not depend on it."""
        bins = int(bins)
        if not SHIFT_MIN_BINS <= bins <= SHIFT_MAX_BINS:
            raise ValueError(f"bins {bins} outside {SHIFT_MIN_BINS}..{SHIFT_MAX_BINS}")
        t = shift_permille(min_delta_permille)
        limit = _byte_limit(max_bytes, SHIFT_BUDGET_BYTES)
        candidates = list(candidates)
        return self._shift_groups(candidates, self._readstats_batch(candidates), self._shift_slots(candidates, slot_b), bins, t, limit)

    def _shift_groups(self, candidates, b: CandidateBatch, slots_b, nb: int, t: int, limit: int):
        names = self._bin_names(b)
        width = nb * nb + SHIFT_EXTRA

        def call(k, e, sub, rows, table):                                 # (the library lays the rows out itself: no row prefix goes in)
            _lib.check(self.lib.nm_motif_shift_count(self.ctx, *self._compare_args(sub, slots_b[k:e]), nb, t, _ptr(table, C.c_uint64)))
        n_rows = [len(names[int(bid)]) for bid in b.bins]
        for j, contigs, table in _table_groups(b, names, n_rows, 2 * width * 8, limit, (2, width), np.uint64, call):
            yield candidates[j], contigs, table

    def motif_shift(self, candidates, min_delta_permille=250, select=SHIFT_SELECT, max_records=None, slot_b=None):
        """Generator over the SHIFTED paired sites of ``candidates`` whose direction is in ``select`` (a selection of "up", "down"),
        nm_motif_shift_sites; samples, directions and the threshold as in ``motif_shift_counts``.  Yields ``SiteBatch`` objects in
        candidate order; their ``records`` (fields candidate, contig, pos, code, n_valid_a, n_mod_a, n_valid_b, n_mod_b; code = 4 for the
        '-' strand | 1 for a site that goes down) concatenated are the sites in the order candidate, contig (``bin_contigs`` order),
        position, '+' before '-'; ``counts``: per candidate (contig names, uint64[n_contigs, 2, 12]), the sums ``SHIFT_SUMS``.  No batch
        holds more than ``max_records`` records (default: ``SITE_BUDGET_BYTES`` of device records, 25 bytes each).  The concatenation
        does not depend on ``max_records``."""
        candidates = list(candidates)
        b = self._readstats_batch(candidates)
        slots_b = self._shift_slots(candidates, slot_b)
        sel, t = shift_select(select), shift_permille(min_delta_permille)
        limit = self._record_limit(max_records, SHIFT_RECORD_BYTES)
        return self._shift_windows(candidates, b, slots_b, sel, t, limit)

    def _shift_windows(self, candidates, b: CandidateBatch, slots_b, sel: int, t: int, limit: int):
        # the candidates' totals under `sel` are sums of the count table: n_shift_up / n_shift_down over contigs and strands
        nb = SHIFT_MIN_BINS
        names, rows = self._site_rows(b)
        sums = np.zeros((int(rows[-1]), 2, SHIFT_EXTRA), dtype=np.uint64)
        for j, (_, _, table) in enumerate(self._shift_groups(candidates, b, slots_b, nb, t, SHIFT_BUDGET_BYTES)):
            sums[int(rows[j]):int(rows[j + 1])] = table[:, :, nb * nb:]
        wanted = [SHIFT_SUMS.index(n) for n, d in (("n_shift_up", 1), ("n_shift_down", 2)) if sel & d]
        totals = np.array([int(sums[int(rows[j]):int(rows[j + 1])][:, :, wanted].sum()) for j in range(len(b))], dtype=np.uint64)

        def group_args(k, e):
            return (self.ctx, *self._compare_args(b.slice(k, e), slots_b[k:e]), t, sel)
        windows = self._record_windows(self.lib.nm_motif_shift_sites, group_args, totals, limit, SHIFT_DTYPE, "candidate", "batch",
                                       values=("n_valid_a", "n_mod_a", "n_valid_b", "n_mod_b"))
        yield from self._site_batches(windows, b, names, rows, sums)

    # ------------------------------------------------------------------ motif methylation by local GC content (nm_motif_gc_count)
    def motif_gc(self, candidates, half=31, max_bytes=None):
        """Generator over the sites of ``candidates`` (sequence of (Motif, mod_type, bin), or a CandidateBatch with slots from
        ``slot_of_mod``, as ``motif_site_counts`` takes them) counted apart by the GC content around them (nm_motif_gc_count).  A site
        is an occurrence of ``motif_site_counts`` with its state; its window is the W = 2 half + 1 positions centred on the modified
        base, g the number of G or C among them.  Yields one item per candidate, in call order: (contig names in ``bin_contigs`` order,
        int64[n_contigs, 2 (occurrence strand), 3 (mod, nomod, nocall), W + 2]) — the sites per g = 0..W and, last, the EDGE sites
        whose window leaves the contig or holds a letter that is not A, C, G or T.  Summed over the last axis it is the row of
        ``motif_site_counts``.  ``half``: 0..31.  Consecutive candidates share one library call while their tables fit ``max_bytes``
        (default ``GC_BUDGET_BYTES``); a group always holds at least one candidate.  What is yielded does not depend on ``max_bytes``."""
        half = int(half)
        if not 0 <= half <= GC_MAX_HALF:
            raise ValueError(f"half {half} outside 0..{GC_MAX_HALF}")
        limit = _byte_limit(max_bytes, GC_BUDGET_BYTES)
        return self._gc_groups(self._as_batch(candidates), half, limit)

    def _gc_groups(self, b: CandidateBatch, half: int, limit: int):
        names = self._bin_names(b)
        width = 2 * half + 3

        def call(k, e, sub, rows, table):
            _lib.check(self.lib.nm_motif_gc_count(self.ctx, *self._batch_args(sub), half, _ptr(rows, C.c_uint64), _ptr(table, C.c_int64)))
        n_rows = [len(names[int(bid)]) for bid in b.bins]
        for _, contigs, table in _table_groups(b, names, n_rows, 6 * width * 8, limit, (2, 3, width), np.int64, call):
            yield contigs, table

    # ------------------------------------------------------------------ motif methylation inside annotated regions (nm_regions_*, nm_motif_regions_*)
    def upload_regions(self, contig_ids, starts, ends, classes, class_names):
        """Intervals [starts[i], ends[i]) (0-based, half-open) of contig ``contig_ids[i]``, class ``classes[i]`` = index into
        ``class_names`` (1..8 names), rasterised into class planes on the resident assembly (nm_regions_create).  The intervals of a
        class are a union; a class may have none.  Replaces a previous set; ``close`` and every ``upload_assembly*`` drop it."""
        class_names = list(class_names)
        cid, st, en, cl = (np.ascontiguousarray(a, dtype=t) for a, t in ((contig_ids, np.uint32), (starts, np.uint64), (ends, np.uint64), (classes, np.uint8)))
        if not len(cid) == len(st) == len(en) == len(cl):
            raise ValueError("contig_ids, starts, ends and classes differ in length")
        h = C.c_void_p()
        _lib.check(self.lib.nm_regions_create(self.ctx, len(cid), _ptr(cid, C.c_uint32), _ptr(st, C.c_uint64), _ptr(en, C.c_uint64), _ptr(cl, C.c_uint8),
                                              len(class_names), C.byref(h)))
        self.clear_regions()
        self.regions, self.region_classes = h, class_names

    def clear_regions(self):
        """Drop the region set (nm_regions_destroy); nothing happens without one."""
        if getattr(self, "regions", None):
            self.lib.nm_regions_destroy(self.regions)
        self.regions, self.region_classes = C.c_void_p(), []

    def region_covered(self) -> np.ndarray:
        """int64[n_classes, n_contigs]: the positions of every contig inside every class (nm_regions_covered)."""
        out = np.zeros((max(len(self.region_classes), 1), max(len(self.contig_names), 1)), dtype=np.uint64)
        _lib.check(self.lib.nm_regions_covered(self.regions, _ptr(out, C.c_uint64)))
        return out[:len(self.region_classes), :len(self.contig_names)].astype(np.int64)

    def region_mask(self, contig, cls) -> np.ndarray:
        """bool[L]: the positions of ``contig`` (name or id) inside class ``cls`` (name or index), read back from the plane."""
        i = self.contig_index[contig] if isinstance(contig, str) else int(contig)
        c = self.region_classes.index(cls) if isinstance(cls, str) else int(cls)
        length = int(self.contig_lengths[i])
        words = np.zeros(max((length + 31) // 32, 1), dtype=np.uint32)
        _lib.check(self.lib.nm_regions_plane(self.regions, c, i, _ptr(words, C.c_uint32)))
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:length].astype(bool)

    def region_chunk_classes(self, contig) -> np.ndarray:
        """uint8 per chunk of 8192 positions of ``contig`` (name or id): the classes with a position in the chunk, as the count pass
        reads them (nm_regions_chunk_classes; the library says how many chunks there are)."""
        i = self.contig_index[contig] if isinstance(contig, str) else int(contig)
        n = C.c_uint32(0)
        _lib.check(self.lib.nm_regions_chunk_classes(self.regions, i, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _lib.check(self.lib.nm_regions_chunk_classes(self.regions, i, _ptr(out, C.c_uint8), n.value, C.byref(n)))
        return out[:n.value]

    def motif_regions_counts(self, candidates, max_bytes=None):
        """Generator over the sites of ``candidates`` (sequence of (Motif, mod_type, bin), or a CandidateBatch with slots from
        ``slot_of_mod``) counted per class of the uploaded region set (nm_motif_regions_count).  A site is an occurrence of
        ``motif_site_counts`` with its state; it is inside a class when its MODIFIED BASE lies in an interval of the class, and outside
        when it is inside none.  Yields one item per candidate, in call order: (contig names in ``bin_contigs`` order,
        int64[n_contigs, K + 1, 2 (occurrence strand), 3 (mod, nomod, nocall)]), K = the uploaded classes, cell K = outside.  A site
        inside several classes is counted in each.  Consecutive candidates share one library call while their tables fit ``max_bytes``
        (default ``REGIONS_BUDGET_BYTES``); what is yielded does not depend on it."""
        limit = _byte_limit(max_bytes, REGIONS_BUDGET_BYTES)
        return self._regions_groups(self._as_batch(candidates), limit)

    def _regions_groups(self, b: CandidateBatch, limit: int):
        names = self._bin_names(b)
        cells = len(self.region_classes) + 1

        def call(k, e, sub, rows, table):
            _lib.check(self.lib.nm_motif_regions_count(self.ctx, self.regions, *self._batch_args(sub), 7, 0, 1, _ptr(rows, C.c_uint64), None, _ptr(table, C.c_int64)))
        n_rows = [len(names[int(bid)]) for bid in b.bins]
        for _, contigs, table in _table_groups(b, names, n_rows, cells * 48, limit, (cells, 2, 3), np.int64, call):
            yield contigs, table

    def motif_regions_sites(self, candidates, states=SITE_STATES, classes=None, outside=False, max_records=None):
        """Generator over the sites of ``candidates`` inside the uploaded regions (nm_motif_regions_sites): the occurrences whose state
        is in ``states`` and that are inside at least one class of ``classes`` (names, default every class; "outside" among them, or
        ``outside`` True, adds the sites outside every uploaded class).  Yields ``SiteBatch`` objects in candidate order; their
        ``records`` (``REGION_DTYPE``: ``motif_sites``' fields and ``classes``, the mask of ALL uploaded classes the site is inside, 0 for
        an outside site) concatenated are the sites in ``motif_sites``' order; ``counts`` as ``motif_regions_counts`` yields them.  No
        batch holds more than ``max_records`` records; the concatenation does not depend on it."""
        b = self._as_batch(candidates)
        state_set = site_state_set(states)
        class_set, want = region_class_set(self.region_classes, classes)
        want = int(bool(want or outside))
        limit = self._record_limit(max_records, REGION_RECORD_BYTES)
        names, rows = self._site_rows(b)
        cells = len(self.region_classes) + 1
        table = np.zeros((max(int(rows[-1]), 1), cells, 2, 3), dtype=np.int64)
        totals = np.zeros(max(len(b), 1), dtype=np.uint64)
        _lib.check(self.lib.nm_motif_regions_count(self.ctx, self.regions, *self._batch_args(b), state_set, class_set, want, _ptr(rows, C.c_uint64),
                                                   _ptr(totals, C.c_uint64), _ptr(table, C.c_int64)))

        def group_args(k, e):
            return (self.ctx, self.regions, *self._batch_args(b.slice(k, e)), state_set, class_set, want)
        windows = self._record_windows(self.lib.nm_motif_regions_sites, group_args, totals[:len(b)], limit, REGION_DTYPE, "candidate", "batch",
                                       values=(("classes", np.uint8),))
        yield from self._site_batches(windows, b, names, rows, table[:int(rows[-1])])

    # ------------------------------------------------------------------ runs of same-state sites along contigs (nm_motif_runs_*)
    def motif_run_counts(self, candidates, max_run=16, nocall_breaks=False, max_bytes=None):
        """The RUNS of the sites of ``candidates`` (sequence of (Motif, mod_type, bin), or a CandidateBatch with slots from
        ``slot_of_mod``) counted per contig (nm_motif_runs_count).  A site is an occurrence of ``motif_site_counts`` with its state; on a
        contig the sites of both strands are taken by ascending position, the called ones form the sequence (nocall sites are
        transparent; with ``nocall_breaks`` they take part and end a run like any change of state), and a run is a maximal stretch of
        consecutive sequence elements of one state.  Returns a list, per candidate, of (contig names in ``bin_contigs`` order,
        int64[n_contigs, 3 (mod, nomod, nocall), 3 + R]), R = ``max_run`` (2..64): [s][0] runs, [s][1] sites (both strands; the nocall
        sites also when they do not take part), [s][2] the longest run, [s][3 + j] runs of exactly j + 1 sites, the last cell runs of R
        or more.  Consecutive candidates share one library call while their tables fit ``max_bytes`` (default ``RUNS_BUDGET_BYTES``);
        what is returned does not depend on it."""
        r = run_length_limit(max_run)
        limit = _byte_limit(max_bytes, RUNS_BUDGET_BYTES)
        b = self._as_batch(candidates)
        names = self._bin_names(b)
        nb = int(bool(nocall_breaks))

        def call(k, e, sub, rows, table):
            _lib.check(self.lib.nm_motif_runs_count(self.ctx, *self._batch_args(sub), r, nb, _ptr(rows, C.c_uint64), _ptr(table, C.c_int64)))
        n_rows = [len(names[int(bid)]) for bid in b.bins]
        return [(contigs, table) for _, contigs, table in _table_groups(b, names, n_rows, 3 * (3 + r) * 8, limit, (3, 3 + r), np.int64, call)]

    def motif_runs(self, candidates, states=("nomod",), min_run=3, nocall_breaks=False, max_records=None):
        """Generator over the runs of ``candidates`` (as ``motif_run_counts`` defines them) whose state is in ``states`` and that hold
        at least ``min_run`` sites (nm_motif_runs_sites).  Yields ``SiteBatch`` objects in candidate order; their ``records``
        (``RUN_DTYPE``: candidate, contig, pos = the position of the run's first site, code = state 0 mod / 1 nomod / 2 nocall, last =
        the position of its last site, n_sites) concatenated are the runs in the order candidate, contig (``bin_contigs`` order),
        ascending start; ``counts`` is None.  "nocall" in ``states`` needs ``nocall_breaks``.  No batch holds more than ``max_records``
        records (default: ``SITE_BUDGET_BYTES`` of device records, 17 bytes each); the concatenation does not depend on it."""
        b = self._as_batch(candidates)
        state_set = run_state_set(states, nocall_breaks)
        min_run = int(min_run)
        if min_run < 1:
            raise ValueError(f"min_run {min_run}: at least 1")
        nb = int(bool(nocall_breaks))
        limit = self._record_limit(max_records, RUN_RECORD_BYTES)
        return self._run_windows(b, state_set, min_run, nb, limit)

    def _run_windows(self, b: CandidateBatch, state_set: int, min_run: int, nb: int, limit: int):
        # the candidates' totals: the offsets of one call that asks for no record
        off = np.zeros(len(b) + 1, dtype=np.uint64)
        written = C.c_uint64(0)
        _lib.check(self.lib.nm_motif_runs_sites(self.ctx, *self._batch_args(b), state_set, min_run, nb, 0, 0, None, None, None, None, None, _ptr(off, C.c_uint64),
                                                C.byref(written)))
        totals = np.diff(off)

        def group_args(k, e):
            return (self.ctx, *self._batch_args(b.slice(k, e)), state_set, min_run, nb)
        for k, e, first, held, rec in self._record_windows(self.lib.nm_motif_runs_sites, group_args, totals, limit, RUN_DTYPE, "candidate", "batch",
                                                           values=("last", "n_sites")):
            yield SiteBatch(first_candidate=k, n_candidates=e - k, first_record=first, batch_records=held, records=rec, counts=None)

    # ------------------------------------------------------------------ shared sites of a motif and its partners (nm_motif_overlap_count)
    def motif_overlap(self, candidates, partners, max_bytes=None):
        """Generator over the sites ``candidates`` (sequence of (Motif, mod_type, bin), or a CandidateBatch with slots from
        ``slot_of_mod``, as ``motif_site_counts`` takes them) share with their partners (nm_motif_overlap_count).  ``partners[k]``: a
        list of Motif, read in candidate k's bin and mod slot; at most ``OVERLAP_MAX_PARTNERS``.  A site is an occurrence of
        ``motif_site_counts`` with its state; two motifs share a site when both have that (contig, position, strand).  Yields one
        item per candidate, in call order: (contig names in ``bin_contigs`` order, int64[P_k + 2, n_contigs, 2 (occurrence strand),
        3 (mod, nomod, nocall)]) — block 0 the candidate's own sites (its ``motif_site_counts`` rows), block 1 + q the sites it
        shares with its q-th partner, the last block the REST: its sites no partner has (without partners: block 0 again).
        Consecutive candidates share one library call while their tables fit ``max_bytes`` (default ``OVERLAP_BUDGET_BYTES``); a
        group always holds at least one candidate.  What is yielded does not depend on ``max_bytes``."""
        limit = _byte_limit(max_bytes, OVERLAP_BUDGET_BYTES)
        b = self._as_batch(candidates)
        partners = [list(p) for p in partners]
        if len(partners) != len(b):
            raise ValueError(f"{len(b)} candidates but {len(partners)} partner lists")
        worst = max((len(p) for p in partners), default=0)
        if worst > OVERLAP_MAX_PARTNERS:
            raise ValueError(f"a candidate has {worst} partners, above OVERLAP_MAX_PARTNERS = {OVERLAP_MAX_PARTNERS}")
        return self._overlap_groups(b, partners, limit)

    def _overlap_groups(self, b: CandidateBatch, partners: list, limit: int):
        names = self._bin_names(b)
        blocks = [len(p) + 2 for p in partners]
        part0 = np.zeros(len(b) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in partners], out=part0[1:])
        flat = [(m, 0, 0) for p in partners for m in p]
        pb = self.make_batch(flat, slot_of=lambda mt: 0) if flat else None

        def call(k, e, sub, rows, table):
            q0, q1 = int(part0[k]), int(part0[e])
            off = (part0[k:e + 1] - q0).astype(np.uint32)
            if q1 > q0:
                ps = pb.slice(q0, q1)
                pargs = (_ptr(ps.lens, C.c_uint8), _ptr(ps.modpos, C.c_uint8), _ptr(ps.offsets, C.c_uint32), _ptr(ps.masks, C.c_uint8))
            else:
                pargs = (None, None, None, None)
            _lib.check(self.lib.nm_motif_overlap_count(self.ctx, *self._batch_args(sub), _ptr(off, C.c_uint32), *pargs, _ptr(rows, C.c_uint64),
                                                       _ptr(table, C.c_int64)))
        n_rows = [blocks[j] * len(names[int(bid)]) for j, bid in enumerate(b.bins)]
        for j, contigs, table in _table_groups(b, names, n_rows, OVERLAP_ROW_BYTES, limit, (2, 3), np.int64, call):
            yield contigs, table.reshape(blocks[j], len(contigs), 2, 3)

    # ------------------------------------------------------------------ coverage of a set of motifs (nm_motif_coverage_*)
    def _coverage_args(self, sets):
        """sets = [(bin name or id, mod type or slot number, [Motif, ...]), ...] -> (the leading arguments of nm_motif_coverage_*,
        the arrays they point into (set_bin, set_slot, set_cand_offset, the candidate arrays), the number of motifs per set)."""
        sets = [(b, mt, list(motifs)) for b, mt, motifs in sets]
        n_sets = len(sets)
        bi, so = self.bin_index, self.slot_of_mod
        set_bin = np.fromiter((bi[s[0]] if isinstance(s[0], str) else int(s[0]) for s in sets), dtype=np.uint32, count=n_sets)
        set_slot = np.fromiter((so[s[1]] if isinstance(s[1], str) else int(s[1]) for s in sets), dtype=np.uint8, count=n_sets)
        n_motifs = [len(s[2]) for s in sets]
        cand_off = np.zeros(n_sets + 1, dtype=np.uint32)
        np.cumsum(np.asarray(n_motifs, dtype=np.uint32), out=cand_off[1:])
        flat = [(m, 0, 0) for s in sets for m in s[2]]
        if flat:
            b = self.make_batch(flat, slot_of=lambda mt: 0)
            lens, modpos, moff, masks = b.lens, b.modpos, b.offsets, b.masks
        else:
            lens, modpos, masks = (np.zeros(1, dtype=np.uint8) for _ in range(3))
            moff = np.zeros(1, dtype=np.uint32)
        keep = (set_bin, set_slot, cand_off, lens, modpos, moff, masks)
        args = (self.ctx, n_sets, _ptr(set_bin, C.c_uint32), _ptr(set_slot, C.c_uint8), _ptr(cand_off, C.c_uint32), _ptr(lens, C.c_uint8),
                _ptr(modpos, C.c_uint8), _ptr(moff, C.c_uint32), _ptr(masks, C.c_uint8))
        return args, keep, n_motifs

    def _coverage_counts(self, sets):
        args, keep, n_motifs = self._coverage_args(sets)
        set_bin = keep[0]
        n_bins = len(self.bin_index)
        # (a bin the engine does not hold is the library's to refuse: it gets no rows here)
        names = {int(b): (self.bin_contigs(int(b)) if int(b) < n_bins else []) for b in np.unique(set_bin).tolist()}
        per_set = [len(names[int(b)]) for b in set_bin]
        set_rows = np.zeros(len(per_set) + 1, dtype=np.uint64)
        np.cumsum(np.asarray(per_set, dtype=np.uint64), out=set_rows[1:])
        cand_rows = np.zeros(sum(n_motifs) + 1, dtype=np.uint64)
        np.cumsum(np.repeat(np.asarray(per_set, dtype=np.uint64), np.asarray(n_motifs, dtype=np.int64)), out=cand_rows[1:])
        set_table = np.zeros((max(int(set_rows[-1]), 1), 10), dtype=np.int64)
        cand_table = np.zeros((max(int(cand_rows[-1]), 1), 4), dtype=np.int64)
        totals = np.zeros(max(len(per_set), 1), dtype=np.uint64)
        _lib.check(self.lib.nm_motif_coverage_count(*args, _ptr(set_rows, C.c_uint64), _ptr(cand_rows, C.c_uint64), _ptr(totals, C.c_uint64),
                                                    _ptr(set_table, C.c_int64), _ptr(cand_table, C.c_int64)))
        return names, set_bin, n_motifs, set_rows, cand_rows, totals[:len(per_set)].astype(np.int64), set_table, cand_table

    def motif_coverage(self, sets):
        """How much of the methylation of a (bin, mod type) a SET of motifs explains (nm_motif_coverage_count; the reference only logs
        "% of sequences remaining" inside find_best_candidates, find_motifs_bin.py:801-823).  ``sets`` = [(bin, mod_type, [Motif, ...]),
        ...]; a set may be empty.  Returns per set (contig names in ``bin_contigs`` order, int64[n_contigs, 10], [int64[n_contigs, 4]
        per motif]): the set table holds per strand (forward, then reverse) mod_total, mod_explained, nomod_total, nomod_covered,
        nocall_covered; a motif's table (fwd mod, fwd nomod, rev mod, rev nomod) of the positions ONLY this motif of the set covers."""
        names, set_bin, n_motifs, set_rows, cand_rows, _, set_table, cand_table = self._coverage_counts(sets)
        out, k = [], 0
        for s in range(len(n_motifs)):
            per = [cand_table[int(cand_rows[j]):int(cand_rows[j + 1])] for j in range(k, k + n_motifs[s])]
            out.append((names[int(set_bin[s])], set_table[int(set_rows[s]):int(set_rows[s + 1])], per))
            k += n_motifs[s]
        return out

    def unexplained_sites(self, sets, max_records=None):
        """Generator over the methylated positions NO motif of their set covers (nm_motif_coverage_sites).  Yields structured arrays
        (fields set, contig, pos, code; code = 4 on the '-' strand, else 0) whose concatenation is in the order set, contig
        (``bin_contigs`` order), position, '+' before '-'.  No batch holds more than ``max_records`` records (default
        ``SITE_BUDGET_BYTES`` of device records); the concatenation does not depend on ``max_records``."""
        limit = self._record_limit(max_records)
        sets = [(b, mt, list(motifs)) for b, mt, motifs in sets]
        totals = self._coverage_counts(sets)[5]
        windows = self._record_windows(self.lib.nm_motif_coverage_sites, lambda k, e: self._coverage_args(sets[k:e])[0], totals, limit,
                                       UNEXPLAINED_DTYPE, "set", "call")
        for _, _, _, _, rec in windows:
            yield rec

    def set_score_lanes(self, lanes: int):
        """2: consecutive ``score_into_device`` calls alternate between two streams, so that independent batches
        overlap on the device (include/nmscan.h: nm_set_score_lanes); 1: strict order (default)."""
        _lib.check(self.lib.nm_set_score_lanes(self.ctx, int(lanes)))

    def sync(self):
        """All scoring work queued on this engine has finished (both lanes)."""
        _lib.check(self.lib.nm_sync(self.ctx))

    def score_into_device(self, batch: CandidateBatch, device_ptr: int):
        """Asynchronous variant: counts land in device memory (e.g. a torch int64 tensor) on the engine stream."""
        _lib.check(self.lib.nm_score_batch_device(self.ctx, *self._batch_args(batch), C.c_void_p(device_ptr)))

    def hit_positions(self, contig, mod_type, motif: Motif, which: int) -> np.ndarray:
        """Ascending contig-local positions; which = 0 meth fwd, 1 nonmeth fwd, 2 meth rev, 3 nonmeth rev
        (motif_model_contig(save_motif_positions=True), find_motifs_bin.py:1322-1329)."""
        cid = self.contig_index[contig] if isinstance(contig, str) else int(contig)
        b = self.make_batch([(motif, mod_type, 0)])
        n = C.c_uint64(0)
        cap = 1 << 16
        while True:
            out = np.empty(cap, dtype=np.int64)
            _lib.check(self.lib.nm_hit_positions(self.ctx, cid, self.slot_of_mod[mod_type], int(b.lens[0]), int(b.modpos[0]),
                                                 _ptr(b.masks, C.c_uint8), which, _ptr(out, C.c_int64), cap, C.byref(n)))
            if n.value <= cap:
                return out[:n.value].copy()
            cap = int(n.value)

    # ------------------------------------------------------------------ multi-GPU exchange (nm_comm_*, RCCL)
    def comm_unique_id(self) -> bytes:
        """The 128-byte id rank 0 creates; the host carries it to the other ranks (nm_comm_unique_id)."""
        buf = (C.c_uint8 * 128)()
        _lib.check(self.lib.nm_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        """Collective: join the RCCL communicator of the run (nm_comm_init)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _lib.check(self.lib.nm_comm_init(self.ctx, int(rank), int(world), buf))
        self.comm_world = int(world)

    def allreduce_counts_device(self, device_ptr: int, n: int, slot: int = 0):
        """Start the in-place sum of a device int64[n] table over all ranks on the communication stream
        (nm_allreduce_counts_async); ``comm_wait(slot)`` before the engine stream touches that buffer again."""
        _lib.check(self.lib.nm_allreduce_counts_async(self.ctx, C.c_void_p(device_ptr), int(n), int(slot)))

    def comm_wait(self, slot: int = 0):
        _lib.check(self.lib.nm_comm_wait(self.ctx, int(slot)))

    def comm_sync(self):
        _lib.check(self.lib.nm_comm_sync(self.ctx))

    def comm_info(self) -> dict:
        """What the RCCL communicator reports about itself (nm_comm_info): world, rank, device, RCCL version code;
        world 0 = no communicator on this engine."""
        info = (C.c_int32 * 4)()
        _lib.check(self.lib.nm_comm_info(self.ctx, info))
        return {"world": int(info[0]), "rank": int(info[1]), "device": int(info[2]), "rccl_version": int(info[3])}

    def allreduce_host(self, counts: np.ndarray) -> np.ndarray:
        """Sum an integer numpy array over all ranks (nm_allreduce_counts_host); returns the same dtype and shape."""
        a = np.ascontiguousarray(counts, dtype=np.int64).copy()
        if a.size:
            _lib.check(self.lib.nm_allreduce_counts_host(self.ctx, _ptr(a, C.c_int64), a.size))
        return a.astype(counts.dtype, copy=False).reshape(counts.shape)

    # ------------------------------------------------------------------ measurement
    def stats(self) -> dict:
        w = (C.c_uint64 * 8)()
        _lib.check(self.lib.nm_stats(self.ctx, w))
        keys = ["total_bp", "padded_bp", "seq_plane_bytes", "state_plane_bytes", "launches", "last_workgroups",
                "last_compact", "last_general"]
        parked = C.c_int(0)
        _lib.check(self.lib.nm_last_score_parked(self.ctx, C.byref(parked)))
        return {**dict(zip(keys, [int(x) for x in w])), "last_parked": int(parked.value)}

    def last_score_enqueue(self) -> int:
        """How the last scoring call was enqueued (include/nmscan.h: NM_ENQ_*): bit 0 the timing pair bound to the clear and the scoring
        dispatch, bit 2 the scoring stream (found idle) waits for the programs instead of the host; 0: the enqueue of every call that is
        not ``score_into_device``, and of every call under NM_SCORE_ENQUEUE=0."""
        flags = C.c_uint32(0)
        _lib.check(self.lib.nm_last_score_enqueue(self.ctx, C.byref(flags)))
        return int(flags.value)

    def timing_reset(self, enable=True):
        """True / 1: collect the scoring launches; 2: every device phase of the library (pre-filters, window gathers, window
        batches, background counts); False / 0: stop."""
        _lib.check(self.lib.nm_timing_reset(self.ctx, int(enable)))

    def timing_total(self):
        """(sum of scoring-kernel durations in ms, number of launches) since ``timing_reset(True)``."""
        ms, n = C.c_double(0), C.c_uint64(0)
        _lib.check(self.lib.nm_timing_total_ms(self.ctx, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def timing_intervals(self, epoch=None) -> np.ndarray:
        """float64[n, 2]: begin / end of every phase since ``timing_reset`` in ms after the first phase of ``epoch`` (another engine on
        this device; default: this one) — nm_timing_intervals."""
        ref = self if epoch is None else epoch
        n = C.c_uint64(0)
        _lib.check(self.lib.nm_timing_intervals(self.ctx, ref.ctx, 0, None, None, C.byref(n)))
        out = np.zeros((2, max(int(n.value), 1)), dtype=np.float64)
        if n.value:
            _lib.check(self.lib.nm_timing_intervals(self.ctx, ref.ctx, int(n.value), _ptr(out[0], C.c_double), _ptr(out[1], C.c_double), C.byref(n)))
        return np.ascontiguousarray(out[:, :int(n.value)].T)

    def last_kernel_ms(self) -> float:
        ms = C.c_float(0)
        _lib.check(self.lib.nm_last_kernel_ms(self.ctx, C.byref(ms)))
        return float(ms.value)
