"""The enqueue of a device-output scoring call (csrc/nmscan.hip: score_enqueue_form, score_prepare, score_collect): the count table
cleared by a dispatch of the library's own, the timing pair bound to the two dispatches instead of recorded around them, and the
staging pair released by the second event of the pair when launches are collected.  Every case is compared by equality with the same
call under NM_SCORE_ENQUEUE=0 (the enqueue as it was, same process) and with the brute force of tests/test_gpu_score_park.py; which
enqueue a call took is read from the engine (``last_score_enqueue``), never inferred.

16.5 kbp: three bins with one contig each — 92 bp, 8 192 bp (exactly one chunk) and 8 213 bp (one chunk and a tail) — and a fourth bin
that holds no contig; both mod types; candidate tables of 1, 10, 28, 29 and 64 motifs (light, parked heavy, unparked heavy,
literal-only)."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

from test_gpu_score_park import BASES, ParkData, make_shapes
from test_gpu_score_tail_pack import CANONICAL, COMPLEMENT, _with_env

pytestmark = pytest.mark.gpu

BOUND = 1                                                     # include/nmscan.h: NM_ENQ_BOUND_EVENTS (bits 1 and 2 are reserved, never reported)
LENGTHS = [[92], [8192], [8213], []]
HERE = os.path.dirname(os.path.abspath(__file__))


def stage_ring():
    text = open(os.path.join(HERE, "..", "nanomotif_amd", "csrc", "nmscan_internal.h")).read()
    return int(re.search(r"#define NM_STAGE_RING (\d+)", text).group(1))


class EnqueueData(ParkData):
    """ParkData's brute force (``fast``, ``groups``) over the contigs above; bin_3 is numbered and empty."""

    def __init__(self, seed=17):
        rng = np.random.default_rng(seed)
        self.names, self.bins, self.seqs = [], [], []
        for b, contigs in enumerate(LENGTHS):
            for k, n in enumerate(contigs):
                self.names.append("contig_%d_%d" % (b, k))
                self.bins.append("bin_%d" % b)
                self.seqs.append("".join(rng.choice(list(BASES), size=n)))
        self.bin_names = ["bin_%d" % b for b in range(len(LENGTHS))]
        self.calls, self.columns, self.state, self._brute, self._fast, self._member = {}, {}, {}, {}, {}, {}
        self.codes = [np.frombuffer(s.encode(), dtype=np.uint8) for s in self.seqs]
        for mt, base in CANONICAL.items():
            cid, pos, strand, frac = [], [], [], []
            for i, a in enumerate(self.codes):
                for st, letter in (("+", base), ("-", COMPLEMENT[base])):
                    p = np.flatnonzero(a == ord(letter))
                    f = rng.choice([0.95, 0.05, 0.5], size=len(p), p=[0.45, 0.45, 0.1])
                    cid.append(np.full(len(p), i, np.uint32)); pos.append(p.astype(np.uint32)); strand.append(np.full(len(p), ord(st), np.uint8)); frac.append(f)
                    state = np.zeros(len(a), np.uint8)
                    state[p[f > 0.5]] = 1
                    state[p[f < 0.5]] = 2
                    self.state[(mt, i, st)] = state
            self.columns[mt] = tuple(np.concatenate(x) for x in (cid, pos, strand, frac))


@pytest.fixture(scope="module")
def data():
    return EnqueueData()


@pytest.fixture(scope="module")
def shapes():
    return make_shapes(57, seed=23)


@pytest.fixture(scope="module")
def engine(data):
    assert "NM_SCORE_ENQUEUE" not in os.environ
    eng = data.engine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def tables(data, shapes):
    """name -> (candidates, brute-force counts, parked or None where the kernel is not a class kernel)."""
    literals = shapes[0::3]
    out = {}
    for name, sizes, pool, parked in (
            ("1", {(1, "a"): 1}, shapes, None),
            ("10", {(0, "a"): 2, (0, "m"): 1, (1, "a"): 1, (1, "m"): 2, (2, "a"): 1, (2, "m"): 1, (3, "a"): 1, (3, "m"): 1}, shapes, None),
            ("28", {(2, "a"): 28}, shapes, 1),
            ("29", {(2, "m"): 29}, shapes, 0),
            ("64", {(0, "a"): 16, (1, "m"): 16, (2, "a"): 16, (3, "m"): 16}, literals, None)):
        cands, want = data.groups(sizes, pool)
        assert len(cands) == int(name)
        out[name] = (cands, want, parked)
    assert all(out[k][1].sum() > 0 for k in ("10", "28", "29", "64"))
    assert out["64"][1][48:].sum() == 0                                   # (bin_3 holds nothing)
    return out


def device_run(engine, cands, table=None, fill=-1):
    """One asynchronous call into a fresh (or the given) device table; returns the table, not synchronised."""
    import torch
    if table is None:
        table = torch.full((len(cands), 2), fill, dtype=torch.int64, device="cuda:0")
    engine.score_into_device(engine.make_batch(cands), table.data_ptr())
    return table


def test_every_table_both_enqueues_and_the_report(engine, tables):
    for name, (cands, want, parked) in tables.items():
        for what, env in (("default", None), ("NM_SCORE_ENQUEUE=0", "0"), ("NM_SCORE_ENQUEUE=1", "1"), ("NM_SCORE_ENQUEUE=4", "4")):
            def run():
                engine.sync()
                t = device_run(engine, cands)
                flags = engine.last_score_enqueue()
                engine.sync()
                return t.cpu().numpy(), flags
            got, flags = run() if env is None else _with_env("NM_SCORE_ENQUEUE", env, run)
            assert flags == {None: BOUND, "0": 0, "1": BOUND, "4": 0}[env], (name, what, flags)
            assert got.tolist() == want.tolist(), (name, what)
            if parked is not None:
                assert engine.stats()["last_parked"] == parked, (name, what)
            assert engine.last_kernel_ms() > 0


def test_one_table_reused_by_consecutive_calls(engine, tables):
    """Calls with different candidate tables into ONE device table, no synchronisation between them: every clear stays in front of
    its kernel and behind the kernel before it, and clears the rows of its own call only."""
    import torch
    order = ["64", "1", "29", "10", "28", "64", "1", "28"]
    for what, env in (("default", None), ("NM_SCORE_ENQUEUE=0", "0")):
        def run():
            table = torch.full((64, 2), -7, dtype=torch.int64, device="cuda:0")
            model = np.full((64, 2), -7, dtype=np.int64)
            for k in order:
                device_run(engine, tables[k][0], table)
                model[:len(tables[k][0])] = tables[k][1]
            engine.sync()
            assert table.cpu().numpy().tolist() == model.tolist(), what
            for k in order:                                                # and one at a time
                device_run(engine, tables[k][0], table)
                model[:len(tables[k][0])] = tables[k][1]
                engine.sync()
                assert table.cpu().numpy().tolist() == model.tolist(), (what, k)
        run() if env is None else _with_env("NM_SCORE_ENQUEUE", env, run)


@pytest.mark.parametrize("collect", [False, True], ids=["busy recorded", "pool event as marker"])
def test_twice_the_ring_and_one_distinct_tables(engine, data, shapes, collect):
    """2 x NM_STAGE_RING + 1 calls in a row, every one with its own candidates: a staging pair handed out before the kernel that reads
    it has finished shows as another call's rows."""
    n_calls = 2 * stage_ring() + 1
    batches = [data.groups({(k % 3, "a"): 1 + k, ((k + 1) % 3, "m"): n_calls - k}, shapes) for k in range(n_calls)]
    assert len({tuple(w.ravel().tolist()) for _, w in batches}) == n_calls
    for what, env in (("default", None), ("NM_SCORE_ENQUEUE=0", "0")):
        def run():
            engine.timing_reset(collect)
            out = [device_run(engine, c) for c, _ in batches]
            flags = engine.last_score_enqueue()
            engine.sync()
            if collect:
                assert engine.timing_total()[1] == n_calls
            engine.timing_reset(False)
            return [t.cpu().numpy() for t in out], flags
        got, flags = run() if env is None else _with_env("NM_SCORE_ENQUEUE", env, run)
        assert (flags & BOUND) == (0 if env else BOUND), what
        for k, (g, (_, want)) in enumerate(zip(got, batches)):
            assert g.tolist() == want.tolist(), (what, k)


def test_timing_on_off_on_reuses_the_event_pool(engine, data, shapes, tables):
    """nm_timing_reset(1), calls, nm_timing_reset(0), calls, nm_timing_reset(1), calls: the pool's events are handed out again from
    the start, while staging pairs of the first phase remember some of them as their release marker."""
    ring = stage_ring()
    phases = [(True, ring - 3), (False, ring - 2), (True, 2 * ring + 1)]
    batches = [data.groups({(1 + k % 2, "m"): 3 + k, (2 - k % 2, "a"): 30 - k}, shapes) for k in range(sum(n for _, n in phases))]
    for what, env in (("default", None), ("NM_SCORE_ENQUEUE=0", "0")):
        def run():
            engine.sync()
            out, at = [], 0
            for collect, n in phases:
                engine.timing_reset(collect)                              # (waits for the scoring streams)
                t0 = time.perf_counter()
                out += [device_run(engine, c) for c, _ in batches[at:at + n]]
                at += n
                total_ms, launches = engine.timing_total()                # (waits for the phase's last event)
                engine.sync()
                wall_ms = (time.perf_counter() - t0) * 1e3
                assert launches == (n if collect else 0), (what, collect, launches)
                if collect:
                    spans = engine.timing_intervals()
                    per_launch = spans[:, 1] - spans[:, 0]
                    print(what, "launches", launches, "kernel ms", round(total_ms, 4), "wall ms", round(wall_ms, 4), "shortest", float(per_launch.min()))
                    assert len(per_launch) == n and (per_launch > 0).all(), (what, per_launch.tolist())
                    assert 0 < total_ms <= wall_ms, (what, total_ms, wall_ms)
            engine.timing_reset(False)
            return [t.cpu().numpy() for t in out]
        got = run() if env is None else _with_env("NM_SCORE_ENQUEUE", env, run)
        for k, (g, (_, want)) in enumerate(zip(got, batches)):
            assert g.tolist() == want.tolist(), (what, k)


@pytest.mark.parametrize("lanes", [1, 2])
def test_lanes(engine, tables, lanes):
    names = ["64", "1", "29", "10", "28"] * 2
    for what, env in (("default", None), ("NM_SCORE_ENQUEUE=0", "0")):
        def run():
            engine.set_score_lanes(lanes)
            try:
                out = [device_run(engine, tables[k][0]) for k in names]
                flags = engine.last_score_enqueue()
                engine.sync()
            finally:
                engine.set_score_lanes(1)
            return [t.cpu().numpy() for t in out], flags
        got, flags = run() if env is None else _with_env("NM_SCORE_ENQUEUE", env, run)
        assert (flags & BOUND) == (0 if env else BOUND), what
        for k, g in zip(names, got):
            assert g.tolist() == tables[k][1].tolist(), (what, lanes, k)


def test_two_lanes_that_write_one_table(engine, tables):
    """The two-lane case of tests/test_gpu_lanes.py in which both lanes write one table: the lane that comes second waits for the
    other's release marker, whichever event that is."""
    import torch
    names = ["64", "1", "29", "10", "28"]
    padded = {k: (tables[k][0] + [tables[k][0][0]] * (64 - len(tables[k][0])),
                  np.concatenate([tables[k][1], np.repeat(tables[k][1][:1], 64 - len(tables[k][0]), axis=0)])) for k in names}
    for collect in (False, True):
        for what, env in (("default", None), ("NM_SCORE_ENQUEUE=0", "0")):
            def run():
                table = torch.zeros((64, 2), dtype=torch.int64, device="cuda:0")
                engine.timing_reset(collect)
                engine.set_score_lanes(2)
                try:
                    for rep in range(4):
                        for k in names:
                            device_run(engine, padded[k][0], table)
                            if (rep, k) in ((1, "29"), (3, "64")):
                                engine.sync()
                                assert table.cpu().numpy().tolist() == padded[k][1].tolist(), (what, collect, rep, k)
                                assert engine.score(tables["10"][0]).tolist() == tables["10"][1].tolist()      # flips the lane parity
                    engine.sync()
                    assert table.cpu().numpy().tolist() == padded[names[-1]][1].tolist(), (what, collect)
                finally:
                    engine.set_score_lanes(1)
                    engine.timing_reset(False)
            run() if env is None else _with_env("NM_SCORE_ENQUEUE", env, run)


def test_a_call_on_an_idle_stream_and_one_behind_a_long_batch(engine, data, shapes, tables):
    """A first call on an idle stream, and a call issued while a long batch is in flight (40 000 candidates of one group on an 8 kbp
    bin: one wave walks them all, milliseconds).  Both take the one short enqueue there is: the host waits for the compiled programs
    in either case (letting an idle stream wait instead was measured and taken out, profiles/r28/step_gap.md)."""
    import torch
    cands, want = data.groups({(2, "a"): 50}, shapes)
    long_cands = cands * 800
    long_batch = engine.make_batch(long_cands)
    long_table = torch.full((len(long_cands), 2), -1, dtype=torch.int64, device="cuda:0")
    small = engine.make_batch(tables["10"][0])
    small_table = torch.full((10, 2), -1, dtype=torch.int64, device="cuda:0")
    engine.sync()
    engine.score_into_device(long_batch, long_table.data_ptr())
    first = engine.last_score_enqueue()
    engine.score_into_device(small, small_table.data_ptr())
    second = engine.last_score_enqueue()
    engine.sync()
    assert first == BOUND and second == BOUND, (first, second)
    assert small_table.cpu().numpy().tolist() == tables["10"][1].tolist()
    assert long_table.cpu().numpy().tolist() == np.tile(want, (800, 1)).tolist()


def test_other_entry_points_keep_their_enqueue_and_a_refused_call_between(engine, tables):
    from nanomotif_amd._lib import NmScanError, check
    cands, want, _ = tables["28"]
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))

    def device_ok():
        t = device_run(engine, cands)
        flags = engine.last_score_enqueue()
        engine.sync()
        assert flags & BOUND and t.cpu().numpy().tolist() == want.tolist()
    device_ok()
    assert engine.score(cands).tolist() == want.tolist() and engine.last_score_enqueue() == 0          # host counts
    device_ok()
    check(engine.lib.nm_score_batch_begin(engine.ctx, *engine._batch_args(engine.make_batch(cands))))      # begin / end
    assert engine.last_score_enqueue() == 0
    got = np.full((len(cands), 2), -1, dtype=np.int64)
    check(engine.lib.nm_score_batch_end(engine.ctx, p(got, C.c_int64)))
    assert got.tolist() == want.tolist()
    device_ok()
    bad = engine.make_batch(cands)
    bad.slots[:] = 5                                                      # a mod slot that holds no pileup
    import torch
    table = torch.full((len(cands), 2), -1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(NmScanError):
        engine.score_into_device(bad, table.data_ptr())
    engine.sync()
    assert (table.cpu().numpy() == -1).all()                              # (refused before anything was enqueued)
    device_ok()


def test_spec_batches_of_a_search_before_and_after():
    """The native search's speculative child batches (motifs written on the device, their own stream) and its begin / end batches keep
    their enqueue; device-output calls on the same engine before and after a search take the short one and count what the host-count
    call counts."""
    import torch
    from nanomotif_amd import e2e_synth, synth, synth_device
    from nanomotif_amd.engine import ScanEngine
    from nanomotif_amd.motif import Motif
    dev = torch.device("cuda:0")
    mg = synth.make_metagenome(synth.SynthSpec(n_contigs=6, total_bp=900_000, n_bins=2, mod_types=("a", "m"), seed=41, min_contig_bp=50_000))
    cands = [(Motif(s, mp), mt, b) for b in sorted(set(mg.bin_names)) for mt in ("a", "m") for s, mp in
             ((("GATC", 1), ("A", 0), ("G[AG].GAAG[CT]", 5), ("CCAGG", 2)) if mt == "a" else (("GATC", 3), ("C", 0), ("C[CT]GG", 0), ("CCAGG", 1)))]
    eng = ScanEngine(0)

    def device_calls_equal_the_host_call():
        want = eng.score(cands)
        assert want.sum() > 0 and eng.last_score_enqueue() == 0
        for what, env in (("default", None), ("NM_SCORE_ENQUEUE=0", "0")):
            def run():
                tab = device_run(eng, cands)
                flags = eng.last_score_enqueue()
                eng.sync()
                return tab.cpu().numpy(), flags
            got, flags = run() if env is None else _with_env("NM_SCORE_ENQUEUE", env, run)
            assert (flags & BOUND) == (0 if env else BOUND) and got.tolist() == want.tolist(), what
    try:
        synth_device.load_engine_from_device(eng, mg, dev)
        device_calls_equal_the_host_call()
        rows, t = e2e_synth.run(mg, eng, dev)                             # (uploads the assembly again, filters, searches)
        assert t["speculation_hits"] > 0 and len(rows) > 0                # spec batches ran
        assert eng.last_score_enqueue() == 0
        device_calls_equal_the_host_call()
    finally:
        eng.close()
