"""nm_plan_windows (csrc/nmwindows.hip: bg_draw_kernel, win_gather_all_kernel, rank_build_kernel and the select of bg_counts_kernel)
against the plain-Python brute force of tests/window_plan_geometry.py on its geometry input, by equality only.  Every run reads the
NM_PLAN_TIMING line to prove which path drew the samples: `device draws` for the plan as it is, `host draws` under NM_HOST_DRAWS=1 and
for a plan with a pool call too long for the device.  tests/test_window_plan_host.py shows on the CPU that every border is in the input."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import window_plan_geometry as wg
from nanomotif_amd import search as ps
from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL

pytestmark = pytest.mark.gpu

_runs = {}                # (plan id, host draws) -> _Run, made by the first test that needs it


class _PlanSpy:
    """the engine's library with nm_plan_windows recorded: plan_all returns counts / n_bg, the test wants n_bg itself"""

    def __init__(self, lib):
        self._lib, self.n_bg = lib, None

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def nm_plan_windows(self, *args):
        rc = self._lib.nm_plan_windows(*args)
        self.n_bg = np.ctypeslib.as_array(args[15], shape=(int(args[1]),)).copy()          # task_n_bg (include/nmscan.h)
        return rc


class _Run:
    pass


def _upload(plan):
    from nanomotif_amd.engine import ScanEngine
    eng = ScanEngine(0)
    names = list(plan.seqs)
    eng.upload_assembly(names, [plan.seqs[n] for n in names], [plan.bin_of[n] for n in names])
    assert eng.other_letters() == 0
    for mt, rows in plan.rows.items():
        if not rows:
            continue
        cid, pos, strand, frac = [], [], [], []
        for name, rs in rows.items():
            for p, s, f in rs:
                cid.append(eng.contig_index[name]); pos.append(p); strand.append(ord(s)); frac.append(f)
        order = np.random.default_rng(3).permutation(len(cid))                               # rows arrive in no particular order
        eng.upload_pileup(mt, np.array(cid, np.uint32)[order], np.array(pos, np.uint32)[order], np.array(strand, np.uint8)[order],
                          np.array(frac, np.float64)[order], high=wg.HIGH)
    return eng


def _planned(plan, tag, host, capfd, monkeypatch):
    """plan_all on ``plan`` with NM_PLAN_TIMING=1, once per (plan, mode) and module"""
    if (tag, host) in _runs:
        return _runs[(tag, host)]
    from nanomotif_amd.engine import DeviceWindowExtractor, DeviceWindowStore
    monkeypatch.setenv("NM_PLAN_TIMING", "1")
    if host:
        monkeypatch.setenv("NM_HOST_DRAWS", "1")
    else:
        monkeypatch.delenv("NM_HOST_DRAWS", raising=False)
    run = _Run()
    run.eng = _upload(plan)
    run.store = DeviceWindowStore(run.eng)
    ext = DeviceWindowExtractor(run.eng, run.store, {n: len(s) for n, s in plan.seqs.items()}, None, plan.pad,
                                background_sampling_frequency=plan.freq)
    spy = _PlanSpy(run.eng.lib)
    run.eng.lib = spy
    random.seed(424242)                                         # anything but the plan's seed: plan_all has to seed itself
    capfd.readouterr()
    try:
        run.pssms = ext.plan_all([(key, names, key[1]) for key, names in plan.tasks], seed=plan.seed, one_stream_per_bin=True)
    finally:
        run.eng.lib = spy._lib
    run.state = random.getstate()
    run.lines = [ln for ln in capfd.readouterr().err.splitlines() if "[nm_plan_windows]" in ln]
    run.n_bg = dict(zip((key for key, _ in plan.tasks), spy.n_bg.tolist()))
    _runs[(tag, host)] = run
    return run


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for run in _runs.values():
        run.eng.close()
    _runs.clear()


def _assert_drew(run, where):
    assert len(run.lines) == 1, run.lines
    assert re.search(r"\((device|host) draws\)", run.lines[0]).group(1) == where, run.lines[0]


def _assert_equals_brute(plan, run, brute, state):
    kept = [key for key, _ in plan.tasks if brute[key] is not None]
    assert list(run.pssms) == kept and len(kept) < len(plan.tasks)
    for key in kept:
        counts, n_bg, windows = brute[key]
        assert run.n_bg[key] == n_bg, key
        assert run.store.totals[key] == len(windows), key
        assert np.array_equal(run.pssms[key], np.array(counts, dtype=np.int64) / n_bg), key          # bitwise
    assert all(run.n_bg[key] == 0 for key, _ in plan.tasks if brute[key] is None)
    assert run.state == state


@pytest.mark.parametrize("host", [False, True], ids=["device_draws", "host_draws"])
def test_plan_equals_brute_force(host, capfd, monkeypatch):
    """tasks kept, background PSSMs bitwise, n_bg, window totals and the interpreter's generator afterwards; and the path that drew"""
    plan = wg.build_input()
    run = _planned(plan, "geometry", host, capfd, monkeypatch)
    _assert_drew(run, "host" if host else "device")
    brute, state = wg.brute_of_input()
    _assert_equals_brute(plan, run, brute, state)


@pytest.mark.parametrize("host", [False, True], ids=["device_draws", "host_draws"])
def test_windows_through_the_window_engine(host, capfd, monkeypatch):
    """total, the all-'.' PSSM (the windows themselves for a task of one) and PSSMs narrowed by a literal, a two-base set and the centre,
    at three columns, for every kept task: what win_gather_all_kernel wrote against the brute force's window list"""
    plan = wg.build_input()
    run = _planned(plan, "geometry", host, capfd, monkeypatch)
    brute, _ = wg.brute_of_input()
    batch, want = [], []
    for key, _ in plan.tasks:
        if brute[key] is None:
            continue
        windows = brute[key][2]
        batch.append((key, ps.WinReq("total")))
        want.append(len(windows))
        for motif in wg.request_motifs(plan.pad, MOD_TYPE_TO_CANONICAL[key[1]]):
            batch.append((key, ps.WinReq("pssm", motif)))
            want.append(wg.expected_pssm(windows, motif))
    got = run.store.execute(batch)
    empty = 0
    for (key, req), g, w in zip(batch, got, want):
        if req.kind == "total":
            assert g == w, key
        else:
            assert g[0] == w[0] and np.array_equal(g[1], np.array(w[1], dtype=np.int64)), (key, req.motif)
            empty += w[0] == 0
    assert empty > 0                                            # n_active == 0 replies are among them


def test_select_returns_the_window_of_every_rank(capfd, monkeypatch):
    """nm_bg_counts with one sample per task for every rank 0 .. n-1 of each select contig: the reply is the one-hot window of the k-th
    valid start; rank n is refused, and the engine answers the next valid call"""
    plan = wg.build_input()
    eng = _planned(plan, "geometry", False, capfd, monkeypatch).eng
    u32, u64, i64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    pad, W = plan.pad, 2 * plan.pad + 1

    def counts_of(name, ranks):
        n = len(ranks)
        sc = np.full(n, eng.contig_index[name], dtype=np.uint32)
        sr = np.array(ranks, dtype=np.uint32)
        begin = np.arange(n + 1, dtype=np.uint64)
        out = np.zeros((n, 4, W), dtype=np.int64)
        rc = eng.lib.nm_bg_counts(eng.ctx, ord(plan.base_of[name]), pad, n, sc.ctypes.data_as(u32), sr.ctypes.data_as(u32), n,
                                  begin.ctypes.data_as(u64), out.ctypes.data_as(i64))
        return rc, out

    assert len(plan.select_contigs) >= 4
    for name in plan.select_contigs:
        seq = plan.seqs[name]
        starts = wg.valid_starts(seq, plan.base_of[name], pad)
        want = np.zeros((len(starts), 4, W), dtype=np.int64)
        for k, s in enumerate(starts):
            for col, ch in enumerate(seq[s - pad:s + pad + 1]):
                if ch != "N":
                    want[k, wg.ROWS.index(ch), col] = 1
        rc, got = counts_of(name, range(len(starts)))
        assert rc == 0, eng.lib.nm_last_error()
        wrong = np.flatnonzero((got != want).any(axis=(1, 2)))
        assert len(wrong) == 0, (name, [(int(k), starts[k]) for k in wrong[:8]])
        rc, _ = counts_of(name, [len(starts)])
        assert rc != 0 and b"valid starts" in eng.lib.nm_last_error(), name
        rc, got = counts_of(name, [len(starts) - 1, 0])
        assert rc == 0 and np.array_equal(got, want[[-1, 0]]), name


def test_pool_call_too_long_for_the_device_is_drawn_on_the_host(capfd, monkeypatch):
    """a pool call with k > 4096 sends the whole plan to the host threads; the same plan without it is drawn on the device; both equal
    the brute force"""
    for with_long, where in ((False, "device"), (True, "host")):
        plan = wg.build_long_pool_input(with_long)
        run = _planned(plan, "long_pool_%d" % with_long, False, capfd, monkeypatch)
        _assert_drew(run, where)
        saved = random.getstate()
        brute, state = wg.brute_plan(plan)
        random.setstate(saved)
        kept = [key for key, _ in plan.tasks]
        assert list(run.pssms) == kept
        for key in kept:
            counts, n_bg, windows = brute[key]
            assert run.n_bg[key] == n_bg and run.store.totals[key] == len(windows), key
            assert np.array_equal(run.pssms[key], np.array(counts, dtype=np.int64) / n_bg), key
        assert run.state == state
