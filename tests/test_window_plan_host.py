"""The helpers of tests/window_plan_geometry.py checked on the CPU: the tile model of the sampler against the interpreter's
``random.sample``, the brute force of the window plan against ``search.extract_windows`` (each pins the other), and the census of the
geometry input: every border the GPU tests of tests/test_gpu_window_plan.py rely on is in the input, by count."""
import random

import numpy as np
import pytest

import window_plan_geometry as wg
from nanomotif_amd import search as ps
from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL


@pytest.fixture(scope="module")
def inp():
    return wg.build_input()


def _streams_with_calls(inp):
    return [inp.calls_of_stream(s) for s in wg.streams_of(inp.tasks)]


def test_tile_model_equals_random_sample(inp):
    """samples and raw draws consumed, on every stream of the input and of the long-pool plan"""
    for plan in (inp, wg.build_long_pool_input()):
        raw = wg.raw_outputs(plan.seed, 1 << 16)
        streams = _streams_with_calls(plan)
        assert len(streams) >= 32 and all(streams)
        for calls in streams:
            samples, consumed, _ = wg.tile_stream(raw, calls)
            random.seed(plan.seed)
            assert samples == [random.sample(range(n), k) for n, k in calls], calls
            rng = random.Random(plan.seed)
            for _ in range(consumed):
                rng.getrandbits(32)
            assert rng.getstate() == random.getstate(), calls


def test_committed_cut_values_are_what_the_search_finds():
    assert wg.search_cut(0) == wg.CUT_LANE_0_N and wg.search_cut(63) == wg.CUT_LANE_63_N


def test_every_event_is_in_the_input(inp):
    brute, _ = wg.brute_of_input()
    census = wg.census(inp, brute)
    missing = [e for e in wg.required_events() if census[e] < 1]
    assert not missing, missing
    assert sum(len(s) for s in inp.seqs.values()) <= 2_000_000
    streams = wg.streams_of(inp.tasks)
    assert len(streams) >= 40 and sum(len(s) > 1 for s in streams) >= 2          # the device path; streams of several tasks
    # the setsize border falls where random.py puts it
    assert wg.setsize_of(50) == 277 and wg.setsize_of(85) == 277 and wg.setsize_of(86) == 1045 and wg.setsize_of(1400) == 16405
    # every k is what its length was chosen for, well away from where ceil could differ between two implementations
    for name, seq in inp.seqs.items():
        x = len(seq) * inp.freq
        assert x < 49.5 or abs(x - round(x)) > 0.05, name
    # the long-pool plan: one pool call with k > 4096, and none without it
    for with_long, want in ((True, 1), (False, 0)):
        plan = wg.build_long_pool_input(with_long)
        assert wg.sampler_census(plan)["pool_k_above_4096"] == want and len(wg.streams_of(plan.tasks)) >= 32


def _host_task(plan, key, names):
    """search.extract_windows on one task: contigs as uint8 arrays, confident rows per strand in ascending order"""
    mt = key[1]
    seqs = {n: np.frombuffer(plan.seqs[n].encode(), dtype=np.uint8) for n in names}
    plus, minus = {}, {}
    for n in names:
        rows = plan.rows[mt].get(n, [])
        plus[n] = np.array(sorted(p for p, s, f in rows if s == "+" and f >= wg.HIGH), dtype=np.int64)
        minus[n] = np.array(sorted(p for p, s, f in rows if s == "-" and f >= wg.HIGH), dtype=np.int64)
    return ps.extract_windows(seqs, plus, minus, mt, plan.pad, plan.freq)


@pytest.mark.parametrize("which", ["geometry", "long_pool"])
def test_brute_force_and_extract_windows_pin_each_other(which):
    plan = wg.build_input() if which == "geometry" else wg.build_long_pool_input()
    letters = np.array([ord(c) for c in "?AC?G???T??????N"], dtype=np.uint8)
    for key, names in plan.tasks:
        random.seed(plan.seed)
        brute = wg.brute_task(plan.seqs, plan.rows[key[1]], names, MOD_TYPE_TO_CANONICAL[key[1]], plan.pad, plan.freq)
        state = random.getstate()
        random.seed(plan.seed)
        host = _host_task(plan, key, names)
        assert random.getstate() == state, key
        assert (brute is None) == (host is None), key
        if brute is None:
            continue
        counts, n_bg, windows = brute
        assert [bytes(letters[row]).decode() for row in host[0]] == windows, key
        assert np.array_equal(np.array(counts, dtype=np.int64) / n_bg, host[1]), key


def test_expected_pssm_equals_the_host_window_store(inp):
    brute, _ = wg.brute_of_input()
    store = ps.HostWindowStore()
    for key, names in inp.tasks:
        if brute[key] is None:
            continue
        windows = brute[key][2]
        store.add_task(key, np.array([[wg.SET_OF[ch] for ch in w] for w in windows], dtype=np.uint8))
        for motif in wg.request_motifs(inp.pad, MOD_TYPE_TO_CANONICAL[key[1]]):
            n, counts = wg.expected_pssm(windows, motif)
            got = store.execute([(key, ps.WinReq("pssm", motif))])[0]
            assert got[0] == n and (n == 0 or np.array_equal(got[1], np.array(counts))), (key, motif)
