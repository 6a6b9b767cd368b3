"""Host side of ``nanomotif motif_tracks`` (no GPU): the brute force both suites compare against — built only from
``oracle.scan.subseq_indices`` / ``oracle.motif.Motif`` (through ``test_motif_profile_host.occurrences``) and ``oracle.scan.split_positions``
(through ``test_gpu_motif_compare.oracle_calls``) — the conditions on the geometry input it runs on, the window layout, the segmentation on
hand-written tables, the three files byte for byte, ``--window``, and the exports in the header and the binding.

The brute force is the definition: ``tracks_of`` bins every occurrence by ``p // W`` into column ``3 * strand + state``."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser
from test_gpu_motif_compare import oracle_calls, reach_class, state_of
from test_motif_profile_host import occurrences, profile_cands
from test_motif_strands_host import geometry_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192
WINDOWS = (128, 384, 640, 4096, 8192, 16384, 1 << 20)                   # the GPU suite's window sizes


# ------------------------------------------------------------------------------------------------ the brute force
def n_windows(length, W):
    return max(1, -(-length // W))


def tracks_of(seq, calls, motif, i, W):
    """int64[n_windows, 6] of one candidate on one contig: (fwd mod, fwd nomod, fwd nocall, rev mod, rev nomod, rev nocall) per window."""
    t = np.zeros((n_windows(len(seq), W), 6), dtype=np.int64)
    for p, s in occurrences(seq, motif, i):
        t[p // W, 3 * s + state_of((p, s), calls)] += 1
    return t


@functools.lru_cache(maxsize=None)
def geometry_calls():
    """contig name -> (M, U) of the geometry input's "a" pileup at the default thresholds."""
    from oracle.scan import _EMPTY
    names, seqs, _, _, _, piles = geometry_input()
    return {n: oracle_calls(piles["a"].get(n, _EMPTY), 0.3, 0.7) for n in names}


@functools.lru_cache(maxsize=None)
def classified(name, motif, i):
    """(positions, columns) of the occurrences of one candidate on one contig of the geometry input: found and classified once, binned
    per window size by ``expected_table``."""
    _, seqs, _, _, _, _ = geometry_input()
    calls = geometry_calls()[name]
    occ = occurrences(seqs[name], motif, i)
    return (np.array([p for p, _ in occ], dtype=np.int64), np.array([3 * s + state_of((p, s), calls) for p, s in occ], dtype=np.int64))


def track_cands():
    """[(bin, mod type, motif, mod position)]: the candidates of ``test_motif_profile_host.profile_cands`` on mod type ``a``."""
    return [c for c in profile_cands() if c[1] == "a"]


def bin_contigs_of():
    names, _, bins, _, _, _ = geometry_input()
    return {b: [n for n in names if bins[n] == b] for b in ("b0_empty", "b1", "b2")}


@functools.lru_cache(maxsize=None)
def expected_table(b, motif, i, W):
    """(contig names, window prefix, int64[n_windows of the bin, 6]) of one candidate: the item ``ScanEngine.motif_tracks`` yields."""
    _, seqs, _, _, _, _ = geometry_input()
    names = bin_contigs_of()[b]
    prefix = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum([n_windows(len(seqs[n]), W) for n in names], out=prefix[1:])
    table = np.zeros((int(prefix[-1]), 6), dtype=np.int64)
    for k, n in enumerate(names):
        pos, col = classified(n, motif, i)
        np.add.at(table, (prefix[k] + pos // W, col), 1)
    table.setflags(write=False)
    return names, prefix, table


# ------------------------------------------------------------------------------------------------ 1. conditions on the input
def test_the_vectorised_binning_is_the_loop():
    _, seqs, _, _, _, _ = geometry_input()
    for name, b in (("edge", "b1"), ("small", "b1"), ("tiny2", "b1"), ("mid", "b2")):
        for W in (128, 384, 8192):
            names, prefix, table = expected_table(b, "GATC", 1, W)
            k = names.index(name)
            assert np.array_equal(table[prefix[k]:prefix[k + 1]], tracks_of(seqs[name], geometry_calls()[name], "GATC", 1, W)), (name, W)


def test_the_input_is_not_degenerate():
    _, seqs, _, _, _, _ = geometry_input()
    calls = geometry_calls()
    assert {reach_class(m, i) for _, _, m, i in track_cands()} == {0, 1, 2} and {b for b, _, _, _ in track_cands()} == {"b1", "b2"}
    # A @ 0 on the 30 kbp contig: every column is non-zero in all but at most one window
    assert len(seqs["big"]) == 30_000
    for W, n_win in ((128, 235), (384, 79), (640, 47), (8192, 4)):
        t = tracks_of(seqs["big"], calls["big"], "A", 0, W)
        assert len(t) == n_win
        nonzero = (t > 0).sum(axis=0)
        print("A @ 0, W =", W, "non-zero windows per column:", nonzero.tolist())
        assert (nonzero >= n_win - 1).all(), (W, nonzero.tolist())
    # GATC @ 1 at W = 384: window 21 takes one occurrence from either side of a chunk border — the row two work items add to
    occ = occurrences(seqs["big"], "GATC", 1)
    assert sorted(x for x in occ if 8064 <= x[0] < 8448) == [(8191, 0), (8192, 1)]
    assert 8191 // CHUNK != 8192 // CHUNK and 8191 // 384 == 8192 // 384 == 21
    t = tracks_of(seqs["big"], calls["big"], "GATC", 1, 384)
    assert t[21].sum() == 2 and t[21, :3].sum() == 1 and t[21, 3:].sum() == 1
    print("GATC @ 1, W = 384: non-empty windows", int(t.any(axis=1).sum()), "column sums", t.sum(axis=0).tolist())
    assert t.any(axis=1).sum() >= 50 and (t.sum(axis=0) > 20).all()
    # the contigs shorter than the motif give one all-zero window each; exactly one chunk gives 64 windows at 128
    for name in ("tiny1", "tiny2", "tiny3"):
        for W in (128, 1 << 20):
            t = tracks_of(seqs[name], calls[name], "GATC", 1, W)
            assert t.shape == (1, 6) and not t.any()
    assert len(seqs["edge"]) == CHUNK and len(tracks_of(seqs["edge"], calls["edge"], "GATC", 1, 128)) == 64
    # both bins hold occurrences of every candidate, and windows astride a chunk border exist at 384 and 640 only
    for b, _, m, i in track_cands():
        assert expected_table(b, m, i, 4096)[2].sum() > 0, (b, m)
    assert CHUNK % 384 and CHUNK % 640 and not CHUNK % 128 and not CHUNK % 4096


# ------------------------------------------------------------------------------------------------ 2. the layout
def test_window_prefix_and_the_allowed_sizes():
    from nanomotif_amd.engine import TRACK_BUDGET_BYTES, TRACK_ROW_BYTES, TRACKS_MIN_WINDOW, track_window, window_prefix
    assert (TRACKS_MIN_WINDOW, TRACK_ROW_BYTES, TRACK_BUDGET_BYTES) == (128, 24, 256 << 20)
    lengths = [1, 127, 128, 129, 8192, 8193, 30_000]
    want = {128: [1, 1, 1, 2, 64, 65, 235], 384: [1, 1, 1, 1, 22, 22, 79], 8192: [1, 1, 1, 1, 1, 2, 4], 1 << 20: [1] * 7}
    for W, counts in want.items():
        assert [max(1, math.ceil(n / W)) for n in lengths] == counts
        p = window_prefix(lengths, W)
        assert p.dtype == np.int64 and p[0] == 0 and np.diff(p).tolist() == counts, W
    assert window_prefix([], 128).tolist() == [0] and window_prefix([0], 128).tolist() == [0, 1]
    assert [track_window(w) for w in (128, "256", 1 << 30)] == [128, 256, 1 << 30]
    for bad in (0, 100, 127, 129, 4000, (1 << 30) + 128, 1 << 31, -128):
        with pytest.raises(ValueError) as e:
            track_window(bad)
        assert "window" in str(e.value)
        with pytest.raises(ValueError):
            window_prefix([10], bad)


def test_engine_refuses_a_window_before_it_needs_a_device():
    from nanomotif_amd.engine import ScanEngine
    eng = ScanEngine.__new__(ScanEngine)                                # no context: the checks come first
    for bad in (100, 0, 1 << 31):
        with pytest.raises(ValueError):
            ScanEngine.motif_tracks(eng, [], window=bad)
        with pytest.raises(ValueError):
            ScanEngine.track_windows(eng, 0, bad)
    with pytest.raises(ValueError):
        ScanEngine.motif_tracks(eng, [], max_bytes=0)
    eng.ctx = None                                                      # (nothing for __del__ to destroy)


# ------------------------------------------------------------------------------------------------ 3. segmentation
def ll_plain(m, n):
    out = 0.0
    if m > 0:
        out += m * math.log(m / n)
    if n - m > 0:
        out += (n - m) * math.log((n - m) / n)
    return out


def gains_by_loops(mod, nomod, min_called):
    """{k: gain} of every admissible split of the whole series, one split at a time."""
    m, c = sum(mod), sum(mod) + sum(nomod)
    out = {}
    for k in range(1, len(mod)):
        m_l, c_l = sum(mod[:k]), sum(mod[:k]) + sum(nomod[:k])
        if c_l >= min_called and c - c_l >= min_called:
            out[k] = 2 * (ll_plain(m_l, c_l) + ll_plain(m - m_l, c - c_l) - ll_plain(m, c))
    return out


def test_a_step_is_found_where_it_is():
    from nanomotif_amd.motif_tracks import segment
    mod, nomod = [8] * 20 + [0] * 20, [0] * 20 + [8] * 20
    bounds, first = segment(mod, nomod, 30.0, 20, 8)
    assert bounds == [0, 20, 40]
    k, gain, left, right = first
    assert (k, left, right) == (20, (160, 160), (0, 160))
    assert abs(gain - 2 * 320 * math.log(2)) <= 1e-9 * 2 * 320 * math.log(2)
    by_loops = gains_by_loops(mod, nomod, 20)
    assert max(by_loops, key=lambda q: (by_loops[q], -q)) == 20 and abs(by_loops[20] - gain) <= 1e-9 * gain


def test_a_uniform_contig_is_one_segment():
    from nanomotif_amd.motif_tracks import segment
    bounds, first = segment([8] * 40, [0] * 40, 30.0, 20, 8)
    assert bounds == [0, 40] and first[1] == 0.0 and first[0] == 3       # every gain is 0: the lowest admissible k (24 called sites)
    assert segment([], [], 30.0, 20, 8) == ([0, 0], None) and segment([5], [5], 30.0, 0, 8) == ([0, 1], None)
    assert segment([0] * 10, [0] * 10, 30.0, 20, 8) == ([0, 10], None)


def test_an_island_is_three_segments():
    from nanomotif_amd.motif_tracks import segment
    mod = [8] * 12 + [0] * 8 + [8] * 20
    nomod = [0] * 12 + [8] * 8 + [0] * 20
    bounds, first = segment(mod, nomod, 30.0, 20, 8)
    assert bounds == [0, 12, 20, 40]
    by_loops = gains_by_loops(mod, nomod, 20)
    best = max(by_loops, key=lambda q: (by_loops[q], -q))
    assert first[0] == best and abs(first[1] - by_loops[best]) <= 1e-9 * by_loops[best]
    # --max_segments 2 stops at two, at the best first split; 1 never splits
    assert segment(mod, nomod, 30.0, 20, 2)[0] == [0, best, 40] and segment(mod, nomod, 30.0, 20, 1)[0] == [0, 40]
    # a gain below --min_gain is reported and not accepted
    bounds, first = segment(mod, nomod, 1e6, 20, 8)
    assert bounds == [0, 40] and first[0] == best


def test_admissibility_and_ties():
    from nanomotif_amd.motif_tracks import segment
    # the step sits 2 windows = 16 called sites from the end: no split there at --min_called 20, the nearest admissible one instead
    mod, nomod = [8] * 38 + [0] * 2, [0] * 38 + [8] * 2
    assert segment(mod, nomod, 30.0, 16, 8)[0] == [0, 38, 40]
    bounds, first = segment(mod, nomod, 30.0, 20, 8)
    assert first[0] == 37 and first[3] == (8, 24)
    by_loops = gains_by_loops(mod, nomod, 20)
    assert set(by_loops) == set(range(3, 38)) and max(by_loops, key=lambda q: (by_loops[q], -q)) == 37
    # too few called sites in all: nothing is admissible
    assert segment([8, 8], [0, 0], 0.0, 20, 8) == ([0, 2], None)
    # windows without a called site between the two halves: the splits at 10, 11 and 12 hold the same sums; the lowest wins
    mod, nomod = [8] * 10 + [0, 0] + [0] * 10, [0] * 10 + [0, 0] + [8] * 10
    bounds, first = segment(mod, nomod, 30.0, 20, 8)
    by_loops = gains_by_loops(mod, nomod, 20)
    assert by_loops[10] == by_loops[11] == by_loops[12] == max(by_loops.values())
    assert bounds == [0, 10, 22] and first[0] == 10
    # two steps of equal gain in two segments: the leftmost segment is split first (--max_segments 3 shows which)
    mod = [8] * 5 + [0] * 5 + [8] * 5 + [0] * 5 + [8] * 5
    nomod = [8 - x for x in mod]
    assert segment(mod, nomod, 30.0, 20, 8)[0] == [0, 5, 10, 15, 20, 25]
    first_two = segment(mod, nomod, 30.0, 20, 2)[0]
    three = segment(mod, nomod, 30.0, 20, 3)[0]
    assert len(first_two) == 3 and len(three) == 4 and set(first_two) <= set(three)


NOISE_SEED = 22                                                         # (its largest gain is 11.9; the seeds 0 .. 39 give 1.6 .. 11.9)


def test_a_noisy_uniform_series_stays_one_segment():
    from nanomotif_amd.motif_tracks import segment
    rng = np.random.default_rng(NOISE_SEED)
    called = rng.poisson(8, size=300)
    mod = rng.binomial(called, 0.9)
    nomod = called - mod
    by_loops = gains_by_loops(mod.tolist(), nomod.tolist(), 20)
    print("largest brute-force gain of the null series:", max(by_loops.values()))
    assert max(by_loops.values()) < 30
    bounds, first = segment(mod, nomod, 30.0, 20, 8)
    assert bounds == [0, 300]
    best = max(by_loops, key=lambda q: (by_loops[q], -q))
    assert first[0] == best and abs(first[1] - by_loops[best]) <= 1e-9 * by_loops[best]
    assert len(segment(mod, nomod, by_loops[best] * 0.5, 20, 8)[0]) > 2  # the knob: a lower --min_gain splits it


# ------------------------------------------------------------------------------------------------ 4. the three files
def _cand(bin, motif, mod_type, pos):
    from nanomotif_amd.motif_sites import SiteCandidate
    return SiteCandidate(bin, motif, mod_type, pos)


def test_the_three_files_byte_for_byte():
    from nanomotif_amd.motif_tracks import CONTIGS_HEADER, SEGMENTS_HEADER, TRACKS_HEADER, format_files
    W = 256
    lengths = {"c1": 1000, "c2": 200}                                   # 4 windows, the last one 232 bp; 1 window
    names, prefix = ["c1", "c2"], np.array([0, 4, 5])
    table = np.array([[10, 0, 1, 12, 0, 0], [11, 1, 0, 10, 0, 2], [0, 9, 0, 0, 12, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]], dtype=np.uint32)
    bg = np.array([[50, 50, 7, 50, 50, 7], [60, 40, 0, 40, 60, 0], [10, 90, 0, 10, 90, 0], [0, 0, 9, 0, 0, 9], [3, 1, 0, 1, 3, 0]], dtype=np.uint32)
    cands = [_cand("b1", "GATC", "a", 1)]
    contigs, segments, tracks = format_files(cands, [(names, prefix, table)], {("b1", "a"): bg}, lengths, W, min_gain=30.0, min_called=20,
                                             max_segments=8, tracks=True)
    gain = 2 * (ll_plain(43, 44) + ll_plain(0, 21) - ll_plain(43, 65))
    assert contigs == ("\t".join(CONTIGS_HEADER) + "\n" +
                       f"b1\tc1\tGATC\ta\t1\t1000\t4\t43\t22\t3\t0.661538\t2\t512\t{gain:.3f}\t0.977273\t0.000000\tbreakpoint\n"
                       "b1\tc2\tGATC\ta\t1\t200\t1\t2\t2\t2\t0.500000\t1\t\t\t\t\tuniform\n")
    assert segments == ("\t".join(SEGMENTS_HEADER) + "\n" +
                        "b1\tc1\tGATC\ta\t1\t0\t0\t512\t43\t1\t3\t0.977273\t200\t200\t0.500000\n"
                        "b1\tc1\tGATC\ta\t1\t1\t512\t1000\t0\t21\t0\t0.000000\t20\t180\t0.100000\n"
                        "b1\tc2\tGATC\ta\t1\t0\t0\t200\t2\t2\t2\t0.500000\t4\t4\t0.500000\n")
    assert tracks == ("\t".join(TRACKS_HEADER) + "\n" +
                      "c1\t0\t256\tb1\tGATC\ta\t1\t10\t0\t1\t12\t0\t0\t1.000000\n"
                      "c1\t256\t512\tb1\tGATC\ta\t1\t11\t1\t0\t10\t0\t2\t0.954545\n"
                      "c1\t512\t768\tb1\tGATC\ta\t1\t0\t9\t0\t0\t12\t0\t0.000000\n"
                      "c2\t0\t200\tb1\tGATC\ta\t1\t1\t1\t1\t1\t1\t1\t0.500000\n")
    assert CONTIGS_HEADER == ["bin", "contig", "motif", "mod_type", "mod_position", "length", "n_windows", "n_mod", "n_nomod", "n_nocall", "frac_mod",
                              "n_segments", "best_split", "best_gain", "frac_left", "frac_right", "flag"]
    assert SEGMENTS_HEADER == ["bin", "contig", "motif", "mod_type", "mod_position", "segment", "start", "end", "n_mod", "n_nomod", "n_nocall", "frac_mod",
                               "bg_n_mod", "bg_n_nomod", "bg_frac_mod"]
    # without --tracks no third file; without a background block its columns are empty; --min_gain above the gain: reported, not accepted
    contigs, segments, tracks = format_files(cands, [(names, prefix, table)], {}, lengths, W, min_gain=100.0)
    assert tracks is None
    assert contigs.split("\n")[1] == f"b1\tc1\tGATC\ta\t1\t1000\t4\t43\t22\t3\t0.661538\t1\t512\t{gain:.3f}\t0.977273\t0.000000\tuniform"
    assert segments.split("\n")[1:3] == ["b1\tc1\tGATC\ta\t1\t0\t0\t1000\t43\t22\t3\t0.661538\t\t\t", "b1\tc2\tGATC\ta\t1\t0\t0\t200\t2\t2\t2\t0.500000\t\t\t"]
    # three segments and more are islands
    isl = np.zeros((40, 6), dtype=np.uint32)
    isl[:, 0] = [8] * 12 + [0] * 8 + [8] * 20
    isl[:, 4] = [0] * 12 + [8] * 8 + [0] * 20
    contigs, segments, _ = format_files(cands, [(["c1"], np.array([0, 40]), isl)], {}, {"c1": 40 * W - 5}, W)
    # (the first split is the island's far end: 96 of 160 against 160 of 160 beats 96 of 96 against 160 of 224)
    assert contigs.split("\n")[1].split("\t")[11:] == ["3", str(20 * W), "%.3f" % gains_by_loops(isl[:, 0].tolist(), isl[:, 4].tolist(), 20)[20], "0.600000",
                                                       "1.000000", "islands"]
    assert [r.split("\t")[5:8] for r in segments.split("\n")[1:-1]] == [["0", "0", str(12 * W)], ["1", str(12 * W), str(20 * W)],
                                                                         ["2", str(20 * W), str(40 * W - 5)]]


def test_background_keys_follow_the_candidates():
    from nanomotif_amd.motif_tracks import background_keys
    cands = [_cand("b2", "GATC", "a", 1), _cand("b1", "CCWGG", "m", 1), _cand("b2", "AATT", "a", 0), _cand("b2", "CCWGG", "m", 1)]
    assert background_keys(cands) == [("b2", "a"), ("b1", "m"), ("b2", "m")] and background_keys([]) == []


def test_parser_accepts_motif_tracks(capsys):
    from nanomotif_amd.motif_tracks import parse_window
    p = create_parser()
    a = p.parse_args(["motif_tracks", "asm.fasta", "p.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "tr"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.out, a.bin_motifs) == ("motif_tracks", "asm.fasta", "p.bed", "contig_bin.tsv", "tr", ["out/bin-motifs.tsv"])
    assert (a.window, a.min_gain, a.min_called, a.max_segments, a.tracks) == (4096, 30.0, 20, 8, False)
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose, a.threads) == (0.3, 0.7, 5, None, False, 1)
    a = p.parse_args(["motif_tracks", "asm.fasta", "p.bed.gz", "-d", "bins", "--bin_motifs", "a.tsv", "b.tsv", "--window", "128", "--min_gain", "12.5",
                      "--min_called", "5", "--max_segments", "3", "--tracks", "--device", "1", "-v", "-t", "4"])
    assert (a.window, a.min_gain, a.min_called, a.max_segments, a.tracks, a.bin_motifs, a.device) == (128, 12.5, 5, 3, True, ["a.tsv", "b.tsv"], 1)
    assert p.parse_args(["motif_tracks", "a", "p", "-c", "cb", "--bin_motifs", "b", "--window", str(1 << 30)]).window == 1 << 30
    for bad in ("100", "0", str(1 << 31), "x", "-128", "4097"):
        with pytest.raises(SystemExit):
            p.parse_args(["motif_tracks", "asm.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "b.tsv", "--window", bad])
        assert "--window" in capsys.readouterr().err
        with pytest.raises(ValueError) as e:
            parse_window(bad)
        assert "--window" in str(e.value)
    with pytest.raises(SystemExit):
        p.parse_args(["motif_tracks", "asm.fasta", "p.bed", "-c", "cb.tsv"])
    capsys.readouterr()
    assert "motif_tracks" in p.format_help()


def test_exports_are_declared_bound_and_built():
    from nanomotif_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    assert "int nm_tracks_windows(" in header and "int nm_motif_tracks_count(" in header and "#define NM_TRACKS_MIN_WINDOW 128" in header
    assert "nm_tracks_windows" in _lib.SYMBOLS and "nm_motif_tracks_count" in _lib.SYMBOLS
    assert any(os.path.basename(s) == "nmtracks.hip" for s in build.SRC_HIP)
    lib = _lib.load()
    q = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    bins, slots, lens, modpos, off, masks = (np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.array([1], np.uint8), np.zeros(1, np.uint8),
                                             np.zeros(1, np.uint32), np.array([1], np.uint8))
    rows, counts = np.array([0, 1], np.uint64), np.zeros(6, np.uint32)
    cand = (q(bins, C.c_uint32), q(slots, C.c_uint8), q(lens, C.c_uint8), q(modpos, C.c_uint8), q(off, C.c_uint32), q(masks, C.c_uint8))
    call = lambda cand=cand, window=4096, rows=q(rows, C.c_uint64), out=q(counts, C.c_uint32): lib.nm_motif_tracks_count(None, 1, *cand, window, rows, out)
    # refused with a NULL ctx, before any device call, and by name: the window before the ctx
    for kw, word in ((dict(cand=(None,) * 6), "NULL"), (dict(rows=None), "NULL"), (dict(out=None), "NULL"), (dict(cand=cand[:3] + (None,) + cand[4:]), "NULL"),
                     (dict(window=100), "window_bp"), (dict(window=0), "window_bp"), (dict(window=1 << 31), "window_bp"), (dict(window=(1 << 30) + 128), "window_bp"),
                     (dict(), "ctx")):
        assert call(**kw) == -1, kw                                     # NM_EINVAL
        assert word in lib.nm_last_error().decode(), (kw, lib.nm_last_error())
    n = C.c_uint32(0)
    for window, word in ((100, "window_bp"), (0, "window_bp"), (128, "ctx")):
        assert lib.nm_tracks_windows(None, 0, window, None, 0, C.byref(n)) == -1 and word in lib.nm_last_error().decode()
    assert lib.nm_tracks_windows(None, 0, 128, None, 0, None) == -1 and "NULL" in lib.nm_last_error().decode()
    assert not counts.any()
