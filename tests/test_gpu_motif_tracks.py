"""GPU: motif methylation along contigs (nm_tracks_windows, nm_motif_tracks_count, ``ScanEngine.motif_tracks``, ``nanomotif motif_tracks``)
against the brute force of ``test_motif_tracks_host`` (built only from ``oracle.scan.subseq_indices``, ``oracle.scan.split_positions`` and
``oracle.motif.Motif``).  Counts are integers: every comparison is an equality over the WHOLE table of every candidate.  The conditions on
the input (``test_motif_tracks_host.test_the_input_is_not_degenerate``) need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from nanomotif_amd.motif import Motif
from test_gpu_motif_compare import _body, _run
from test_motif_strands_host import geometry_input
from test_motif_tracks_host import WINDOWS, expected_table, gains_by_loops, n_windows, track_cands, tracks_of

gpu = pytest.mark.gpu
NM_EINVAL, NM_ESTATE, NM_ERANGE = -1, -3, -5


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


@pytest.fixture(scope="module")
def tracks_engine(engine_cls):
    names, seqs, bins, bin_names, rows, _ = geometry_input()
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names], bin_names=bin_names)
    eng.upload_pileup("a", *rows)
    yield eng
    eng.close()


def engine_cands(cands):
    return [(Motif(m, i), mt, b) for b, mt, m, i in cands]


def first_difference(cand, names, prefix, got, want):
    """The first differing (candidate, contig, window, column) of two tables, for the message."""
    r, col = np.argwhere(np.asarray(got, np.int64) != want)[0].tolist()
    k = int(np.searchsorted(prefix, r, side="right")) - 1
    return cand, names[k], r - int(prefix[k]), col, int(got[r, col]), int(want[r, col])


def check_items(cands, items, W):
    assert len(items) == len(cands)
    for c, (names, prefix, table) in zip(cands, items):
        e_names, e_prefix, e_table = expected_table(c[0], c[2], c[3], W)
        assert list(names) == e_names and np.array_equal(prefix, e_prefix), (c, W)
        assert table.dtype == np.uint32 and table.shape == e_table.shape, (c, W, table.shape)
        assert np.array_equal(table, e_table), (W, first_difference(c, e_names, e_prefix, table, e_table))


# ------------------------------------------------------------------------------------------------ 1. a literal case
@gpu
def test_literal_case_by_hand(engine_cls):
    """"GATC" * 40 (160 bp), GATC @ 1, W = 128: on '+' the A at 1, 5, .. 157 (32 below 128, 8 from it on), on '-' the A read at 2, 6, ..
    158 (32 and 8).  Rows: (1, +) 0.9 mod, (5, +) 0.1 nomod, (129, +) 1.0 mod, (2, -) 0.8 mod, (6, -) 0.5 no call, (130, -) 0.0 nomod,
    (3, +) 1.0 no occurrence."""
    eng = engine_cls()
    eng.upload_assembly(["c"], ["GATC" * 40], ["b"])
    eng.upload_pileup("a", [0] * 7, [1, 2, 3, 5, 6, 129, 130], np.frombuffer(b"+-++-+-", np.uint8), [0.9, 0.8, 1.0, 0.1, 0.5, 1.0, 0.0])
    assert eng.track_windows("b", 128).tolist() == [0, 2] and eng.track_windows("b", 256).tolist() == [0, 1]
    items = list(eng.motif_tracks([(Motif("GATC", 1), "a", "b")], window=128))
    assert len(items) == 1
    names, prefix, table = items[0]
    assert names == ["c"] and prefix.tolist() == [0, 2] and table.dtype == np.uint32
    assert table.tolist() == [[1, 1, 30, 1, 0, 31],
                              [1, 0, 7, 0, 1, 7]]
    (_, _, whole), = eng.motif_tracks([(Motif("GATC", 1), "a", "b")], window=256)
    assert whole.tolist() == [[2, 1, 37, 1, 1, 38]]
    assert list(eng.motif_tracks([], window=128)) == []
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. geometry
@gpu
@pytest.mark.parametrize("W", WINDOWS)
def test_windows_that_break_naive_reduction(tracks_engine, W):
    """Every candidate of the host file's input (G = 1, 2, 3; occurrences astride word, lane and chunk borders; the N run; contigs shorter
    than the motif; both non-empty bins) at 128 (one lane per window), 384 (runs of 3 lanes, windows astride chunk borders), 640 (runs of
    5), 4096, 8192 (one window per work item), 16384 (several work items per window) and 2^20 (one window per contig): the whole table
    equals the brute force."""
    eng = tracks_engine
    cands = track_cands()
    before = eng.stats()["launches"]
    items = list(eng.motif_tracks(engine_cands(cands), window=W))
    assert 1 <= eng.stats()["launches"] - before <= 3                   # one call: a launch per reach width, whatever W
    check_items(cands, items, W)
    # a candidate in the empty bin yields no rows, also between two others in one call
    three = [("b0_empty", "a", "GATC", 1), ("b2", "a", "GATC", 1), ("b0_empty", "a", "A", 0), ("b1", "a", "A", 0)]
    got = list(eng.motif_tracks(engine_cands(three), window=W))
    for k in (0, 2):
        assert got[k][0] == [] and got[k][1].tolist() == [0] and got[k][2].shape == (0, 6)
    check_items([three[1], three[3]], [got[1], got[3]], W)
    alone = list(eng.motif_tracks(engine_cands(three[:1]), window=W))
    assert alone[0][0] == [] and alone[0][2].shape == (0, 6)


# ------------------------------------------------------------------------------------------------ 3. identities
@gpu
def test_identities_on_the_device_results(tracks_engine):
    """(a) a contig's windows sum to its row of ``motif_site_counts``; (b) W = 2^20 IS ``motif_site_counts``; (c) the W = 256 table summed
    in pairs is the W = 512 table, a contig's odd last window standing alone; (d) a ``max_bytes`` below one candidate's table and the
    default yield the same sequence."""
    eng = tracks_engine
    cands = track_cands()
    ecands = engine_cands(cands)
    per_contig = eng.motif_site_counts(ecands)
    for W in (128, 384, 4096):
        for c, (names, prefix, table), (s_names, six) in zip(cands, eng.motif_tracks(ecands, window=W), per_contig):
            assert names == s_names
            sums = np.array([table[prefix[k]:prefix[k + 1]].sum(axis=0, dtype=np.int64) for k in range(len(names))]).reshape(-1, 6)
            assert np.array_equal(sums, six), (c, W)
    for c, (names, prefix, table), (_, six) in zip(cands, eng.motif_tracks(ecands, window=1 << 20), per_contig):
        assert prefix.tolist() == list(range(len(names) + 1)) and np.array_equal(table, six) and six.sum() > 0, c
    odd = 0
    for c, (names, p256, t256), (_, p512, t512) in zip(cands, eng.motif_tracks(ecands, window=256), eng.motif_tracks(ecands, window=512)):
        for k in range(len(names)):
            a = t256[p256[k]:p256[k + 1]].astype(np.int64)
            odd += len(a) % 2
            if len(a) % 2:
                a = np.concatenate([a, np.zeros((1, 6), np.int64)])
            assert np.array_equal(a.reshape(-1, 2, 6).sum(axis=1), t512[p512[k]:p512[k + 1]]), (c, names[k])
    assert odd > 0
    default = list(eng.motif_tracks(ecands, window=384))
    before = eng.stats()["launches"]
    small = list(eng.motif_tracks(ecands, window=384, max_bytes=24))    # less than any candidate's table: a call per candidate
    assert eng.stats()["launches"] - before == len(cands)
    assert len(small) == len(default)
    for (n1, p1, t1), (n2, p2, t2) in zip(small, default):
        assert n1 == n2 and np.array_equal(p1, p2) and np.array_equal(t1, t2)
    check_items(cands, small, 384)
    middle = list(eng.motif_tracks(ecands, window=384, max_bytes=3 * 24 * 120))    # a few candidates a call
    for (n1, p1, t1), (n2, p2, t2) in zip(middle, default):
        assert n1 == n2 and np.array_equal(p1, p2) and np.array_equal(t1, t2)


# ------------------------------------------------------------------------------------------------ 4. refusals
@gpu
def test_errors_are_loud_and_leave_the_engine_usable(tracks_engine):
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.engine import _ptr
    eng = tracks_engine
    cand = ("b1", "a", "GATC", 1)
    b = eng.make_batch(engine_cands([cand]))
    n_rows = int(eng.track_windows("b1", 384)[-1])
    table = np.zeros((n_rows + 2, 6), np.uint32)
    launches = eng.stats()["launches"]

    def call(n=1, window=384, slots=b.slots, rows=(0, n_rows + 2)):
        slots, rows = np.asarray(slots, np.uint8), np.asarray(rows, np.uint64)
        return eng.lib.nm_motif_tracks_count(eng.ctx, n, _ptr(b.bins, C.c_uint32), _ptr(slots, C.c_uint8), _ptr(b.lens, C.c_uint8), _ptr(b.modpos, C.c_uint8),
                                             _ptr(b.offsets, C.c_uint32), _ptr(b.masks, C.c_uint8), window, _ptr(rows, C.c_uint64), _ptr(table, C.c_uint32))
    last = lambda: eng.lib.nm_last_error().decode()
    assert call(window=100) == NM_EINVAL and "window_bp" in last()
    assert call(window=0) == NM_EINVAL and "window_bp" in last()
    assert call(window=1 << 31) == NM_EINVAL and "window_bp" in last()
    assert call(slots=[5]) == NM_ESTATE and "slot 5" in last()          # nothing uploaded there
    assert call(rows=(0, n_rows - 1)) == NM_EINVAL and "row_offset" in last() and "candidate 0" in last()
    assert call(rows=(1, n_rows + 1)) == NM_EINVAL and "row_offset[0]" in last()
    assert call(n=0, rows=(0,)) == 0                                    # NM_OK
    with pytest.raises(ValueError):
        eng.motif_tracks(engine_cands([cand]), window=100)
    with pytest.raises(NmScanError) as e:                               # beyond the reach limit: nm_motif_sites' code
        list(eng.motif_tracks([(Motif("A" + "." * 100 + "T", 0), "a", "b1")], window=384))
    assert e.value.code == NM_ERANGE
    n = C.c_uint32(0)
    assert eng.lib.nm_tracks_windows(eng.ctx, 7, 128, None, 0, C.byref(n)) == NM_EINVAL and "bin" in last()
    short = np.zeros(2, np.uint64)
    assert eng.lib.nm_tracks_windows(eng.ctx, eng.bin_index["b1"], 128, _ptr(short, C.c_uint64), 1, C.byref(n)) == NM_ERANGE and n.value == 6
    assert not table.any() and eng.stats()["launches"] == launches      # a refused call has written nothing and reached no kernel
    assert call() == 0
    names, prefix, want = expected_table("b1", "GATC", 1, 384)
    assert np.array_equal(table[:n_rows], want) and not table[n_rows:].any()          # the rows beyond the bin's windows stay zero


# ------------------------------------------------------------------------------------------------ 5. the command
HEAD = "reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement\n"
COMMAND_BP, COMMAND_W, SPACING = 40_960, 1024, 256
ISLAND = (12_288, 20_480)


def command_input():
    """Three 40 960 bp contigs of one bin with GATC planted every 256 bp; every A of a planted GATC has a pileup row on both strands:
    ``plain`` all 1.0, ``chimera`` 1.0 below 20 480 and 0.0 from it on, ``island`` 0.0 inside [12 288, 20 480) and 1.0 outside.
    Returns (seqs, {name: [(position, strand, fraction)]})."""
    rng = np.random.default_rng(5)
    seqs, rows = {}, {}
    fraction = {"plain": lambda p: 1.0, "chimera": lambda p: 1.0 if p < 20_480 else 0.0, "island": lambda p: 0.0 if ISLAND[0] <= p < ISLAND[1] else 1.0}
    for name in ("plain", "chimera", "island"):
        s = list("".join(rng.choice(list("ACGT"), size=COMMAND_BP)))
        mine = []
        for q in range(100, COMMAND_BP, SPACING):
            s[q:q + 4] = "GATC"
            mine += [(q + 1, 0, fraction[name](q + 1)), (q + 2, 1, fraction[name](q + 2))]
        seqs[name], rows[name] = "".join(s), mine
    return seqs, rows


def test_the_command_input_is_decided_by_the_brute_force():
    """No GPU.  The planted tables segment as the test below expects, by the loop-by-loop gains."""
    seqs, rows = command_input()
    for name, seq in seqs.items():
        calls = ({(p, s) for p, s, f in rows[name] if f == 1.0}, {(p, s) for p, s, f in rows[name] if f == 0.0})
        t = tracks_of(seq, calls, "GATC", 1, COMMAND_W)
        assert len(t) == 40 and ((t[:, [0, 1, 3, 4]].sum(axis=1)) == 8).all()
        mod, nomod = (t[:, 0] + t[:, 3]).tolist(), (t[:, 1] + t[:, 4]).tolist()
        gains = gains_by_loops(mod, nomod, 20)
        best = max(gains, key=lambda k: (gains[k], -k))
        if name == "plain":
            assert max(gains.values()) == 0
        elif name == "chimera":
            assert best == 20 and gains[best] > 400
        else:
            assert best == 20 and gains[best] > 30 and [k for k in range(40) if nomod[k]] == list(range(12, 20))


@gpu
def test_command_on_planted_contigs(tmp_path):
    """``motif_tracks --window 1024 --tracks`` in a child process on a written assembly: ``plain`` is uniform, ``chimera`` a breakpoint at
    20 480 exactly (the junction sits on a window edge), ``island`` three segments with the planted bounds; counts and the background
    columns equal the brute force; the per-window file sums to the per-contig one."""
    seqs, rows = command_input()
    tmp = str(tmp_path)
    with open(tmp + "/assembly.fasta", "w") as f:
        for name, s in seqs.items():
            f.write(f">{name}\n" + "\n".join(s[k:k + 80] for k in range(0, len(s), 80)) + "\n")
    with open(tmp + "/contig_bin.tsv", "w") as f:
        f.write("".join(f"{name}\tbinA\n" for name in seqs))
    with open(tmp + "/pileup.bed", "w") as f:
        for name in seqs:
            for p, s, frac in rows[name]:
                nmod = 20 if frac == 1.0 else 0
                f.write(f"{name}\t{p}\t{p + 1}\ta\t20\t{'+-'[s]}\t{p}\t{p + 1}\t255,0,0\t20\t{100 * frac:.2f}\t{nmod}\t{20 - nmod}\t0\t0\t0\t0\t0\n")
    with open(tmp + "/bin-motifs.tsv", "w") as f:
        f.write(HEAD + "binA\tGATC\t1\ta\t1\t1\tpalindrome\t\t\t\t\n")
    _run(tmp, "motif_tracks", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "bin-motifs.tsv", "--out", "tr", "--window", str(COMMAND_W),
                               "--tracks"])
    from nanomotif_amd.motif_tracks import CONTIGS_HEADER, SEGMENTS_HEADER, TRACKS_HEADER
    head, contigs = _body(tmp + "/tr/motif-tracks-contigs.tsv")
    assert head == CONTIGS_HEADER and [r[:5] for r in contigs] == [["binA", n, "GATC", "a", "1"] for n in seqs]
    head, segments = _body(tmp + "/tr/motif-tracks-segments.tsv")
    assert head == SEGMENTS_HEADER
    head, windows = _body(tmp + "/tr/motif-tracks.tsv")
    assert head == TRACKS_HEADER
    assert os.path.exists(tmp + "/tr/args.motif_tracks.json") and os.path.exists(tmp + "/tr/logs/timings.motif_tracks.json")
    col = {h: i for i, h in enumerate(CONTIGS_HEADER)}
    want_bounds = {"plain": [0, COMMAND_BP], "chimera": [0, 20_480, COMMAND_BP], "island": [0, ISLAND[0], ISLAND[1], COMMAND_BP]}
    want_flag = {"plain": "uniform", "chimera": "breakpoint", "island": "islands"}
    for row in contigs:
        name = row[1]
        print("\t".join(row))
        calls = ({(p, s) for p, s, f in rows[name] if f == 1.0}, {(p, s) for p, s, f in rows[name] if f == 0.0})
        t = tracks_of(seqs[name], calls, "GATC", 1, COMMAND_W)
        bg = tracks_of(seqs[name], calls, "A", 0, COMMAND_W)
        three = (t[:, :3] + t[:, 3:]).sum(axis=0).tolist()
        assert row[col["length"]] == str(COMMAND_BP) and row[col["n_windows"]] == "40" and [int(x) for x in row[col["n_mod"]:col["n_mod"] + 3]] == three
        assert row[col["flag"]] == want_flag[name] and int(row[col["n_segments"]]) == len(want_bounds[name]) - 1
        if name == "plain":
            assert row[col["frac_mod"]] == "1.000000" and row[col["best_gain"]] == "0.000"
        if name == "chimera":
            assert row[col["best_split"]] == "20480" and row[col["frac_left"]] == "1.000000" and row[col["frac_right"]] == "0.000000"
            assert row[col["best_gain"]] == "%.3f" % (2 * 320 * np.log(2))
        mine = [r for r in segments if r[1] == name]
        assert [(int(r[6]), int(r[7])) for r in mine] == list(zip(want_bounds[name][:-1], want_bounds[name][1:])), (name, mine)
        assert [int(r[5]) for r in mine] == list(range(len(mine)))
        for r in mine:
            a, b = int(r[6]) // COMMAND_W, -(-int(r[7]) // COMMAND_W)
            seg, seg_bg = t[a:b].sum(axis=0), bg[a:b].sum(axis=0)
            assert [int(x) for x in r[8:11]] == [int(seg[0] + seg[3]), int(seg[1] + seg[4]), int(seg[2] + seg[5])], r
            assert [int(x) for x in r[12:14]] == [int(seg_bg[0] + seg_bg[3]), int(seg_bg[1] + seg_bg[4])] and int(r[12]) + int(r[13]) > 0, r
            assert r[14] == "%.6f" % (int(r[12]) / (int(r[12]) + int(r[13])))
        # the per-window file: the non-empty windows of the brute force, summing to the per-contig row
        per_window = [r for r in windows if r[0] == name]
        assert [[int(x) for x in r[7:13]] for r in per_window] == [x for x in t.tolist() if any(x)]
        assert [(int(r[1]), int(r[2])) for r in per_window] == [(k * COMMAND_W, (k + 1) * COMMAND_W) for k in range(40) if t[k].any()]
        sums = np.array([[int(x) for x in r[7:13]] for r in per_window]).sum(axis=0)
        assert [int(sums[0] + sums[3]), int(sums[1] + sums[4]), int(sums[2] + sums[5])] == three
    assert n_windows(COMMAND_BP, COMMAND_W) == 40
