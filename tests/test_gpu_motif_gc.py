"""GPU: motif methylation by local GC content (nm_motif_gc_count, ``ScanEngine.motif_gc``, ``nanomotif motif_gc``) against the brute force
of ``test_motif_gc_host`` (plain Python over dense per-position arrays, nothing shared with the engine).  Counts are integers: every
comparison is an equality over the WHOLE table of every candidate.  The conditions on the inputs
(``test_motif_gc_host.test_the_input_is_not_degenerate``, ``test_the_planted_input_yields_its_flags_with_twice_the_margin``) need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from nanomotif_amd.motif import Motif
from test_gpu_motif_compare import _body, _run
from test_gpu_motif_profile import HEAD
from test_motif_gc_host import (CLEAN_BIN, HALVES, HAND, HAND_ROWS, HAND_SEQ, NOISE_BIN, PLANTED_CANDS, PLANTED_HALF, expected_files, gc_cands, gc_contigs, gc_input,
                                gc_tables, planted_expected, planted_metagenome)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


@pytest.fixture(scope="module")
def gc_engine(engine_cls):
    names, seqs, bins, bin_names, rows, _ = gc_input()
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names], bin_names=bin_names)
    for mt in ("a", "m"):
        eng.upload_pileup(mt, *rows[mt])
    yield eng
    eng.close()


def engine_cands(cands):
    return [(Motif(m, i), mt, b) for b, mt, m, i in cands]


# ------------------------------------------------------------------------------------------------ 1. a literal case
@gpu
def test_literal_case_by_hand(engine_cls):
    """GGATCNTGATCCGATC, GATC @ 1, half 2: ``test_motif_gc_host.HAND`` with the reasons beside every row."""
    eng = engine_cls()
    eng.upload_assembly(["c"], [HAND_SEQ], ["b"])
    p, s, f = zip(*HAND_ROWS)
    eng.upload_pileup("a", [0] * len(p), list(p), np.frombuffer("".join(s).encode(), np.uint8), list(f))
    got = list(eng.motif_gc([(Motif("GATC", 1), "a", "b")], half=2))
    assert len(got) == 1 and got[0][0] == ["c"] and got[0][1].dtype == np.int64 and got[0][1].shape == (1, 2, 3, 7)
    assert got[0][1][0].tolist() == HAND
    t0 = list(eng.motif_gc([(Motif("GATC", 1), "a", "b")], half=0))[0][1][0]
    assert t0[..., 0].tolist() == [[1, 1, 1], [2, 1, 0]] and not t0[..., 1:].any()
    assert list(eng.motif_gc([], half=2)) == []
    rows = np.zeros(1, np.uint64)
    assert eng.lib.nm_motif_gc_count(eng.ctx, 0, None, None, None, None, None, None, 2, rows.ctypes.data_as(C.POINTER(C.c_uint64)), None) == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. geometry
@gpu
@pytest.mark.parametrize("half", HALVES)
def test_windows_that_break_naive_sums(gc_engine, half):
    """Every candidate of the host file's input — G = 1, 2, 3; sites on bit 0 and bit 31, on a lane's first and last word, either side of
    a chunk border with the window across it; windows that start and stop to fit at both ends of a contig of three chunks; an N first,
    last, one before and one behind the window; a contig shorter than the window; GC-only beside AT-only contigs; three bins and two mod
    types interleaved, the one-letter backgrounds among them — equals the brute force, whole tables."""
    eng = gc_engine
    cands, exp, contigs = gc_cands(), gc_tables(half), gc_contigs()
    before = eng.stats()["launches"]
    got = list(eng.motif_gc(engine_cands(cands), half=half))
    assert eng.stats()["launches"] - before == 3                          # one launch per width, whatever the window
    assert len(got) == len(cands)
    for c, (names, t), want in zip(cands, got, exp):
        assert names == [n for n, _ in contigs[c[0]]] and t.shape == want.shape == (len(names), 2, 3, 2 * half + 3)
        assert np.array_equal(t, want), (half, c, np.argwhere(t != want)[:5].tolist())
    if half == 0:                                                         # g is the modified base itself: 0 for every 6mA site, 1 for every 5mC site
        for c, (_, t) in zip(cands, got):
            assert t[..., 2].sum() == 0 and t[..., 1 if c[1] == "a" else 0].sum() == 0 and t.sum() == t[..., 0 if c[1] == "a" else 1].sum()
    # a second call gives the same table (no stale counters on chip or in the table)
    again = list(eng.motif_gc(engine_cands(cands), half=half))
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(got, again))
    if half != 16:
        return
    # a candidate in the bin without a contig gives no rows, also between two others in the same call
    three = [("b0_empty", "a", "GATC", 1), ("b2", "m", "C", 0), ("b0_empty", "a", "A", 0), ("b1", "a", "A" + "." * 70 + "T", 0)]
    g3 = list(eng.motif_gc(engine_cands(three), half=half))
    assert g3[0][0] == [] and g3[0][1].shape == (0, 2, 3, 2 * half + 3) and g3[2][1].shape[0] == 0
    for k in (1, 3):
        assert np.array_equal(g3[k][1], exp[cands.index(three[k])])
    assert list(eng.motif_gc(engine_cands(three[:1]), half=half))[0][1].shape[0] == 0
    # reversed and duplicated candidate lists give the permuted tables
    rev = list(eng.motif_gc(engine_cands(cands[::-1]), half=half))
    assert all(np.array_equal(r[1], want) for r, want in zip(rev, exp[::-1]))
    order = [4, 4, 0, 26, 4, 9, 0]
    dup = list(eng.motif_gc(engine_cands([cands[k] for k in order]), half=half))
    assert all(np.array_equal(d[1], exp[k]) for d, k in zip(dup, order))


# ------------------------------------------------------------------------------------------------ 3. identities
@gpu
def test_identities_on_the_device_results(gc_engine):
    """(a) summed over g and edge a row is ``motif_site_counts``; (b) the result does not depend on ``max_bytes``: one group, and a limit
    that forces one candidate per group."""
    eng = gc_engine
    cands = gc_cands()
    ecands = engine_cands(cands)
    own = eng.motif_site_counts(ecands)
    for half in (1, 31):
        got = list(eng.motif_gc(ecands, half=half))
        for c, (names, t), (names6, six) in zip(cands, got, own):
            assert names == names6 and np.array_equal(t.sum(axis=-1).reshape(len(names), 6), six), (half, c)
        before = eng.stats()["launches"]
        single = list(eng.motif_gc(ecands, half=half, max_bytes=1))
        assert eng.stats()["launches"] - before == len(cands)             # one candidate per group: one launch each
        whole = list(eng.motif_gc(ecands, half=half, max_bytes=1 << 40))
        for a, b, c in zip(got, single, whole):
            assert a[0] == b[0] == c[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
    assert sum(int(six.sum()) for _, six in own) > 25_000                # (the two backgrounds alone are a site per position)


# ------------------------------------------------------------------------------------------------ 4. refusals
@gpu
def test_errors_are_loud_and_leave_the_engine_usable(gc_engine, engine_cls):
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.engine import _ptr
    eng = gc_engine
    cands = gc_cands()
    k = cands.index(("b1", "a", "GATC", 1))
    want = gc_tables(31)[k]
    b = eng.make_batch(engine_cands([cands[k]]))
    far = eng.make_batch([(Motif("A" + "." * 100 + "T", 0), "a", "b1")])   # beyond the reach limit
    n_rows = want.shape[0]
    counts = np.zeros((n_rows, 2, 3, 65), np.int64)

    def call(e=eng, bins=b.bins, slots=b.slots, half=31, rows=(0, n_rows), batch=b, nulls=()):
        slots, bins, rows = np.asarray(slots, np.uint8), np.asarray(bins, np.uint32), np.asarray(rows, np.uint64)
        args = [_ptr(bins, C.c_uint32), _ptr(slots, C.c_uint8), _ptr(batch.lens, C.c_uint8), _ptr(batch.modpos, C.c_uint8), _ptr(batch.offsets, C.c_uint32),
                _ptr(batch.masks, C.c_uint8), half, _ptr(rows, C.c_uint64), _ptr(counts, C.c_int64)]
        for j in nulls:
            args[j] = None
        return e.lib.nm_motif_gc_count(e.ctx, 1, *args)
    last = lambda: eng.lib.nm_last_error().decode()

    def fine():
        counts[:] = -1
        assert call() == 0 and np.array_equal(counts, want)
    fine()
    counts[:] = 0
    assert call(half=32) == -1 and "half" in last()                       # NM_EINVAL
    fine()
    counts[:] = 0
    for j in (0, 1, 2, 3, 4, 5, 7, 8):
        assert call(nulls=(j,)) == -1 and "NULL" in last(), j
    fine()
    counts[:] = 0
    assert call(bins=[7]) == -1 and "cand_bin" in last() and "candidate 0" in last()
    fine()
    counts[:] = 0
    assert call(slots=[5]) == -3 and "cand_mod_slot[0]" in last()         # NM_ESTATE: nothing uploaded there
    assert call(slots=[200]) == -3 and "cand_mod_slot[0]" in last()
    fine()
    counts[:] = 0
    assert call(batch=far) == -5                                          # NM_ERANGE: nm_motif_sites' code
    assert call(rows=(0, n_rows - 1)) == -1 and "row_offset" in last()
    fine()
    counts[:] = 0
    # a candidate wrong in two ways is refused in the shared order: bin, slot, program, rows
    assert call(bins=[7], slots=[5]) == -1 and "cand_bin" in last()
    assert call(slots=[5], batch=far) == -3 and "cand_mod_slot[0]" in last()
    assert call(batch=far, rows=(0, 0)) == -5
    assert call(half=32, bins=[7]) == -1 and "half" in last()
    assert not counts.any()                                               # a refused call has written nothing
    fine()
    with pytest.raises(ValueError):
        list(eng.motif_gc(engine_cands([cands[k]]), half=32))
    with pytest.raises(NmScanError) as e:
        list(eng.motif_gc([(Motif("A" + "." * 100 + "T", 0), "a", "b1")]))
    assert e.value.code == -5
    # no upload
    bare = engine_cls()
    counts[:] = 0
    assert call(e=bare) == -3 and "nm_upload_contigs" in bare.lib.nm_last_error().decode() and not counts.any()
    bare.close()
    fine()


# ------------------------------------------------------------------------------------------------ 5. the command
def _bin_motifs_text(cands):
    return HEAD + "".join(f"{b}\t{m}\t{p}\t{mt}\t1\t1\tpalindrome\t\t\t\t\n" for b, m, mt, p in cands)


@gpu
def test_command_on_a_synthetic_metagenome(tmp_path):
    """motif_gc on the planted input of the host file (a bin whose 5mC calls follow the local GC with the generic GCGC listed for it,
    a true GATC beside it, a clean bin, and a row of a mod type the pileup does not hold), in a child process: the four files equal the
    text derived from the brute force over the pre-filtered pileup; the noise motif is flagged ``gc_dependent``, the true one ``none``;
    another window and more buckets than it has values run and agree as well."""
    from nanomotif_amd.motif_gc import BINS_HEADER, CONTIGS_HEADER, MAIN_HEADER, SUMMARY_HEADER
    mg = planted_metagenome()
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    mg.write_bed(tmp + "/pileup.bed")
    open(tmp + "/motifs.tsv", "w").write(_bin_motifs_text(PLANTED_CANDS[:3]))
    open(tmp + "/more.tsv", "w").write(_bin_motifs_text(PLANTED_CANDS[2:]))  # the third row again: a repeat is dropped
    want, targets = planted_expected()
    base = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "motifs.tsv", "more.tsv"]
    r = _run(tmp, "motif_gc", base + ["--out", "gc"])
    assert "the pileup holds no rows of mod type 21839" in r.stdout + r.stderr and "skipped" in r.stdout + r.stderr
    names = ("motif-gc.tsv", "motif-gc-bins.tsv", "motif-gc-contigs.tsv", "motif-gc-summary.tsv")
    for name, header, rows in zip(names, (MAIN_HEADER, BINS_HEADER, CONTIGS_HEADER, SUMMARY_HEADER), want):
        head, body = _body(f"{tmp}/gc/{name}")
        if name == names[3]:
            for row in body:
                print("\t".join(row))
        assert head == header == rows[0] and body == rows[1:], name
    assert os.path.exists(f"{tmp}/gc/args.motif_gc.json") and os.path.exists(f"{tmp}/gc/logs/timings.motif_gc.json")
    flags = {tuple(r[:4]): r[-1] for r in _body(f"{tmp}/gc/motif-gc-summary.tsv")[1]}
    assert flags == {(NOISE_BIN, "GCGC", "m", "1"): "gc_dependent", (NOISE_BIN, "GATC", "a", "1"): "none", (CLEAN_BIN, "GATC", "a", "1"): "none",
                     (CLEAN_BIN, "CCWGG", "m", "1"): "none"}
    assert PLANTED_HALF == 31
    # half 1 with 64 buckets asked for: four values of g, four buckets
    _run(tmp, "motif_gc", base + ["--out", "gc1", "--half", "1", "--gc_bins", "64", "--min_called", "50", "--min_z", "3", "--min_delta", "0.05"])
    want1, _ = expected_files(mg, PLANTED_CANDS, 1, bins=64, min_called=50, min_z=3.0, min_delta=0.05)
    for name, rows in zip(names, want1):
        head, body = _body(f"{tmp}/gc1/{name}")
        assert head == rows[0] and body == rows[1:], name
    assert len(want1[0]) - 1 == 4 * 4
