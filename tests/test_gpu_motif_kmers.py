"""GPU: the methylation of every k-mer context of a bin (nm_kmer_methylation, ``ScanEngine.kmer_methylation``, ``nanomotif motif_kmers``)
against the brute force of ``test_motif_kmers_host`` (strings, slices and a dict of calls).  Counts are integers: every comparison is an
equality over the WHOLE table of every request.  The conditions on the input (``test_motif_kmers_host.test_the_input_is_not_degenerate``)
need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from nanomotif_amd import synth
from nanomotif_amd.motif import Motif
from test_gpu_motif_compare import _filtered_piles, _run
from test_gpu_motif_profile import HEAD
from test_motif_kmers_host import CANONICAL, COMP, SHAPES, SLOTS, all_requests, brute, expected, expected_all, kmer_input, offsets_of

gpu = pytest.mark.gpu
SWITCHES = [{}, {"NM_KMER_GLOBAL_ATOMICS": "1"}, {"NM_KMER_RUN_CHUNKS": "1"}, {"NM_KMER_RUN_CHUNKS": "3"}]


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


def loaded(engine_cls, names, seqs, bins, bin_names, rows):
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names], bin_names=bin_names)
    for mt in SLOTS:
        eng.upload_pileup(mt, *rows[mt])
    return eng


@pytest.fixture(scope="module")
def kmer_engine(engine_cls):
    names, seqs, bins, bin_names, rows, _ = kmer_input()
    eng = loaded(engine_cls, names, seqs, bins, bin_names, rows)
    assert eng.slot_of_mod == {"a": 0, "m": 1, "21839": 2}
    yield eng
    eng.close()


class switched:
    """The environment switches of one call (read per call by the library)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        assert not any(k in os.environ for k in ("NM_KMER_GLOBAL_ATOMICS", "NM_KMER_RUN_CHUNKS"))
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            del os.environ[k]


# ------------------------------------------------------------------------------------------------ 1. a literal case
@gpu
def test_literal_case_by_hand(engine_cls):
    """GATCGATC under classification "a": (1, +) 0.9, (2, -) 0.1, (5, +) 0.95.  The A's at 1 and 5 are '+' sites, both mod; the T's at 2
    and 6 are '-' sites, nomod and without a call.  N*N: every '+' site reads G before and T behind; a '-' site reads the complement of
    the next letter (C -> G) before and of the previous one (A -> T) behind: all four sites fall into row GT = 2 * 4 + 3.  NN*: the site
    at 1 probes position -1 and the '-' site at 6 position 8: incomplete; the other two read C, G = row 6."""
    eng = engine_cls()
    eng.upload_assembly(["c"], ["GATCGATC"], ["b"])
    eng.upload_pileup("a", [0, 0, 0], [1, 2, 5], np.frombuffer(b"+-+", np.uint8), [0.9, 0.1, 0.95])
    zero = [0, 0, 0]
    totals, table = eng.kmer_methylation([("a", "b")], "N*N")
    assert totals.tolist() == [[[2, 0, 0], [0, 1, 1]]] and table.shape == (1, 16, 3) and totals.dtype == table.dtype == np.int64
    assert table[0].tolist() == [zero] * 11 + [[2, 1, 1]] + [zero] * 4
    totals, table = eng.kmer_methylation([("a", "b")], "*")
    assert totals.tolist() == [[[2, 0, 0], [0, 1, 1]]] and table.tolist() == [[[2, 1, 1]]]
    totals, table = eng.kmer_methylation([("a", "b")], "NN*")
    assert totals.tolist() == [[[2, 0, 0], [0, 1, 1]]] and table[0].tolist() == [zero] * 6 + [[1, 1, 0]] + [zero] * 9
    totals, table = eng.kmer_methylation([], "N*N")
    assert totals.shape == (0, 2, 3) and table.shape == (0, 16, 3) and totals.dtype == table.dtype == np.int64
    off = np.array([-1, 1], np.int8)
    assert eng.lib.nm_kmer_methylation(eng.ctx, 0, None, None, 2, off.ctypes.data_as(C.POINTER(C.c_int8)), None, None) == 0
    assert eng.lib.nm_kmer_methylation(eng.ctx, 0, None, None, 0, None, None, None) == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. geometry
@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_every_request_equals_the_brute_force(kmer_engine, shape):
    """Every request (all bins x the slots a, m, 21839) of the host file's input: sites and probes across word, lane and chunk borders, an
    N run across a chunk border, contigs shorter than the shape, windows that leave a contig at either end, a homopolymer (one hot cell)
    and the empty bin — under both reductions and with runs of 1 and of 3 chunks, which end inside a contig, at a contig border and at a
    bin's last chunk.  All of them equal the brute force, hence each other."""
    eng = kmer_engine
    requests = all_requests()
    want_totals, want_table = expected_all(shape)
    for env in SWITCHES:
        with switched(env):
            before = eng.stats()["launches"]
            totals, table = eng.kmer_methylation(requests, shape, max_bytes=1 << 40)
            assert eng.stats()["launches"] - before == 1, env           # one launch per library call, whatever it holds
        assert table.shape == (len(requests), 4 ** len(offsets_of(shape)), 3)
        assert np.array_equal(totals, want_totals), (env, np.argwhere(totals != want_totals)[:5].tolist())
        assert np.array_equal(table, want_table), (env, np.argwhere(table != want_table)[:5].tolist())
        # totals - table.sum = the incomplete sites of the brute force
        assert np.array_equal(totals.sum(axis=1) - table.sum(axis=1), want_totals.sum(axis=1) - want_table.sum(axis=1))


@gpu
def test_request_lists_and_the_byte_budget(kmer_engine):
    eng = kmer_engine
    shape = "NNN*NNN"
    requests = all_requests()
    totals, table = expected_all(shape)
    for order in (list(range(len(requests)))[::-1], [4, 4, 0, 7, 4, 9, 0], [3, 0, 6, 1, 9, 2, 11, 5]):      # reversed, duplicated, interleaved
        t, tab = eng.kmer_methylation([requests[k] for k in order], shape)
        assert np.array_equal(t, totals[order]) and np.array_equal(tab, table[order]), order
    # a request of the empty bin alone (nothing to launch) and between two others; slots by number, bins by id
    before = eng.stats()["launches"]
    t, tab = eng.kmer_methylation([("a", "b0_empty")], shape)
    assert not t.any() and not tab.any() and eng.stats()["launches"] == before
    three = [("m", "b2"), ("a", "b0_empty"), ("a", "b1")]
    t, tab = eng.kmer_methylation(three, shape)
    assert not t[1].any() and not tab[1].any()
    for k in (0, 2):
        assert np.array_equal(t[k], expected(shape, *three[k])[0]) and np.array_equal(tab[k], expected(shape, *three[k])[1])
    t, tab = eng.kmer_methylation([(1, 2), (0, 0), (0, 1)], offsets_of(shape))
    assert np.array_equal(t[0], expected(shape, "m", "b2")[0]) and np.array_equal(tab[2], expected(shape, "a", "b1")[1])
    # the byte budget cuts the list into library calls (one launch each) and changes nothing
    row_bytes = 24 * 4 ** 6 + 48
    for max_bytes, groups in ((1, [(k, k + 1) for k in range(12)]), (2 * row_bytes, [(k, k + 2) for k in range(0, 12, 2)]),
                              (5 * row_bytes, [(0, 5), (5, 10), (10, 12)])):
        before = eng.stats()["launches"]
        t, tab = eng.kmer_methylation(requests, shape, max_bytes=max_bytes)
        launched = eng.stats()["launches"] - before
        assert np.array_equal(t, totals) and np.array_equal(tab, table)
        # (a call that holds only requests of the empty bin launches nothing)
        assert launched == sum(any(b != "b0_empty" for _, b in requests[k:e]) for k, e in groups), (max_bytes, launched)


# ------------------------------------------------------------------------------------------------ 3. identities
@gpu
def test_identities_on_the_device_results(kmer_engine, engine_cls):
    """(a) ``totals`` is ``motif_site_counts`` of the one-letter motif; (b) a row is the strand sum of ``motif_site_counts`` of
    ``kmer_motif`` — candidates through another kernel: every non-empty row at F = 3, 64 seeded rows at F = 6 and at the gapped shape;
    (c) reverse-complementing the assembly and mirroring the calls on a second engine leaves ``table`` and exchanges the strands of
    ``totals``."""
    from nanomotif_amd.engine import kmer_motif
    eng = kmer_engine
    requests = [r for r in all_requests() if r[1] != "b0_empty"]
    totals, _ = eng.kmer_methylation(requests, "*")
    own = eng.motif_site_counts([(Motif(CANONICAL[mt], 0), mt, b) for mt, b in requests])
    for k, (_, six) in enumerate(own):
        assert six.sum() > 0 and np.array_equal(totals[k], six.sum(axis=0).reshape(2, 3)), requests[k]
    rng = np.random.default_rng(7)
    some = [("a", "b1"), ("m", "b1"), ("21839", "b3"), ("a", "b2")]
    for shape in ("N*NN", "NNN*NNN", "NNN*......NNN"):
        _, table = eng.kmer_methylation(some, shape)
        cands, cells = [], []
        for k, (mt, b) in enumerate(some):
            filled = np.nonzero(table[k].sum(axis=1))[0]
            rows = filled if shape == "N*NN" else rng.choice(filled, size=min(64, len(filled)), replace=False)
            assert len(rows) >= (40 if shape == "N*NN" and b != "b2" else 1)
            cands += [(kmer_motif(shape, CANONICAL[mt], int(r)), mt, b) for r in rows]
            cells += [(k, int(r)) for r in rows]
        counts = eng.motif_site_counts(cands)
        for (k, r), (_, six) in zip(cells, counts):
            assert np.array_equal(six.sum(axis=0).reshape(2, 3).sum(axis=0), table[k, r]), (shape, some[k], r)
    # (c) the mirrored input on a second engine
    names, seqs, bins, bin_names, rows, _ = kmer_input()
    length = np.array([len(seqs[n]) for n in names], dtype=np.int64)
    m_seqs = {n: s.translate(COMP)[::-1] for n, s in seqs.items()}
    m_rows = {}
    for mt, (cid, pos, st, fr) in rows.items():
        m_pos = length[cid.astype(np.int64)] - 1 - pos
        o = np.lexsort((m_pos, cid))                                      # (by contig, then position, as a pileup comes)
        m_rows[mt] = (cid[o], m_pos[o], np.where(st == ord("+"), ord("-"), ord("+")).astype(np.uint8)[o], fr[o])
    mirror = loaded(engine_cls, names, m_seqs, bins, bin_names, m_rows)
    try:
        for shape in ("NN*NNN", "NNN*......NNN", "*" + "." * 30 + "N"):
            t, tab = eng.kmer_methylation(requests, shape)
            t_m, tab_m = mirror.kmer_methylation(requests, shape)
            assert np.array_equal(tab_m, tab) and np.array_equal(t_m, t[:, ::-1]) and not np.array_equal(t_m, t), shape
    finally:
        mirror.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
@gpu
def test_errors_are_loud_and_leave_the_engine_usable(kmer_engine, engine_cls):
    from nanomotif_amd._lib import NmScanError
    eng = kmer_engine
    shape = "N*NN"
    totals, table = np.zeros((2, 2, 3), np.uint64), np.zeros((2, 64, 3), np.uint64)
    q = lambda a, t: a.ctypes.data_as(C.POINTER(t))

    def call(bins=(1, 2), slots=(0, 1), offsets=offsets_of(shape)):
        b, s, off = np.asarray(bins, np.uint32), np.asarray(slots, np.uint8), np.asarray(offsets, np.int8)
        return eng.lib.nm_kmer_methylation(eng.ctx, len(b), q(b, C.c_uint32), q(s, C.c_uint8), len(off), q(off, C.c_int8), q(totals, C.c_uint64), q(table, C.c_uint64))
    last = lambda: eng.lib.nm_last_error().decode()

    def valid():
        totals[:], table[:] = 0, 0
        assert call() == 0
        for k, (mt, b) in enumerate((("a", "b1"), ("m", "b2"))):
            assert np.array_equal(totals[k].astype(np.int64), expected(shape, mt, b)[0]) and np.array_equal(table[k].astype(np.int64), expected(shape, mt, b)[1])
        totals[:], table[:] = 0, 0
    for offsets, word in ((list(range(1, 12)), "n_offsets 11"), ([-1, 0, 1], "offsets[1]"), ([-32, 1, 2], "offsets[0]"), ([1, 2, 32], "offsets[2]"),
                          ([1, 1, 2], "offsets[1]"), ([-1, 2, 1], "offsets[2]")):
        assert call(offsets=offsets) == -1 and word in last(), (offsets, last())          # NM_EINVAL, the index named
        assert not totals.any() and not table.any()                                        # a refused call has written nothing
        valid()
    assert call(bins=(1, 4)) == -1 and "request 1" in last() and "req_bin 4" in last()
    valid()
    assert call(slots=(0, 5)) == -3 and "req_mod_slot[1]" in last()                        # NM_ESTATE: nothing uploaded there
    valid()
    assert call(slots=(200, 0)) == -3 and "req_mod_slot[0]" in last()
    assert call(bins=(9, 2), slots=(7, 0)) == -1 and "request 0" in last() and "req_bin" in last()      # wrong in both: refused for the bin
    assert call(bins=(1, 9), slots=(7, 0)) == -3 and "req_mod_slot[0]" in last()           # (requests are checked in order)
    valid()
    for bad, code in (([("a", 4)], -1), ([(5, "b1")], -3)):
        with pytest.raises(NmScanError) as e:
            eng.kmer_methylation(bad, shape)
        assert e.value.code == code
    with pytest.raises(ValueError):
        eng.kmer_methylation([("a", "b1")], "NNN")
    valid()
    fresh = engine_cls()                                                                   # no assembly uploaded
    try:
        with pytest.raises(NmScanError) as e:
            fresh.kmer_methylation([(0, 0)], shape)
        assert e.value.code == -3 and "nm_upload_contigs" in str(e.value)
        fresh.upload_assembly(["c"], ["GATCGATC"], ["b"])
        fresh.upload_pileup("a", [0], [1], np.frombuffer(b"+", np.uint8), [0.9])
        assert fresh.kmer_methylation([("a", "b")], "*")[1].tolist() == [[[1, 0, 3]]]
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 5. the command
COMMAND_SPEC = synth.SynthSpec(n_contigs=4, total_bp=200_000, n_bins=2, mod_types=("a", "m"), seed=61, min_contig_bp=30_000,
                               fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m")))
COMMAND_SHAPE = "N*NN"


def expected_files(mg, shape, motifs):
    """The files' text: the brute force over the pre-filtered pileup, through the module's own formatter."""
    from nanomotif_amd.motif_kmers import format_files
    from nanomotif_amd.motif_sites import SiteCandidate
    from nanomotif_amd.pileup import MOD_TYPES
    piles = _filtered_piles(mg)
    seqs = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    kept = [mt for mt in MOD_TYPES if piles[mt]]                          # slot order
    calls = {mt: {(n, int(p), 0 if s == ord("+") else 1): float(f) for n, pile in piles[mt].items()
                  for p, s, f in zip(pile.position, pile.strand, pile.fraction_mod)} for mt in kept}
    bins = sorted(set(mg.bin_names))
    requests = [(b, mt) for b in bins for mt in kept]
    both = [brute([(n, seqs[n]) for i, n in enumerate(mg.names) if mg.bin_names[i] == b], calls[mt], CANONICAL[mt], offsets_of(shape)) for b, mt in requests]
    cands = None if motifs is None else [SiteCandidate(*m) for m in motifs]
    return format_files(requests, [t for t, _ in both], [t for _, t in both], shape, cands), kept


@gpu
def test_command_on_a_synthetic_metagenome(tmp_path):
    """motif_kmers --shape N*NN from files, each run a child process: without --bin_motifs two files; with a bin-motifs.tsv that lacks the
    planted GATC the four files equal the text derived from the brute force, byte for byte, and GATC is in kmer-unexplained.tsv for both
    bins; once GATC is listed it is not."""
    from nanomotif_amd.motif_kmers import BINS_NAME, MAIN_NAME, OVERCALLED_NAME, UNEXPLAINED_NAME
    mg = synth.make_metagenome(COMMAND_SPEC)
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    mg.write_bed(tmp + "/pileup.bed")
    bins = sorted(set(mg.bin_names))
    row = lambda b, motif, pos, mt: f"{b}\t{motif}\t{pos}\t{mt}\t1\t1\tpalindrome\t\t\t\t\n"
    open(tmp + "/without.tsv", "w").write(HEAD + "".join(row(b, "CCWGG", 1, "m") for b in bins))
    open(tmp + "/gatc.tsv", "w").write(HEAD + "".join(row(b, "GATC", 1, "a") for b in bins))
    files = (MAIN_NAME, BINS_NAME, UNEXPLAINED_NAME, OVERCALLED_NAME)
    common = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--shape", COMMAND_SHAPE]
    read = lambda out, name: open(f"{tmp}/{out}/{name}").read()

    _run(tmp, "motif_kmers", common + ["--out", "plain"])
    want, kept = expected_files(mg, COMMAND_SHAPE, None)
    assert kept == ["m", "a"] or kept == ["a", "m"]
    assert [read("plain", n) for n in files[:2]] == list(want) and not os.path.exists(f"{tmp}/plain/{files[2]}")
    assert os.path.exists(f"{tmp}/plain/logs/timings.motif_kmers.json")

    _run(tmp, "motif_kmers", common + ["--out", "miss", "--bin_motifs", "without.tsv"])
    want, _ = expected_files(mg, COMMAND_SHAPE, [(b, "CCWGG", "m", 1) for b in bins])
    assert [read("miss", n) for n in files] == list(want)
    missed = [line.split("\t") for line in read("miss", UNEXPLAINED_NAME).split("\n")[1:-1]]
    assert {(r[0], r[1], r[2]) for r in missed} >= {(b, "a", "GATC") for b in bins}

    _run(tmp, "motif_kmers", common + ["--out", "found", "--bin_motifs", "without.tsv", "gatc.tsv"])
    want, _ = expected_files(mg, COMMAND_SHAPE, [(b, "CCWGG", "m", 1) for b in bins] + [(b, "GATC", "a", 1) for b in bins])
    assert [read("found", n) for n in files] == list(want)
    found = [line.split("\t") for line in read("found", UNEXPLAINED_NAME).split("\n")[1:-1]]
    assert not any(r[2] == "GATC" for r in found)
    main = [line.split("\t") for line in read("found", MAIN_NAME).split("\n")[1:-1]]
    assert {r[8] for r in main if r[1] == "a" and r[2] == "GATC"} == {"GATC_a_1"}
