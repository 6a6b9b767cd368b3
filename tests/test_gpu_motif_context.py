"""GPU: the sequence context of motif sites by methylation state (nm_motif_context_count, ``ScanEngine.motif_context``, ``nanomotif
motif_context``) against the brute force of ``test_motif_context_host`` (built only from ``occurrences`` / ``probe_class`` of
``test_motif_profile_host`` and string indexing).  Counts are integers: every comparison is an equality over the WHOLE table of every
candidate.  The conditions on the input (``test_motif_context_host.test_the_input_is_not_degenerate``) need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from nanomotif_amd import synth
from nanomotif_amd.motif import Motif
from test_gpu_motif_compare import _body, _filtered_piles, _run
from test_gpu_motif_profile import HEAD, candidates_of_texts
from test_gpu_motif_strands import _rows
from test_motif_context_host import LETTERS, REFINEMENTS, context_expected, context_of, middle, narrowed
from test_motif_profile_host import CANONICAL, TARGETS, Classes, profile_cands, profile_input

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


@pytest.fixture(scope="module")
def context_engine(engine_cls):
    names, seqs, bins, bin_names, rows, _ = profile_input()
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names], bin_names=bin_names)
    for t in TARGETS:
        eng.upload_pileup(t, *rows[t])
    yield eng
    eng.close()


def engine_cands(cands):
    return [(Motif(m, i), mt, b) for b, mt, m, i in cands]


# ------------------------------------------------------------------------------------------------ 1. a literal case
Z = [0, 0, 0, 0, 0]
HAND = [[[[0, 1, 0, 0, 1], Z, Z], [Z, [0, 1, 0, 0, 0], [0, 0, 0, 0, 1]]],        # o = -2: '+' sites probe -1 (outside) and 3 (C); '-' sites 4 (G, read C) and 8 (outside)
        [[[0, 0, 2, 0, 0], Z, Z], [Z, [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]]],        # o = -1: the G before the A; '-' sites 3 and 7 (C, read G)
        [[[2, 0, 0, 0, 0], Z, Z], [Z, [1, 0, 0, 0, 0], [1, 0, 0, 0, 0]]],        # o = 0: the A itself; '-' sites sit on a T, read A
        [[[0, 0, 0, 2, 0], Z, Z], [Z, [0, 0, 0, 1, 0], [0, 0, 0, 1, 0]]],        # o = 1: the T; '-' sites 1 and 5 (A, read T)
        [[[0, 2, 0, 0, 0], Z, Z], [Z, [0, 1, 0, 0, 0], [0, 1, 0, 0, 0]]]]        # o = 2: the C; '-' sites 0 and 4 (G, read C)


@gpu
def test_literal_case_by_hand(engine_cls):
    """GATCGATC, GATC @ 1, radius 2: the motif occurs on '+' with its A at 1 and 5 and on '-' with its A at 2 and 6.  Classification "a":
    (1, +) 0.9, (2, -) 0.1, (5, +) 0.95: both '+' sites are mod, (2, -) is nomod, (6, -) has no call.  Layout [offset][occurrence
    strand][mod, nomod, nocall][A, C, G, T, other]."""
    eng = engine_cls()
    eng.upload_assembly(["c"], ["GATCGATC"], ["b"])
    eng.upload_pileup("a", [0, 0, 0], [1, 2, 5], np.frombuffer(b"+-+", np.uint8), [0.9, 0.1, 0.95])
    states, table = eng.motif_context([(Motif("GATC", 1), "a", "b")], radius=2)
    assert states.tolist() == [[[2, 0, 0], [0, 1, 1]]] and table.shape == (1, 5, 2, 3, 5)
    assert table[0].tolist() == HAND
    states, table = eng.motif_context([], radius=2)
    assert states.shape == (0, 2, 3) and table.shape == (0, 5, 2, 3, 5) and states.dtype == table.dtype == np.int64
    assert eng.lib.nm_motif_context_count(eng.ctx, 0, None, None, None, None, None, None, 2, None, None) == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. geometry
@gpu
@pytest.mark.parametrize("radius", [0, 1, 10, 31])
def test_layouts_and_offsets_that_break_naive_shifting(context_engine, radius):
    """Every candidate of the host file's input (G = 1, 2, 3; own base and probe across word, lane and chunk borders; an N run across a
    chunk border; contigs shorter than the motif; probes before the start and past the end of a contig): ``states`` and the whole table
    equal the brute force, under both reductions."""
    eng = context_engine
    cands, exp = profile_cands(), context_expected()
    states, table = eng.motif_context(engine_cands(cands), radius=radius)
    assert table.shape == (len(cands), 2 * radius + 1, 2, 3, 5)
    for k, c in enumerate(cands):
        want = middle(exp[k][1], radius)
        assert np.array_equal(states[k], exp[k][0]), (c, states[k].tolist(), exp[k][0].tolist())
        assert np.array_equal(table[k], want), (c, np.argwhere(table[k] != want)[:5].tolist())
    assert "NM_CONTEXT_WAVE_ATOMICS" not in os.environ
    os.environ["NM_CONTEXT_WAVE_ATOMICS"] = "1"
    try:
        s_w, t_w = eng.motif_context(engine_cands(cands), radius=radius)
    finally:
        del os.environ["NM_CONTEXT_WAVE_ATOMICS"]
    assert np.array_equal(s_w, states) and np.array_equal(t_w, table)
    if radius != 10:
        return
    # a candidate in the empty bin gives zeros, also between two others in the same call
    three = [("b0_empty", "a", "GATC", 1), ("b2", "a", "GATC", 1), ("b0_empty", "a", "A", 0), ("b1", "m", "C..GG", 0)]
    s3, t3 = eng.motif_context(engine_cands(three), radius=radius)
    assert not s3[0].any() and not t3[0].any() and not s3[2].any() and not t3[2].any()
    for k, c in ((1, three[1]), (3, three[3])):
        assert np.array_equal(s3[k], states[cands.index(c)]) and np.array_equal(t3[k], table[cands.index(c)])
    s1, t1 = eng.motif_context(engine_cands(three[:1]), radius=radius)
    assert not s1.any() and not t1.any()
    # reversed and duplicated candidate lists give the permuted table
    s_r, t_r = eng.motif_context(engine_cands(cands[::-1]), radius=radius)
    assert np.array_equal(s_r, states[::-1]) and np.array_equal(t_r, table[::-1])
    order = [4, 4, 0, 17, 4, 9, 0]
    s_d, t_d = eng.motif_context(engine_cands([cands[k] for k in order]), radius=radius)
    assert np.array_equal(s_d, states[order]) and np.array_equal(t_d, table[order])
    # one launch per width, whatever the radius
    before = eng.stats()["launches"]
    eng.motif_context(engine_cands(cands), radius=31)
    assert eng.stats()["launches"] - before == 3


# ------------------------------------------------------------------------------------------------ 3. identities
@gpu
def test_identities_on_the_device_results(context_engine):
    """(a) ``states`` is ``motif_site_counts``; (b) every row sums to ``states``; (c) the cell (o, X) is ``motif_site_counts`` of the
    motif narrowed to X at o — a candidate of another width through another kernel; (d) radius 10 is the middle of radius 31; (e) the
    reverse-complement candidate is the mirror (``test_motif_context_host.test_the_reverse_complement_candidate_is_the_mirror``)."""
    from nanomotif_amd._lib import NmScanError
    eng = context_engine
    cands = profile_cands()
    ecands = engine_cands(cands)
    states, table = eng.motif_context(ecands, radius=31)
    own = eng.motif_site_counts(ecands)
    for k, (c, (_, six)) in enumerate(zip(cands, own)):
        assert six.sum() > 0 and np.array_equal(states[k], six.sum(axis=0).reshape(2, 3)), c
    assert np.array_equal(table.sum(axis=-1), np.broadcast_to(states[:, None], table.shape[:-1]))
    checked = refused = 0
    for m, i, mt in (("GATC", 1, "a"), ("G[AG]TC", 1, "a"), ("C..GG", 0, "m"), ("A" + "." * 40 + "C", 0, "a")):
        k = cands.index(("b1", mt, m, i))
        fine, cells = [], []
        for o in (-31, -3, -1, 1, 2, 31):
            for x, letter in enumerate(LETTERS):
                f = narrowed(m, i, o, letter)
                if f is None:                                            # the motif excludes the letter: nothing there
                    assert not table[k, o + 31, :, :, x].any(), (m, o, letter)
                    continue
                fine.append((Motif(f[0], f[1]), mt, "b1"))
                cells.append((o, x))
        for f, (o, x) in zip(fine, cells):
            try:
                six = eng.motif_site_counts([f])[0][1].sum(axis=0).reshape(2, 3)
            except NmScanError as e:                                     # only a motif beyond the reach limit may be refused
                assert e.code == -5 and max(f[0].mod_position, len(f[0].tokens) - 1 - f[0].mod_position) > 95, f
                refused += 1
                continue
            assert np.array_equal(six, table[k, o + 31, :, :, x]), (m, o, LETTERS[x])
            checked += int(six.sum() > 0)
    assert checked >= 60 and refused == 0                                # within radius 31 no narrowed motif leaves the reach limit
    s10, t10 = eng.motif_context(ecands, radius=10)
    assert np.array_equal(s10, states) and np.array_equal(t10, table[:, 21:42])
    mirrored = [(Motif(m, i).reverse_compliment(), mt, b) for b, mt, m, i in cands]
    s_m, t_m = eng.motif_context(mirrored, radius=31)
    comp = [3, 2, 1, 0, 4]
    assert np.array_equal(s_m.sum(axis=2), states.sum(axis=2)[:, ::-1])
    assert np.array_equal(t_m.sum(axis=3), table.sum(axis=3)[:, ::-1, ::-1][..., comp])
    assert not np.array_equal(t_m.sum(axis=3), table.sum(axis=3)) and not np.array_equal(t_m.sum(axis=3), table.sum(axis=3)[:, ::-1, ::-1])


@gpu
def test_errors_are_loud_and_leave_the_engine_usable(context_engine):
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.engine import _ptr
    eng = context_engine
    cands, exp = profile_cands(), context_expected()
    k = cands.index(("b1", "a", "GATC", 1))
    b = eng.make_batch(engine_cands([cands[k]]))
    states, counts = np.zeros((1, 2, 3), np.uint64), np.zeros((1, 63, 2, 3, 4), np.int64)

    def call(bins=b.bins, slots=b.slots, radius=31):
        slots, bins = np.asarray(slots, np.uint8), np.asarray(bins, np.uint32)
        return eng.lib.nm_motif_context_count(eng.ctx, 1, _ptr(bins, C.c_uint32), _ptr(slots, C.c_uint8), _ptr(b.lens, C.c_uint8), _ptr(b.modpos, C.c_uint8),
                                              _ptr(b.offsets, C.c_uint32), _ptr(b.masks, C.c_uint8), radius, _ptr(states, C.c_uint64), _ptr(counts, C.c_int64))
    last = lambda: eng.lib.nm_last_error().decode()
    assert call(radius=32) == -1 and "radius" in last()                 # NM_EINVAL
    assert call(bins=[7]) == -1 and "cand_bin" in last() and "candidate 0" in last()
    assert call(slots=[5]) == -3 and "cand_mod_slot[0]" in last()       # NM_ESTATE: nothing uploaded there
    assert call(slots=[200]) == -3 and "cand_mod_slot[0]" in last()
    with pytest.raises(ValueError):
        eng.motif_context(engine_cands([cands[k]]), radius=32)
    with pytest.raises(NmScanError) as e:                               # beyond the reach limit: nm_motif_sites' code
        eng.motif_context([(Motif("A" + "." * 100 + "T", 0), "a", "b1")])
    assert e.value.code == -5
    assert not states.any() and not counts.any()                        # a refused call has written nothing
    assert call() == 0
    assert np.array_equal(states[0].astype(np.int64), exp[k][0]) and np.array_equal(counts[0], exp[k][1][..., :4])


# ------------------------------------------------------------------------------------------------ 4. the command
COMMAND_SPEC = synth.SynthSpec(n_contigs=4, total_bp=300_000, n_bins=2, mod_types=("a", "m"), seed=61, min_contig_bp=40_000,
                               fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m")))
COMMAND_RADIUS = 8


def expected_files(mg, cands, radius, min_called=20, min_gain=30.0):
    """The bodies of the three files: the brute force over the pre-filtered pileup, through the module's own formatter."""
    from nanomotif_amd.motif import iupac_to_regex
    from nanomotif_amd.motif_context import format_files
    from nanomotif_amd.motif_sites import SiteCandidate
    from nanomotif_amd.pileup import MOD_TYPES
    piles = _filtered_piles(mg)
    seqs = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    targets = [mt for mt in MOD_TYPES if piles[mt]]                      # slot order
    classes = Classes(seqs, piles, targets)
    bins = sorted(set(mg.bin_names))
    contigs = {bn: [n for i, n in enumerate(mg.names) if mg.bin_names[i] == bn] for bn in bins}
    known = [c for c in cands if c[2] in targets]
    tables = [context_of(contigs[bn], mt, iupac_to_regex(m), p, radius, classes)[1] for bn, m, mt, p in known]
    bg_keys = [(bn, mt) for bn in bins for mt in targets]
    bg_tables = [context_of(contigs[bn], mt, CANONICAL[mt], 0, radius, classes)[1] for bn, mt in bg_keys]
    texts = format_files([SiteCandidate(*c) for c in known], tables, bg_keys, bg_tables, min_called, min_gain)
    return [[line.split("\t") for line in t.split("\n")[1:-1]] for t in texts], targets


@gpu
def test_command_on_a_synthetic_metagenome(tmp_path):
    """motif_discovery, then motif_context --radius 8 on its bin-motifs.tsv plus a hand-written one (an under-specified GAT @ 1 and a
    row of a mod type the pileup does not hold), each in a child process: the three files equal the text derived from the brute force
    over the pre-filtered pileup; the offset-0 rows of the planted motifs sum to n_mod / n_nomod of bin-motifs.tsv and their flag is
    none; --radius 0 and --radius 31 run."""
    mg = synth.make_metagenome(COMMAND_SPEC)
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    mg.write_bed(tmp + "/pileup.bed")
    _run(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    found = open(tmp + "/out/bin-motifs.tsv").read()
    planted = [r for r in _rows(found)[1] if (r["motif"], r["mod_type"], r["mod_position"]) in (("GATC", "a", "1"), ("CCWGG", "m", "1"))]
    assert {r["motif"] for r in planted} == {"GATC", "CCWGG"}
    first = sorted(set(mg.bin_names))[0]
    extra = HEAD + f"{first}\tGAT\t1\ta\t1\t1\tnon-palindrome\t\t\t\t\n" + f"{first}\tGATC\t1\t21839\t1\t1\tpalindrome\t\t\t\t\n"
    open(tmp + "/extra.tsv", "w").write(extra)
    cands = candidates_of_texts([found, extra])
    (f_main, f_bins, f_summary), targets = expected_files(mg, cands, COMMAND_RADIUS)
    n_known = len(cands) - 1
    assert len(f_main) == n_known * (2 * COMMAND_RADIUS + 1) * 4 and len(f_bins) == 2 * len(targets) * (2 * COMMAND_RADIUS + 1) * 4 and len(f_summary) == n_known
    r = _run(tmp, "motif_context", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "extra.tsv", "--out", "cx",
                                    "--radius", str(COMMAND_RADIUS)])
    assert "the pileup holds no rows of mod type 21839" in r.stdout + r.stderr and "skipped" in r.stdout + r.stderr
    from nanomotif_amd.motif_context import MAIN_HEADER, SUMMARY_HEADER
    head, body = _body(f"{tmp}/cx/motif-context.tsv")
    assert head == MAIN_HEADER and body == f_main
    assert _body(f"{tmp}/cx/motif-context-bins.tsv") == (MAIN_HEADER, f_bins)
    head, summary = _body(f"{tmp}/cx/motif-context-summary.tsv")
    for row in summary:
        print("\t".join(row))
    assert head == SUMMARY_HEADER and summary == f_summary
    assert os.path.exists(f"{tmp}/cx/args.motif_context.json") and os.path.exists(f"{tmp}/cx/logs/timings.motif_context.json")
    by_key = {tuple(r[:4]): r for r in summary}
    for r in planted:
        key = (r["reference"], r["motif"], r["mod_type"], r["mod_position"])
        centre = [row for row in body if tuple(row[:4]) == key and row[4] == "0"]
        assert len(centre) == 4 and sum(int(row[6]) for row in centre) == int(r["n_mod"]) and sum(int(row[7]) for row in centre) == int(r["n_nomod"]), r
        assert by_key[key][4:6] == [r["n_mod"], r["n_nomod"]] and by_key[key][-1] == "none", by_key[key]
    # GAT @ 1 where GATC is methylated: the C behind it is what separates
    row = by_key[(first, "GAT", "a", "1")]
    assert row[8] == "2" and row[10] == "C" and row[11:13] == ["GATC", "1"] and row[-1] == "underspecified", row
    for radius in (0, 31):
        _run(tmp, "motif_context", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", f"cx{radius}",
                                    "--radius", str(radius)])
        head, body_r = _body(f"{tmp}/cx{radius}/motif-context.tsv")
        keys = {tuple(r[:4]) for r in body_r}
        assert len(body_r) == len(keys) * (2 * radius + 1) * 4
        inner = [r for r in body_r if abs(int(r[4])) <= min(radius, COMMAND_RADIUS)]
        assert inner == [r for r in f_main if tuple(r[:4]) in keys and abs(int(r[4])) <= radius]
