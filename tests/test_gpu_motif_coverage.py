"""GPU: coverage of a bin's methylation by a set of motifs (nm_motif_coverage_count / nm_motif_coverage_sites,
``ScanEngine.motif_coverage`` / ``unexplained_sites``, ``nanomotif motif_coverage``) against a brute-force oracle of Python sets built only
from ``oracle.scan.subseq_indices``, ``oracle.scan.split_positions`` and ``oracle.motif.Motif``.  Counts and records are integers: every
comparison is an equality over ALL sets, contigs and candidates of its input."""
import ctypes as C
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from helpers import oracle_bin_inputs
from nanomotif_amd import synth
from nanomotif_amd.motif import Motif

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_cover(seq, motif_str, pos):
    """{(position, strand)} one candidate covers on one contig: the stripped motif on '+' (strand 0), its reverse complement on '-'
    (strand 1), every (overlapping) occurrence shifted to the modified base."""
    from oracle.motif import Motif as OMotif
    from oracle.scan import subseq_indices
    st = OMotif(motif_str, pos).new_stripped_motif()
    out = set()
    for strand, m in ((0, st), (1, st.reverse_compliment())):
        out |= {(int(p), strand) for p in subseq_indices(m.string, seq) + m.mod_position}
    return out


def oracle_calls(pile, low, high):
    """(M, U): the distinct (position, strand) calls of one contig; a position called both ways is methylated."""
    from oracle.scan import split_positions
    mf, nf, mr, nr = split_positions(pile, low, high)
    M = {(int(p), 0) for p in mf} | {(int(p), 1) for p in mr}
    U = ({(int(p), 0) for p in nf} | {(int(p), 1) for p in nr}) - M
    return M, U


class Expected:
    """What the contract says about ``sets`` = [(bin, mod type, [(motif string, mod position), ...]), ...]: per set the int64[n, 10]
    table, per candidate the int64[n, 4] exclusive table and its own (fwd mod, fwd nomod, rev mod, rev nomod), and the unexplained
    records in contract order.  ``bin_contigs``: bin -> contig names in row order; ``contig_index``: contig name -> id."""

    def __init__(self, sets, bin_contigs, contig_index, seqs, piles, low=0.3, high=0.7):
        from oracle.scan import _EMPTY
        self.tables, self.exclusive, self.own, rec = [], [], [], []
        on = lambda xs, strand: {x for x in xs if x[1] == strand}
        for si, (b, mt, motifs) in enumerate(sets):
            names = bin_contigs[b]
            table = np.zeros((len(names), 10), dtype=np.int64)
            excl = [np.zeros((len(names), 4), dtype=np.int64) for _ in motifs]
            own = [np.zeros((len(names), 4), dtype=np.int64) for _ in motifs]
            for r, name in enumerate(names):
                M, U = oracle_calls(piles[mt].get(name, _EMPTY), low, high)
                covers = [oracle_cover(seqs[name], s, p) for s, p in motifs]
                times = Counter(x for c in covers for x in c)
                cover = set(times)
                once = {x for x, n in times.items() if n == 1}
                for strand in (0, 1):
                    Ms, Us, cs = on(M, strand), on(U, strand), on(cover, strand)
                    table[r, 5 * strand:5 * strand + 5] = (len(Ms), len(Ms & cs), len(Us), len(Us & cs), len(cs - Ms - Us))
                for j, c in enumerate(covers):
                    e = c & once
                    excl[j][r] = (len(on(e & M, 0)), len(on(e & U, 0)), len(on(e & M, 1)), len(on(e & U, 1)))
                    own[j][r] = (len(on(c & M, 0)), len(on(c & U, 0)), len(on(c & M, 1)), len(on(c & U, 1)))
                rec += [(si, contig_index[name], p, 4 * strand) for p, strand in sorted(M - cover)]    # ascending position, '+' before '-'
            self.tables.append(table)
            self.exclusive.append(excl)
            self.own.append(own)
        self.records = rec


def engine_sets(sets):
    return [(b, mt, [Motif(s, p) for s, p in motifs]) for b, mt, motifs in sets]


def records_of(eng, sets, max_records=None):
    """All records of ``eng.unexplained_sites`` as a list of (set, contig, pos, code), and the number of deliveries."""
    parts = list(eng.unexplained_sites(engine_sets(sets), max_records=max_records))
    assert max_records is None or all(len(p) <= max_records for p in parts)
    rec = np.concatenate(parts) if parts else np.zeros(0, dtype=[("set", "u4"), ("contig", "u4"), ("pos", "u4"), ("code", "u1")])
    return list(zip(rec["set"].tolist(), rec["contig"].tolist(), rec["pos"].tolist(), rec["code"].tolist())), len(parts)


def check(eng, sets, seqs, piles, low=0.3, high=0.7, what=""):
    """Tables and records of ``sets`` in ONE call each == the oracle; the identities of the contract.  Returns (Expected, got tables)."""
    bin_contigs = {b: eng.bin_contigs(b) for b, _, _ in sets}
    exp = Expected(sets, bin_contigs, eng.contig_index, seqs, piles, low, high)
    got = eng.motif_coverage(engine_sets(sets))
    assert len(got) == len(sets)
    for si, (names, table, per) in enumerate(got):
        assert names == bin_contigs[sets[si][0]]
        assert table.shape == exp.tables[si].shape and np.array_equal(table, exp.tables[si]), (what, sets[si][:2], table.tolist(), exp.tables[si].tolist())
        assert (table[:, 1] <= table[:, 0]).all() and (table[:, 6] <= table[:, 5]).all()
        assert len(per) == len(sets[si][2])
        for j, t in enumerate(per):
            assert np.array_equal(t, exp.exclusive[si][j]), (what, sets[si][:2], sets[si][2][j], t.tolist(), exp.exclusive[si][j].tolist())
    rec, _ = records_of(eng, sets)
    assert rec == exp.records, (what, len(rec), len(exp.records))
    assert len(rec) == sum(int((t[:, 0] - t[:, 1] + t[:, 5] - t[:, 6]).sum()) for _, t, _ in got)
    return exp, got


def _upload_metagenome(eng, mg, mod_types, low=0.3, high=0.7, min_cov=5):
    idx = list(range(len(mg.names)))
    eng.upload_assembly([mg.names[i] for i in idx], [mg.contig_ascii(i) for i in idx], [mg.bin_names[i] for i in idx])
    for mt in mod_types:
        first = True
        for local, i in enumerate(idx):
            p = mg.contig_pileup(i, mt)
            keep = p["nvalid"] > min_cov
            eng.upload_pileup(mt, np.full(int(keep.sum()), local, np.uint32), p["position"][keep], p["strand"][keep],
                              synth.pct_to_fraction(p["pct_hundredths"][keep]), low=low, high=high, append=not first)
            first = False


def reach_class(s, p):
    sets, mp = Motif(s, p).stripped_sets()
    r = max(mp, len(sets) - 1 - mp)
    return 0 if r <= 31 else 1 if r <= 63 else 2


# ------------------------------------------------------------------------------------------------ 1. the literal case
def test_literal_case_by_hand(engine_cls):
    """TACGGACGCCACG, '+' rows at 1 (0.9), 5 (0.95), 10 (0.1): ACG occurs at 1, 5, 10; GAC at 4 with its modified base at 5."""
    from oracle.scan import ContigPileup
    eng = engine_cls()
    eng.upload_assembly(["c"], ["TACGGACGCCACG"], ["b"])
    eng.upload_pileup("a", [0, 0, 0], [1, 5, 10], np.frombuffer(b"+++", np.uint8), [0.9, 0.95, 0.1])
    cov = lambda motifs: eng.motif_coverage([("b", "a", motifs)])[0]
    names, table, per = cov([Motif("ACG", 0)])
    assert names == ["c"] and table.tolist() == [[2, 2, 1, 1, 0, 0, 0, 0, 0, 0]] and [t.tolist() for t in per] == [[[2, 1, 0, 0]]]
    assert records_of(eng, [("b", "a", [("ACG", 0)])])[0] == []
    _, table, per = cov([Motif("ACG", 0), Motif("GAC", 1)])
    assert table.tolist() == [[2, 2, 1, 1, 0, 0, 0, 0, 0, 0]]
    assert [t.tolist() for t in per] == [[[1, 1, 0, 0]], [[0, 0, 0, 0]]]   # position 5 is shared
    _, table, per = cov([Motif("GAC", 1)])
    assert table.tolist() == [[2, 1, 1, 0, 0, 0, 0, 0, 0, 0]] and [t.tolist() for t in per] == [[[1, 0, 0, 0]]]
    assert records_of(eng, [("b", "a", [("GAC", 1)])])[0] == [(0, 0, 1, 0)]
    _, table, per = cov([])
    assert table.tolist() == [[2, 0, 1, 0, 0, 0, 0, 0, 0, 0]] and per == []
    assert records_of(eng, [("b", "a", [])])[0] == [(0, 0, 1, 0), (0, 0, 5, 0)]
    # all four in one call, and against the oracle
    pile = ContigPileup(np.array([1, 5, 10]), np.frombuffer(b"+++", np.uint8), np.array([0.9, 0.95, 0.1]))
    sets = [("b", "a", [("ACG", 0)]), ("b", "a", [("ACG", 0), ("GAC", 1)]), ("b", "a", [("GAC", 1)]), ("b", "a", [])]
    check(eng, sets, {"c": "TACGGACGCCACG"}, {"a": {"c": pile}})
    assert records_of(eng, sets)[0] == [(2, 0, 1, 0), (3, 0, 1, 0), (3, 0, 5, 0)]
    assert list(eng.unexplained_sites([])) == [] and eng.motif_coverage([]) == []
    eng.close()


# ------------------------------------------------------------------------------------------------ 2., 3. the synthetic metagenome
MOTIFS_A = [("GATC", 1), ("[AG]GATC[CT]", 2), ("GATC.......A", 1), ("GCAC......GTT", 2), ("AAC......GTGC", 1), ("A" + "." * 70 + "T", 0),
            ("G" + "." * 62 + "A", 63)]
MOTIFS_M = [("CC[AT]GG", 1), ("CCAGG", 1), ("C..GG", 0), ("C" + "." * 94 + "G", 0)]
NESTED = {("[AG]GATC[CT]", 2), ("GATC.......A", 1), ("CCAGG", 1)}      # every site also on GATC@1 / on CC[AT]GG@1 (C..GG is modified at 0)


def _zoo_metagenome():
    spec = synth.SynthSpec(n_contigs=20, total_bp=500_000, n_bins=8, mod_types=("a", "m"), seed=77, min_contig_bp=3_000, n_fraction=0.002,
                           fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m"), ("GCACNNNNNNGTT", 2, "a")))
    mg = synth.make_metagenome(spec)
    piles, seqs = {}, {}
    for mt in ("a", "m"):
        piles[mt], seqs = oracle_bin_inputs(mg, mt)
    return mg, seqs, piles


def _zoo_sets(mg):
    bins = sorted(set(mg.bin_names))
    assert len(bins) == 8
    return [(b, mt, list(MOTIFS_A if mt == "a" else MOTIFS_M)) for b in bins for mt in ("a", "m")]


def assert_not_degenerate(sets, exp):
    """The facts that keep the comparison from being one of zeros, taken from the ORACLE's side."""
    own, excl = Counter(), Counter()
    for si, (b, mt, motifs) in enumerate(sets):
        t = exp.tables[si].sum(axis=0)
        assert 0 < t[1] + t[6] < t[0] + t[5], (b, mt, t.tolist())
        # every set runs at the widest class with narrower programs sliced to it; the 6mA sets mix all three classes
        assert {reach_class(s, p) for s, p in motifs} == ({0, 1, 2} if mt == "a" else {0, 2})
        for j, m in enumerate(motifs):
            own[m] += int(exp.own[si][j].sum())
            excl[m] += int(exp.exclusive[si][j].sum())
            if m in NESTED:
                assert int(exp.exclusive[si][j].sum()) == 0 and int(exp.own[si][j].sum()) > 0, (b, mt, m)
    # (summed over the bins: a small bin may hold no called occurrence of a 13-mer at all)
    for m in own:
        assert (excl[m] == 0 and own[m] > 0) if m in NESTED else (0 < excl[m] < own[m]), (m, own[m], excl[m])


def test_synthetic_metagenome_all_sets_in_one_call(engine_cls):
    """8 bins x 2 mod types = 16 sets in ONE call; nested motifs, motifs of all three reach classes in one set."""
    mg, seqs, piles = _zoo_metagenome()
    sets = _zoo_sets(mg)
    eng = engine_cls()
    _upload_metagenome(eng, mg, ("a", "m"))
    exp = Expected(sets, {b: eng.bin_contigs(b) for b, _, _ in sets}, eng.contig_index, seqs, piles)
    assert_not_degenerate(sets, exp)
    before = eng.stats()["launches"]
    got = eng.motif_coverage(engine_sets(sets))
    assert eng.stats()["launches"] - before == 1            # every set runs at the widest class: ONE count launch for the 16 sets
    for si in range(len(sets)):
        print("coverage", sets[si][0], sets[si][1], "explained", int(got[si][1][:, [1, 6]].sum()), "of", int(got[si][1][:, [0, 5]].sum()))
    check(eng, sets, seqs, piles)
    eng.close()


def test_one_candidate_sets_are_motif_site_counts(engine_cls):
    """Every set of the metagenome split into one-candidate sets: mod_explained / nomod_covered / nocall_covered are that candidate's
    nm_motif_sites_count row and the exclusive table is its mod / nomod columns."""
    mg, seqs, piles = _zoo_metagenome()
    sets = [(b, mt, [m]) for b, mt, motifs in _zoo_sets(mg) for m in motifs]
    eng = engine_cls()
    _upload_metagenome(eng, mg, ("a", "m"))
    got = eng.motif_coverage(engine_sets(sets))
    counts = eng.motif_site_counts([(Motif(*motifs[0]), mt, b) for b, mt, motifs in sets])
    assert len(got) == len(counts) == 8 * (len(MOTIFS_A) + len(MOTIFS_M))
    n_sites = 0
    for (names, table, per), (cnames, six), s in zip(got, counts, sets):
        assert names == cnames and len(per) == 1
        assert np.array_equal(table[:, [1, 3, 4, 6, 8, 9]], six), s
        assert np.array_equal(per[0], six[:, [0, 1, 3, 4]]), s
        n_sites += int(six.sum())
    assert n_sites > 100_000
    check(eng, sets, seqs, piles)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. all six kernel variants
def test_three_widths_an_empty_set_and_a_motif_listed_twice(engine_cls):
    mg, seqs, piles = _zoo_metagenome()
    bins = sorted(set(mg.bin_names))
    sets = [(bins[0], "a", [("GATC", 1), ("A.A", 0)]),                                       # widest reach class 0
            (bins[1], "m", []),
            (bins[1], "a", [("GATC", 1), ("G" + "." * 40 + "C", 0)]),                        # class 1
            (bins[2], "a", []),
            (bins[2], "m", [("CC[AT]GG", 1), ("C" + "." * 94 + "G", 0), ("CCAGG", 1)]),      # class 2
            (bins[3], "a", [("GATC", 1), ("GATC", 1)])]                                      # the same motif twice
    assert [max([reach_class(s, p) for s, p in m] + [0]) for _, _, m in sets] == [0, 0, 1, 0, 2, 0]
    eng = engine_cls()
    _upload_metagenome(eng, mg, ("a", "m"))
    # the launch counter: the count pass runs once per width (3 variants); the export repeats it, scans, gathers and fills once per width
    before = eng.stats()["launches"]
    got = eng.motif_coverage(engine_sets(sets))
    assert eng.stats()["launches"] - before == 3
    before = eng.stats()["launches"]
    rec, n_deliveries = records_of(eng, sets)
    assert n_deliveries == 1 and eng.stats()["launches"] - before == 3 + (3 + 2 + 3)
    exp, _ = check(eng, sets, seqs, piles)
    # twice the same motif: everything it covers is covered twice, so nothing is exclusive, and the set equals the one-motif set
    assert [t.sum() for t in got[5][2]] == [0, 0] and got[5][1][:, [1, 6]].sum() > 0
    assert np.array_equal(got[5][1], eng.motif_coverage([(bins[3], "a", [Motif("GATC", 1)])])[0][1])
    # an empty set: nothing explained, every methylated call is an unexplained record
    for si in (1, 3):
        t = got[si][1]
        assert t[:, [1, 3, 4, 6, 8, 9]].sum() == 0 and t[:, [0, 5]].sum() > 0
        assert sum(1 for r in rec if r[0] == si) == int(t[:, [0, 5]].sum())
    eng.close()


# ------------------------------------------------------------------------------------------------ 4b. layouts
def _layout_case():
    rng = np.random.default_rng(12)
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    big = list(rand(60_000))                                            # spans eight chunks of 8192
    big[8185:8200] = "N" * 15                                           # an N run across a chunk border
    big[8170:8185] = "GATCGATCGATCGAT"                                  # ... with occurrences right before it
    big[8200:8204] = "GATC"
    big[16380:16390] = "AAAAAAAAAA"                                     # overlapping occurrences across a chunk border
    big[24574:24578] = "GATC"                                           # a palindrome astride a chunk border
    seqs = {"big": "".join(big), "tiny1": "G", "tiny2": "GA", "tiny3": "ATC", "ends_GA": rand(9000) + "GA", "starts_TC": "TC" + rand(500),
            "pal": "GATC" * 50 + "AATT" * 30, "n_only": "N" * 40, "edge": "GATC" + rand(8192 - 8) + "GATC", "edge2": rand(8191) + "A",
            "other_bin": "GATC" + rand(3000) + "GA", "other_bin2": "TC" + rand(100), "alone": rand(20_000)}
    bins = {n: ("b3" if n == "alone" else "b2" if n.startswith("other") else "b1") for n in seqs}
    return seqs, bins, rng


def test_layouts_that_break_naive_chunking(engine_cls):
    """Occurrences across the 8 192-position chunk border, N runs, contigs shorter than a motif, a many-contig (b1), a two-contig (b2) and a
    one-contig bin (b3), with sets of overlapping candidates of all three widths."""
    from oracle.scan import ContigPileup
    seqs, bins, rng = _layout_case()
    names = list(seqs)
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names])
    piles = {"a": {}, "m": {}}
    for mt in ("a", "m"):
        cid, pos, st, fr = [], [], [], []
        for i, n in enumerate(names):
            L = len(seqs[n])
            p = np.sort(rng.choice(L, size=max(1, L // 2), replace=False)).astype(np.int64)
            strand = rng.choice(np.array([ord("+"), ord("-")], dtype=np.uint8), size=len(p))
            f = rng.choice([0.0, 0.3, 0.30000000000000004, 0.5, 0.7, 0.6999999999999999, 1.0], size=len(p))
            if n == "big":                                              # two methylated calls ON the run of N, whatever the draw
                keep = ~np.isin(p, (8186, 8190))
                p, strand, f = np.append(p[keep], [8186, 8190]), np.append(strand[keep], [ord("+"), ord("-")]).astype(np.uint8), np.append(f[keep], [1.0, 1.0])
                o = np.argsort(p)
                p, strand, f = p[o], strand[o], f[o]
            piles[mt][n] = ContigPileup(p, strand, f)
            cid += [i] * len(p); pos += p.tolist(); st += strand.tolist(); fr += f.tolist()
        eng.upload_pileup(mt, cid, pos, np.array(st, np.uint8), fr)
    narrow = [("GATC", 1), ("GATC", 0), ("AA", 0), ("AA", 1), ("A", 0), ("AATT", 1), ("GA.C", 1), ("G[AG]TC", 1), ("A.........A", 0), ("ATC", 2), ("GAT[CG]", 3)]
    wide = narrow[:4] + [("G" + "." * 40 + "C", 0)]
    wider = narrow[:2] + [("G" + "." * 40 + "C", 0), ("A" + "." * 80 + "T", 81), ("T" + "." * 94 + "A", 0)]
    sets = [(b, mt, list(motifs)) for b in ("b1", "b2", "b3") for mt in ("a", "m") for motifs in (narrow, wide, wider, [])]
    exp, got = check(eng, sets, seqs, piles)
    assert sum(int(t.sum()) for e in exp.exclusive for t in e) > 1_000 and len(exp.records) > 10_000
    # spelled out: the N run holds no covered position; positions on it that carry a methylated call are unexplained
    si = sets.index(("b1", "a", narrow))
    big = [r for r in exp.records if r[0] == si and r[1] == names.index("big")]
    M, _ = oracle_calls(piles["a"]["big"], 0.3, 0.7)
    on_n = sorted((p, s) for p, s in M if 8185 <= p < 8200)
    assert {(8186, 0), (8190, 1)} <= set(on_n) and [(r[2], r[3] // 4) for r in big if 8185 <= r[2] < 8200] == on_n
    # ("A", 0) covers every A on '+' and every T on '-': a contig of N only explains nothing
    row = got[si][1][eng.bin_contigs("b1").index("n_only")]
    assert row[[1, 3, 4, 6, 8, 9]].sum() == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 5., 6. records, budgets, thresholds
def _small_case():
    spec = synth.SynthSpec(n_contigs=6, total_bp=120_000, n_bins=2, mod_types=("a",), seed=5, min_contig_bp=3_000, fixed_motifs=(("GATC", 1, "a"),))
    mg = synth.make_metagenome(spec)
    piles, seqs = {}, {}
    piles["a"], seqs = oracle_bin_inputs(mg, "a")
    bins = sorted(set(mg.bin_names))
    sets = [(bins[0], "a", [("GATC", 1), ("G[AG].GAAG[CT]", 5)]), (bins[1], "a", []), (bins[0], "a", [("A" + "." * 70 + "T", 0)]),
            (bins[1], "a", [("GATC", 1), ("[AG]GATC[CT]", 2), ("A", 0)]), (bins[1], "a", [("CC[AT]GG", 1)])]
    return mg, seqs, piles, sets


def test_unexplained_records_do_not_depend_on_the_budget(engine_cls):
    mg, seqs, piles, sets = _small_case()
    eng = engine_cls()
    _upload_metagenome(eng, mg, ("a",))
    exp, got = check(eng, sets, seqs, piles)
    per_set = Counter(r[0] for r in exp.records)
    assert len(exp.records) > 1_000 and per_set[3] == 0 and per_set[1] > 100       # ("A", 0) on '+' leaves nothing; the empty set everything
    whole, n = records_of(eng, sets)
    assert n == 1 and whole == exp.records
    for budget in (1000, 7, 1):
        rec, n_b = records_of(eng, sets, max_records=budget)
        assert rec == exp.records, budget
        assert n_b >= len(exp.records) // budget
    assert len(whole) == sum(int((t[:, 0] - t[:, 1] + t[:, 5] - t[:, 6]).sum()) for _, t, _ in got)
    with pytest.raises(ValueError):
        list(eng.unexplained_sites(engine_sets(sets), max_records=0))
    # the ABI's windows: odd sizes tile the call, nothing beyond what was reported is touched
    from nanomotif_amd import _lib
    from nanomotif_amd.engine import _ptr
    args, keep, _ = eng._coverage_args(engine_sets(sets))
    total, at, parts = len(exp.records), 0, []
    while at < total:
        cap = 333
        contig, pos, code = (np.full(cap + 8, 0xEE, dtype=t) for t in (np.uint32, np.uint32, np.uint8))
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        nw = C.c_uint64(99)
        _lib.check(eng.lib.nm_motif_coverage_sites(*args, at, cap, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8),
                                                   _ptr(off, C.c_uint64), C.byref(nw)))
        assert nw.value == min(cap, total - at) and (code[nw.value:] == 0xEE).all() and (pos[nw.value:] == 0xEE).all()
        assert off.tolist() == [sum(per_set[j] for j in range(s)) for s in range(len(sets) + 1)]
        parts += list(zip(contig[:nw.value].tolist(), pos[:nw.value].tolist(), code[:nw.value].tolist()))
        at += int(nw.value)
    assert parts == [r[1:] for r in exp.records]
    nw = C.c_uint64(99)
    off = np.zeros(len(sets) + 1, dtype=np.uint64)
    _lib.check(eng.lib.nm_motif_coverage_sites(*args, total + 5, 10, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8),
                                               _ptr(off, C.c_uint64), C.byref(nw)))
    assert nw.value == 0 and int(off[-1]) == total
    eng.close()


@pytest.mark.parametrize("low,high", [(0.3, 0.7), (0.1, 0.9)])
def test_thresholds(engine_cls, low, high):
    mg, seqs, piles, sets = _small_case()
    eng = engine_cls()
    _upload_metagenome(eng, mg, ("a",), low=low, high=high)
    exp, _ = check(eng, sets, seqs, piles, low=low, high=high, what=(low, high))
    print("thresholds", low, high, "mod_total", [int(t[:, [0, 5]].sum()) for t in exp.tables], "records", len(exp.records))
    assert len(exp.records) > 500
    eng.close()


def test_thresholds_change_the_result():
    """(oracle side only) the two classifications of test_thresholds are different inputs."""
    mg, seqs, piles, sets = _small_case()
    names = {b: [n for i, n in enumerate(mg.names) if mg.bin_names[i] == b] for b in set(mg.bin_names)}
    index = {n: i for i, n in enumerate(mg.names)}
    a, b = (Expected(sets, names, index, seqs, piles, lo, hi) for lo, hi in ((0.3, 0.7), (0.1, 0.9)))
    assert any(not np.array_equal(x, y) for x, y in zip(a.tables, b.tables)) and a.records != b.records


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors_are_loud_and_leave_the_engine_usable(engine_cls):
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.engine import _ptr
    eng = engine_cls()
    eng.upload_assembly(["c"], ["GATCGATC"], ["b"])
    eng.upload_pileup("a", [0], [1], np.frombuffer(b"+", np.uint8), [1.0])
    for call in (eng.motif_coverage, lambda s: list(eng.unexplained_sites(s))):
        with pytest.raises(NmScanError) as e:                           # no such bin
            call([(7, "a", [Motif("GATC", 1)])])
        assert e.value.code == -1                                       # NM_EINVAL
        with pytest.raises(NmScanError) as e:                           # no pileup in the slot
            call([("b", 1, [Motif("GATC", 1)])])
        assert e.value.code == -3                                       # NM_ESTATE
        with pytest.raises(NmScanError) as e:                           # no such bin and no pileup in the slot: the bin is refused first
            call([(7, 1, [Motif("GATC", 1)])])
        assert e.value.code == -1
        with pytest.raises(NmScanError) as e:                           # reaches further than 95 from the modified base
            call([("b", "a", [Motif("GATC", 1), Motif("A" + "." * 100 + "T", 0)])])
        assert e.value.code == -5                                       # NM_ERANGE
    # offsets that do not ascend, at the ABI
    args, keep, _ = eng._coverage_args([("b", "a", [Motif("GATC", 1)]), ("b", "a", [Motif("TCG", 0)])])
    good = keep[2].copy()
    rows, crows = np.array([0, 1, 2], np.uint64), np.array([0, 1, 2], np.uint64)
    totals, st, ct = np.zeros(2, np.uint64), np.zeros((2, 10), np.int64), np.zeros((2, 4), np.int64)
    tail = lambda r, cr: (_ptr(r, C.c_uint64), _ptr(cr, C.c_uint64), _ptr(totals, C.c_uint64), _ptr(st, C.c_int64), _ptr(ct, C.c_int64))
    keep[2][:] = [0, 2, 1]
    assert eng.lib.nm_motif_coverage_count(*args, *tail(rows, crows)) == -1
    keep[2][:] = [1, 1, 2]
    assert eng.lib.nm_motif_coverage_count(*args, *tail(rows, crows)) == -1
    keep[2][:] = good
    assert eng.lib.nm_motif_coverage_count(*args, *tail(np.array([0, 1, 0], np.uint64), crows)) == -1
    assert eng.lib.nm_motif_coverage_count(*args, *tail(rows, np.array([0, 0, 1], np.uint64))) == -1      # a candidate without a row
    assert eng.lib.nm_motif_coverage_count(eng.ctx, 1, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert eng.lib.nm_motif_coverage_sites(eng.ctx, 1, None, None, None, None, None, None, None, 0, 0, None, None, None, None, None) == -1
    assert eng.lib.nm_motif_coverage_count(*args, *tail(rows, crows)) == 0
    # TCG@0 occurs at 2 on '+'; its reverse complement CGA at 3, modified base at 5 on '-'
    assert st.tolist() == [[1, 1, 0, 0, 1, 0, 0, 0, 0, 2], [1, 0, 0, 0, 1, 0, 0, 0, 0, 1]] and totals.tolist() == [0, 1]
    # the engine is usable afterwards: GATC@1 on GATCGATC covers '+' 1, 5 and '-' 2, 6; the one methylated call (1, '+') is explained
    names, table, per = eng.motif_coverage([("b", "a", [Motif("GATC", 1)])])[0]
    assert table.tolist() == [[1, 1, 0, 0, 1, 0, 0, 0, 0, 2]] and per[0].tolist() == [[1, 0, 0, 0]]
    assert list(eng.unexplained_sites([("b", "a", [Motif("GATC", 1)])]))[0].tolist() == []
    assert [tuple(r) for r in np.concatenate(list(eng.unexplained_sites([("b", "a", [Motif("TCG", 0)])]))).tolist()] == [(0, 0, 1, 0)]
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. the command
def _run(tmp, command, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "nanomotif_amd", command] + args, cwd=tmp, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _filtered_piles(mg):
    """mod type -> {contig -> ContigPileup} after the three pre-filters of motif_discovery (find_motifs_bin.py:399-414), per bin as
    oracle.pipeline.bin_rows builds them."""
    from oracle import pileup as op
    from oracle import pipeline as opl
    from oracle.scan import ContigPileup
    piles = {mt: {} for mt in opl.MODS}
    for b in sorted(set(mg.bin_names)):
        t, idx = opl.bin_table(mg, b)
        t = op.prefilter(t)
        for mt_id, mt in enumerate(opl.MODS):
            for i in idx:
                s = (t["mod_type"] == mt_id) & (t["contig"] == i)
                if s.any():
                    o = np.argsort(t["position"][s], kind="stable")
                    piles[mt][mg.names[i]] = ContigPileup(t["position"][s][o], t["strand"][s][o], t["fraction_mod"][s][o])
    return piles


def _rows(text):
    lines = text.strip().split("\n")
    head = lines[0].split("\t")
    return head, [dict(zip(head, line.split("\t"))) for line in lines[1:]]


def _expected_files(mg, bin_motifs_text, mod_types):
    """The four files the oracle gives for the candidates of a bin-motifs.tsv (complements included, duplicates dropped)."""
    from nanomotif_amd.motif import iupac_to_regex
    piles = _filtered_piles(mg)
    seqs = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    cands, seen = [], set()
    for row in _rows(bin_motifs_text)[1]:
        both = [(row["reference"], row["motif"], row["mod_type"], int(row["mod_position"]))]
        if row["motif_complement"]:
            both.append((row["reference"], row["motif_complement"], row["mod_type"], int(row["mod_position_complement"])))
        for c in both:
            if c not in seen:
                seen.add(c)
                cands.append(c)
    bins = sorted(set(mg.bin_names))
    bin_contigs = {b: [n for i, n in enumerate(mg.names) if mg.bin_names[i] == b] for b in bins}      # contig_bin.tsv order
    keys = [(b, mt) for b in bins for mt in mod_types]
    iupac = {k: [(m, p) for b, m, mt, p in cands if (b, mt) == k] for k in keys}
    sets = [(b, mt, [(iupac_to_regex(m), p) for m, p in iupac[(b, mt)]]) for b, mt in keys]
    exp = Expected(sets, bin_contigs, {n: i for i, n in enumerate(mg.names)}, seqs, piles)
    f_sets, f_contigs, f_motifs = [], [], []
    for si, (b, mt, motifs) in enumerate(sets):
        t = exp.tables[si].sum(axis=0)
        n_mod, n_exp = int(t[0] + t[5]), int(t[1] + t[6])
        f_sets.append([b, mt, str(len(motifs)), str(n_mod), str(n_exp), str(n_mod - n_exp), "%.6f" % (n_exp / n_mod) if n_mod else "nan",
                       str(int(t[2] + t[7])), str(int(t[3] + t[8])), str(int(t[4] + t[9]))])
        f_contigs += [[b, name, mt] + [str(int(x)) for x in exp.tables[si][r]] for r, name in enumerate(bin_contigs[b])]
        for j, (m, p) in enumerate(iupac[(b, mt)]):
            own, ex = exp.own[si][j].sum(axis=0), exp.exclusive[si][j].sum(axis=0)
            f_motifs.append([b, m, mt, str(p), str(int(own[0] + own[2])), str(int(own[1] + own[3])), str(int(ex[0] + ex[2])), str(int(ex[1] + ex[3]))])
    bed = "".join(f"{mg.names[c]}\t{p}\t{p + 1}\t{sets[si][1]}\t0\t{'-' if code else '+'}\t{sets[si][0]}\n" for si, c, p, code in exp.records)
    return f_sets, f_contigs, f_motifs, bed, sets


def _body(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [line.split("\t") for line in lines[1:-1]]


def test_command_after_motif_discovery(tmp_path):
    """motif_discovery then motif_coverage --unexplained_sites, each in a child process: the three tables and the BED equal the oracle's for
    the candidates of the produced bin-motifs.tsv; every row of bin-motifs.tsv finds its n_mod / n_nomod; a bin without motifs has its row."""
    from nanomotif_amd import pileup as pileup_mod
    spec = synth.SynthSpec(n_contigs=4, total_bp=500_000, n_bins=2, mod_types=("a", "m"), seed=61, min_contig_bp=60_000,
                           fixed_motifs=(("GATC", 1, "a"), ("ACCCA", 4, "a"), ("GRNGAAGY", 5, "a"), ("CCWGG", 1, "m")))
    mg = synth.make_metagenome(spec)
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_bed(tmp + "/pileup.bed")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    _run(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    bm = open(tmp + "/out/bin-motifs.tsv").read()
    bm_head, bm_rows = _rows(bm)
    assert {"GATC", "ACCCA", "CCWGG"} <= {r["motif"] for r in bm_rows} and any(r["motif_complement"] for r in bm_rows)
    mod_types = [mt for mt in pileup_mod.MOD_TYPES if mt in ("a", "m")]                   # slot order
    for bin_motifs, out in (("out/bin-motifs.tsv", "cov"), ("one_bin.tsv", "cov_one")):
        if out == "cov_one":                                            # a bin-motifs.tsv that has no motif for the second bin
            dropped = sorted(set(mg.bin_names))[1]
            lines = bm.strip().split("\n")
            bm = "\n".join([lines[0]] + [l for l in lines[1:] if l.split("\t")[0] != dropped]) + "\n"
            assert 1 < len(bm.strip().split("\n")) < len(lines)
            open(tmp + "/one_bin.tsv", "w").write(bm)
        _run(tmp, "motif_coverage", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", bin_motifs, "--out", out, "--unexplained_sites"])
        f_sets, f_contigs, f_motifs, bed, sets = _expected_files(mg, bm, mod_types)
        head, body = _body(f"{tmp}/{out}/motif-coverage.tsv")
        assert head == ["bin", "mod_type", "n_motifs", "n_mod", "n_mod_explained", "n_mod_unexplained", "fraction_explained", "n_nomod",
                        "n_nomod_covered", "n_nocall_covered"]
        for row in body:
            print(out, "\t".join(row))
        assert body == f_sets and len(body) == 2 * len(mod_types)
        assert any(int(r[2]) > 0 and 0 < int(r[4]) < int(r[3]) for r in body)
        head, body = _body(f"{tmp}/{out}/motif-coverage-contigs.tsv")
        assert head[:3] == ["bin", "contig", "mod_type"] and len(head) == 13 and body == f_contigs
        head, body = _body(f"{tmp}/{out}/motif-coverage-motifs.tsv")
        assert head == ["bin", "motif", "mod_type", "mod_position", "n_mod", "n_nomod", "n_mod_exclusive", "n_nomod_exclusive"] and body == f_motifs
        got_bed = open(f"{tmp}/{out}/unexplained-sites.bed").read()
        assert len(got_bed) == len(bed) and got_bed == bed and len(bed) > 0
        assert os.path.exists(f"{tmp}/{out}/args.motif_coverage.json") and os.path.exists(f"{tmp}/{out}/logs/timings.motif_coverage.json")
        # every row of this bin-motifs.tsv: its n_mod / n_nomod (and its complement's) are the motif table's
        table = {(r[0], r[1], r[2], int(r[3])): (int(r[4]), int(r[5])) for r in body}
        assert len(table) == len(body)
        for r in _rows(bm)[1]:
            assert table[(r["reference"], r["motif"], r["mod_type"], int(r["mod_position"]))] == (int(r["n_mod"]), int(r["n_nomod"])), r
            if r["motif_complement"]:
                assert table[(r["reference"], r["motif_complement"], r["mod_type"], int(r["mod_position_complement"]))] == \
                    (int(r["n_mod_complement"]), int(r["n_nomod_complement"])), r
        if out == "cov_one":                                            # the bin without motifs still has its rows: methylation, nothing explained
            rows = [r for r in _body(f"{tmp}/{out}/motif-coverage.tsv")[1] if r[0] == dropped]
            assert len(rows) == len(mod_types) and all(r[2] == "0" and r[4] == "0" and r[6] in ("0.000000", "nan") for r in rows)
            assert any(int(r[3]) > 0 for r in rows)
    # without --unexplained_sites no BED is written and the tables are the same
    _run(tmp, "motif_coverage", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "cov_plain"])
    assert not os.path.exists(tmp + "/cov_plain/unexplained-sites.bed")
    for name in ("motif-coverage.tsv", "motif-coverage-contigs.tsv", "motif-coverage-motifs.tsv"):
        assert open(f"{tmp}/cov_plain/{name}").read() == open(f"{tmp}/cov/{name}").read()
