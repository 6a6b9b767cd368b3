"""CPU: the host half of ``nanomotif motif_overlap`` — the parser, the build list, the NULL-context refusal, pair statistics, ``relation``,
``symbolic`` and every flag with its precedence and both sides of each threshold on hand-made tables, the formatters byte for byte, nan
handling, the symmetry check on a doctored table — and the conditions on the geometry input of ``overlap_geometry`` that the GPU suite
(``test_gpu_motif_overlap``) relies on."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import overlap_geometry as G
from nanomotif_amd import motif_overlap as MO
from nanomotif_amd.motif_coverage import CoverageSet
from nanomotif_amd.motif_sites import SiteCandidate


def table(*blocks):
    """int64[len(blocks), 1 contig, 2, 3] with every block = (mod, nomod, nocall) put on the forward strand."""
    t = np.zeros((len(blocks), 1, 2, 3), np.int64)
    for k, b in enumerate(blocks):
        t[k, 0, 0] = b
    return t


def stats_of(own, shared):
    """SetStats of n motifs from ``own[i]`` = (mod, nomod, nocall) and ``shared[(i, j)]`` for i < j (absent: nothing shared); the rest
    (``only``) is given as own minus the shared parts, which is exact when the partners do not overlap each other."""
    n = len(own)
    sh = lambda i, j: np.asarray(shared.get((min(i, j), max(i, j)), (0, 0, 0)), np.int64)
    tables = []
    for i in range(n):
        others = [sh(i, j) for j in range(n) if j != i]
        tables.append(table(own[i], *others, np.asarray(own[i], np.int64) - sum(others, np.zeros(3, np.int64))))
    return MO.set_stats(tables)


def cset(motifs, b="b", mt="a"):
    return CoverageSet(b, mt, [SiteCandidate(b, m, mt, p) for m, p in motifs])


# ------------------------------------------------------------------------------------------------ parser, build list, NULL ctx
def test_parser_takes_the_arguments_of_the_issue():
    from nanomotif_amd.argparser import create_parser
    p = create_parser()
    a = p.parse_args(["motif_overlap", "asm.fa", "pile.bed", "-c", "cb.tsv", "--bin_motifs", "x.tsv", "y.tsv", "--out", "o"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.bin_motifs, a.out) == ("motif_overlap", "asm.fa", "pile.bed", "cb.tsv", ["x.tsv", "y.tsv"], "o")
    assert (a.all_pairs, a.min_called, a.max_outside, a.min_frac) == (False, 20, 0.3, 0.7)
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device) == (0.3, 0.7, 5, None)
    a = p.parse_args(["motif_overlap", "a", "p", "-c", "c", "--bin_motifs", "x", "--all_pairs", "--min_called", "5", "--max_outside", "0.2", "--min_frac", "0.9"])
    assert (a.all_pairs, a.min_called, a.max_outside, a.min_frac) == (True, 5, 0.2, 0.9)
    with pytest.raises(SystemExit):
        p.parse_args(["motif_overlap", "a", "p", "-c", "c"])                # --bin_motifs is required


def test_the_unit_is_built_and_refuses_a_null_context_without_a_gpu():
    from nanomotif_amd import _lib, build
    assert os.path.join("csrc", "nmoverlap.hip") in [os.path.relpath(s, os.path.dirname(build.__file__)) for s in build.SRC_HIP]
    assert "nm_motif_overlap_count" in _lib.SYMBOLS
    lib = _lib.load()
    one = np.zeros(2, np.uint64)
    off = np.zeros(2, np.uint32)
    u64, u32 = one.ctypes.data_as(C.POINTER(C.c_uint64)), off.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.nm_motif_overlap_count(None, 0, None, None, None, None, None, None, u32, None, None, None, None, u64, None) == -1
    assert b"ctx is NULL" in lib.nm_last_error()
    assert lib.nm_motif_overlap_count(None, 0, None, None, None, None, None, None, None, None, None, None, None, u64, None) == -1
    assert b"NULL argument" in lib.nm_last_error()


# ------------------------------------------------------------------------------------------------ relation, symbolic
def test_relation_is_decided_by_counts():
    r = MO.relation
    assert r(10, 10, 10) == "identical" and r(4, 10, 4) == "a_in_b" and r(10, 4, 4) == "b_in_a" and r(10, 10, 9) == "overlapping"
    assert r(10, 4, 3) == "overlapping" and r(10, 4, 0) == "disjoint"
    assert r(0, 4, 0) == r(4, 0, 0) == r(0, 0, 0) == "no_sites"            # before disjoint
    assert set(MO.RELATIONS) == {"identical", "a_in_b", "b_in_a", "overlapping", "disjoint", "no_sites"}


SYMBOLIC_CASES = [(("GATC", 1), ("RGATCY", 2), "b_in_a"), (("RGATCY", 2), ("GATC", 1), "a_in_b"), (("GATC", 1), ("GATC", 1), "identical"),
                  (("GATC", 1), ("NNNGATC", 4), "identical"), (("GATCN", 1), ("GATC", 1), "identical"), (("GATC", 1), ("GATC", 0), "none"),
                  (("CCWGG", 1), ("CCAGG", 1), "b_in_a"), (("CCAGG", 1), ("CCTGG", 1), "none"), (("GATCH", 1), ("DGATC", 2), "none"),
                  (("SATC", 1), ("GATC", 1), "b_in_a"), (("GATC", 1), ("GTAC", 2), "none"), (("GATCNNNNT", 1), ("GATC", 1), "a_in_b")]


@pytest.mark.parametrize("a,b,want", SYMBOLIC_CASES)
def test_symbolic_on_hand_made_pairs(a, b, want):
    assert MO.symbolic(SiteCandidate("b", a[0], "a", a[1]), SiteCandidate("b", b[0], "a", b[1])) == want
    assert G.symbolic_oracle(a[0], a[1], b[0], b[1]) == want


# ------------------------------------------------------------------------------------------------ the geometry input
def test_the_input_has_what_the_checks_need():
    from test_gpu_motif_compare import reach_class
    bf = G.BruteForce()
    assert [reach_class(m, p) for m, p in G.A_SET] == [0, 0, 0, 0, 1, 2, 0, 0, 0, 0] and {reach_class(m, p) for m, p in G.M_SET} == {0}
    gatc, rgatcy, gatch, dgatc, g40, g70, gtac, gatcn, satc, again = range(10)
    for b in G.BINS:
        st = MO.set_stats(bf.all_others(b, "a"))
        tot, sh = st.own.sum(axis=1), st.shared.sum(axis=2)
        rel = lambda i, j: MO.relation(tot[i], tot[j], sh[i, j])
        # proper nesting in both directions, also of a G = 1 owner in G = 2 and G = 3 partners and the reverse
        assert [rel(gatc, j) for j in (rgatcy, gatch, dgatc, g40, g70)] == ["b_in_a"] * 5 and [rel(j, gatc) for j in (rgatcy, g40, g70)] == ["a_in_b"] * 3
        assert rel(gatc, satc) == "a_in_b" and rel(satc, g70) == "b_in_a"
        # overlapping pairs, among them G = 2 against G = 3
        assert rel(gatch, dgatc) == rel(g40, g70) == rel(rgatcy, g40) == rel(dgatc, g70) == "overlapping" and 0 < sh[gatch, dgatc] < min(tot[gatch], tot[dgatc])
        # disjoint: GTAC against everything; the spellings of GATC identical
        assert all(rel(gtac, j) == "disjoint" for j in range(10) if j != gtac) and tot[gtac] > 0
        assert rel(gatc, again) == rel(gatc, gatcn) == rel(gatcn, again) == "identical"
        # shared sites on both strands for every related pair, in all three states where the smaller motif has 60 sites
        full = bf.all_others(b, "a")
        for i, j in itertools.permutations(range(10), 2):
            if rel(i, j) != "disjoint":
                block = full[i][1 + (j if j < i else j - 1)].sum(axis=0)
                assert block.sum(axis=1).min() > 0, (b, i, j, block.tolist())
                assert block.sum(axis=0).min() > 0 or min(tot[i], tot[j]) < 60, (b, i, j, block.tolist())
        assert st.only[gtac].sum() == tot[gtac] and st.only[satc].sum() == tot[satc] - tot[gatc] > 0 and st.only[[gatc, rgatcy, g40, g70]].sum() == 0
        m = MO.set_stats(bf.all_others(b, "m"))
        mt, ms = m.own.sum(axis=1), m.shared.sum(axis=2)
        assert ms[0, 1] == mt[1] > 0 and ms[0, 2] == mt[2] > 0 and ms[1, 2] == 0 and mt[1] + mt[2] == mt[0] and m.only.sum() == 0
    # GATC. as spelled (the dot inside the contig) is short of GATC by exactly the contig-end occurrence; by the contract it is GATC
    for contig, n in (("mid", 100), ("long", 206)):
        spelled = sum(len(x) for x in G.regex_positions(bf.seqs[contig], "GATC.", 1))
        assert spelled == n - 1 and len(bf.sites(contig, ("GATC.", 1))) == len(bf.sites(contig, ("GATC", 1))) == n
        assert (G.LENGTHS[contig] - 3, 0) in bf.sites(contig, ("GATC.", 1))
    # across the work-item border, on bit 31 and bit 0 of a word, either side of the lane border 127 | 128
    for contig in ("mid", "long"):
        s = bf.sites(contig, ("GATC", 1))
        assert (G.BORDER - 1, 0) in s and (G.BORDER, 1) in s
    assert (127, 0) in bf.sites("mid", ("GATC", 1)) and (128, 0) in bf.sites("long", ("GATC", 1)) and (128, 1) in bf.sites("mid", ("GATC", 1))
    assert (31, 0) in bf.sites("mid", ("CCAGG", 1)) and (64, 0) in bf.sites("mid", ("CCTGG", 1)) and (255, 0) in bf.sites("long", ("CCTGG", 1))
    assert (128 + 8192, 0) in bf.sites("long", ("CCAGG", 1))
    states = np.concatenate([bf.states[mt][n].ravel() for mt in "am" for n in G.NAMES])
    assert all((states == k).mean() > 0.2 for k in range(3))


def test_symbolic_nesting_implies_nesting_by_counts_on_the_brute_force():
    bf = G.BruteForce()
    seen = set()
    for b, mt in itertools.product(G.BINS, "am"):
        ms = G.SETS[mt]
        st = MO.set_stats(bf.all_others(b, mt))
        tot, sh = st.own.sum(axis=1), st.shared.sum(axis=2)
        for i, j in itertools.permutations(range(len(ms)), 2):
            a, c = (G.to_iupac(ms[i][0]), ms[i][1]), (G.to_iupac(ms[j][0]), ms[j][1])
            sym = MO.symbolic(SiteCandidate(b, a[0], mt, a[1]), SiteCandidate(b, c[0], mt, c[1]))
            assert sym == G.symbolic_oracle(*a, *c), (a, c)
            rel = MO.relation(tot[i], tot[j], sh[i, j])
            seen.add((sym, rel))
            if sym == "a_in_b":
                assert rel in ("a_in_b", "identical") and sh[i, j] == tot[i], (a, c, rel)
            elif sym == "identical":
                assert rel == "identical", (a, c, rel)
    assert {("a_in_b", "a_in_b"), ("b_in_a", "b_in_a"), ("identical", "identical"), ("none", "overlapping"), ("none", "disjoint")} <= seen


# ------------------------------------------------------------------------------------------------ pair statistics and the formatters
def test_pair_statistics_and_both_files_byte_for_byte():
    """GATC (60 mod / 40 nomod / 10 nocall) with RGATCY inside it (49 / 1 / 2) and an unrelated GTAC (5 / 25 / 0): GATC outside RGATCY
    is 11 / 39 — a parent carried by its child."""
    own = [(60, 40, 10), (49, 1, 2), (5, 25, 0)]
    st = stats_of(own, {(0, 1): (49, 1, 2)})
    assert st.own.tolist() == [list(x) for x in own] and st.shared[0, 1].tolist() == st.shared[1, 0].tolist() == [49, 1, 2]
    assert st.only.tolist() == [[11, 39, 8], [0, 0, 0], [5, 25, 0]]
    children, parents, duplicates = MO.nesting(st)
    assert (children, parents, duplicates) == ([[1], [], []], [[], [0], []], [[], [], []])
    MO.add_outside(st, children, {0: table(own[0], (49, 1, 2), (11, 39, 8))})
    assert st.outside.tolist() == [[11, 39, 8], [49, 1, 2], [5, 25, 0]]
    s = cset([("GATC", 1), ("RGATCY", 2), ("GTAC", 2)])
    head = "\t".join(MO.PAIRS_HEADER) + "\n"
    row01 = "b\ta\tGATC\t1\tRGATCY\t2\t110\t52\t49\t1\t2\t0.472727\t1.000000\t0.472727\t0.980000\t50\t0.220000\t50\tnan\t0\tb_in_a\tb_in_a\n"
    row02 = "b\ta\tGATC\t1\tGTAC\t2\t110\t30\t0\t0\t0\t0.000000\t0.000000\t0.000000\tnan\t0\t0.600000\t100\t0.166667\t30\tdisjoint\tnone\n"
    row12 = "b\ta\tRGATCY\t2\tGTAC\t2\t52\t30\t0\t0\t0\t0.000000\t0.000000\t0.000000\tnan\t0\t0.980000\t50\t0.166667\t30\tdisjoint\tnone\n"
    assert MO.format_pairs([s], [st]) == head + row01
    assert MO.format_pairs([s], [st], all_pairs=True) == head + row01 + row02 + row12
    want = "\t".join(MO.MOTIFS_HEADER) + "\n" + \
        "b\ta\tGATC\t1\t60\t40\t10\t1\tRGATCY_a_2\t\t\t11\t39\t11\t39\t0.220000\t0.980000\tcarried_by_children\n" + \
        "b\ta\tRGATCY\t2\t49\t1\t2\t1\t\tGATC_a_1\t\t0\t0\t49\t1\t0.980000\tnan\tnone\n" + \
        "b\ta\tGTAC\t2\t5\t25\t0\t0\t\t\t\t5\t25\t5\t25\t0.166667\tnan\tnone\n"
    assert MO.format_motifs([s], [st]) == want
    assert MO.format_pairs([], []) == head and MO.format_motifs([], []) == "\t".join(MO.MOTIFS_HEADER) + "\n"


def test_nan_handling():
    assert MO.ratio_text(0, 0) == "nan" and MO.ratio_text(1, 3) == "0.333333" and MO.ratio_text(3, 3) == "1.000000"
    assert np.isnan(MO.frac_mod((0, 0, 7))) and MO.frac_mod((3, 1, 9)) == 0.75
    # a motif without a site, one with sites but no call: every ratio of their rows is nan, nothing divides by zero
    st = stats_of([(0, 0, 0), (0, 0, 6), (4, 4, 0)], {(1, 2): (0, 0, 0)})
    s = cset([("GATC", 1), ("GTAC", 2), ("CATG", 1)])
    text = MO.format_pairs([s], [st], all_pairs=True).split("\n")
    assert text[1].split("\t")[6:] == ["0", "6", "0", "0", "0", "nan", "0.000000", "0.000000", "nan", "0", "nan", "0", "nan", "0", "no_sites", "none"]
    assert text[3].split("\t")[-2:] == ["disjoint", "none"]
    rows = [r.split("\t") for r in MO.format_motifs([s], [st]).split("\n")[1:4]]
    assert [r[-3:] for r in rows] == [["nan", "nan", "few_sites"], ["nan", "nan", "few_sites"], ["0.500000", "nan", "few_sites"]]
    assert MO.flag_of(0, st, *MO.nesting(st), min_called=0) == "none"      # nan compares false: no flag from an empty part


def flags(own, shared, outside=None, **kw):
    st = stats_of(own, shared)
    nest = MO.nesting(st)
    for i, three in (outside or {}).items():
        st.outside[i] = three
    return [MO.flag_of(i, st, *nest, **kw) for i in range(len(st))]


def test_every_flag_with_its_precedence_and_both_sides_of_each_threshold():
    child = {(0, 1): (49, 1, 0)}
    # carried_by_children: outside 15 / 85 = 0.15, inside 49 / 50
    assert flags([(64, 86, 0), (49, 1, 0)], child, {0: (15, 85, 0)}) == ["carried_by_children", "none"]
    # --max_outside: at the threshold it applies, just above it does not
    assert flags([(79, 71, 0), (49, 1, 0)], child, {0: (30, 70, 0)})[0] == "carried_by_children"
    assert flags([(80, 70, 0), (49, 1, 0)], child, {0: (31, 69, 0)})[0] == "none"
    # --min_frac on the inside: 35 / 50 = 0.7 applies, 34 / 50 does not
    assert flags([(50, 100, 0), (35, 15, 0)], {(0, 1): (35, 15, 0)}, {0: (15, 85, 0)})[0] == "carried_by_children"
    assert flags([(49, 101, 0), (34, 16, 0)], {(0, 1): (34, 16, 0)}, {0: (15, 85, 0)})[0] == "none"
    # --min_called on the outside part: 20 called applies, 19 does not
    assert flags([(52, 18, 0), (49, 1, 0)], child, {0: (3, 17, 0)})[0] == "carried_by_children"
    assert flags([(52, 17, 0), (49, 1, 0)], child, {0: (3, 16, 0)})[0] == "none"
    # submotif: the parent outside this motif is 97 / 100; at 0.7 it applies, below it does not; fewer than 20 called there: not judged
    assert flags([(146, 4, 0), (49, 1, 0)], child, {0: (97, 3, 0)}) == ["none", "submotif"]
    assert flags([(119, 31, 0), (49, 1, 0)], child, {0: (70, 30, 0)})[1] == "submotif"
    assert flags([(118, 32, 0), (49, 1, 0)], child, {0: (69, 31, 0)})[1] == "none"
    assert flags([(68, 1, 0), (49, 1, 0)], child, {0: (19, 0, 0)})[1] == "none" and flags([(69, 1, 0), (49, 1, 0)], child, {0: (20, 0, 0)})[1] == "submotif"
    # few_sites goes before everything: a duplicate, a carried parent and a sub-motif below --min_called are few_sites
    assert flags([(10, 9, 50), (10, 9, 50)], {(0, 1): (10, 9, 50)}) == ["few_sites", "few_sites"]
    assert flags([(10, 10, 0), (10, 10, 0)], {(0, 1): (10, 10, 0)}) == ["none", "duplicate"]          # the EARLIER motif keeps its flag
    assert flags([(146, 4, 0), (10, 9, 0)], {(0, 1): (10, 9, 0)})[1] == "few_sites"
    # duplicate goes before carried_by_children and submotif: motifs 1 and 2 are identical children of a methylated parent
    three = flags([(146, 4, 0), (49, 1, 0), (49, 1, 0)], {(0, 1): (49, 1, 0), (0, 2): (49, 1, 0), (1, 2): (49, 1, 0)}, {0: (97, 3, 0)})
    assert three == ["none", "submotif", "duplicate"]
    # carried_by_children goes before submotif: a motif between a methylated grandparent and its own child
    own = [(300, 100, 0), (64, 86, 0), (49, 1, 0)]                        # the grandparent outside motif 1: 236 / 250
    mid = flags(own, {(0, 1): (64, 86, 0), (0, 2): (49, 1, 0), (1, 2): (49, 1, 0)}, {1: (15, 85, 0)})
    assert mid[1] == "carried_by_children" and flags(own, {(0, 1): (64, 86, 0), (0, 2): (49, 1, 0), (1, 2): (49, 1, 0)}, {1: (60, 40, 0)})[1] == "submotif"
    # the thresholds are arguments
    assert flags([(64, 86, 0), (49, 1, 0)], child, {0: (15, 85, 0)}, max_outside=0.1)[0] == "none"
    assert flags([(146, 4, 0), (49, 1, 0)], child, {0: (97, 3, 0)}, min_frac=0.98)[1] == "none"
    assert flags([(146, 4, 0), (49, 1, 0)], child, {0: (97, 3, 0)}, min_called=51) == ["none", "few_sites"]
    assert set(MO.FLAGS) == {"few_sites", "duplicate", "carried_by_children", "submotif", "none"}


def test_children_that_overlap_each_other_need_the_union():
    """GATCH and DGATC inside GATC share most of their sites: the parent outside BOTH is what call 2 returns, not own - a - b."""
    bf = G.BruteForce()
    ms = G.A_SET[:4]
    tables = [bf.table("b0", "a", m, ms[:i] + ms[i + 1:]) for i, m in enumerate(ms)]
    st = MO.set_stats(tables)
    children = MO.nesting(st)[0]
    assert children[0] == [1, 2, 3] and children[2] == children[3] == [1]
    MO.add_outside(st, children, {i: bf.table("b0", "a", ms[i], [ms[j] for j in children[i]]) for i in (0, 2, 3)})
    naive = st.own[0] - st.shared[0, 2] - st.shared[0, 3]
    assert (st.outside[0] >= 0).all() and naive.min() < 0 and st.outside[0].sum() == st.own[0].sum() - (st.shared[0, 2] + st.shared[0, 3] - st.shared[2, 3]).sum()
    with pytest.raises(RuntimeError, match="does not belong"):
        MO.add_outside(st, children, {0: bf.table("b0", "a", ms[1], [ms[j] for j in children[0]])})


def test_the_symmetry_check_trips_on_a_doctored_table():
    bf = G.BruteForce()
    tables = bf.all_others("b0", "a")
    names = [f"{G.to_iupac(m)}_a_{p}" for m, p in G.A_SET]
    MO.set_stats(tables, names)                                          # symmetric as it comes
    bad = [t.copy() for t in tables]
    bad[1][1, 1, 0, 2] += 1                                              # RGATCY's share with GATC, contig `long`, fwd nocall
    bad[1][1, 1, 1, 2] -= 1                                              # ... moved to the other strand: the pooled numbers still agree
    with pytest.raises(RuntimeError, match=r"not symmetric: GATC_a_1 shares .* with RGATCY_a_2"):
        MO.set_stats(bad, names)
    with pytest.raises(ValueError, match="blocks for a set of"):
        MO.set_stats([t[:-1] for t in tables], names)
