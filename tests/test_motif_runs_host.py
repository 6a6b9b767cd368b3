"""Host side of ``motif_runs`` (no GPU): that every case the geometry input of ``runs_geometry`` was built for is really in it — counted
on the brute force's output —, the Wald-Wolfowitz numbers on hand-computed sequences, the flag rule, ``motif_runs.format_files`` byte for
byte on hand-made tables, the parsers with their refusals and the command's parser spec."""
import math
import os

import numpy as np
import pytest

import runs_geometry as rn
from nanomotif_amd import motif_runs as mr
from nanomotif_amd.argparser import create_parser
from nanomotif_amd.motif_sites import SiteCandidate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = rn.CHUNK
GATC1, A1, C1, G2_1, G3_1 = ("b1", "a", "GATC", 1), ("b1", "a", "A", 0), ("b1", "m", "C", 0), ("b1", "a", "A" + "." * 40 + "C", 0), ("b1", "a", "A" + "." * 70 + "T", 0)
GATC2, A2, C2, G2_2, G3_2 = (("b2",) + c[1:] for c in (GATC1, A1, C1, G2_1, G3_1))
A_CANDS_1, A_CANDS_2 = (GATC1, A1, G2_1, G3_1), (GATC2, A2, G2_2, G3_2)


def elements(cand, contig, nocall_breaks=False):
    """[(position, state)] of the sequence of a candidate on a contig."""
    return [(p, st) for n, p, _, st in rn.sites_of(cand) if n == contig and (nocall_breaks or st != 2)]


def runs(cand, contig, nocall_breaks=False):
    return rn.runs_in(rn.sites_of(cand), [contig], nocall_breaks)[contig]


def run_over(cand, contig, a, b, nocall_breaks=False):
    """The runs whose consecutive elements sit on positions a and b."""
    el = [p for p, _ in elements(cand, contig, nocall_breaks)]
    if a not in el or b not in el or el.index(b) != el.index(a) + 1:
        return []
    return [r for r in runs(cand, contig, nocall_breaks) if r[2] <= a and r[3] >= b]


# ------------------------------------------------------------------------------------------------ 1. the input
def test_the_input_is_small_and_complete():
    seqs, piles = rn.geometry()
    assert sum(rn.LENGTHS.values()) < 200_000 and max(rn.LENGTHS.values()) <= 4 * CHUNK and (rn.LENGTHS["one"], rn.LENGTHS["odd"]) == (8192, 8213)
    assert [len(seqs[n]) for n in rn.NAMES] == [rn.LENGTHS[n] for n in rn.NAMES] and rn.LENGTHS["small"] == 92
    assert len(rn.candidates()) == 12 and {c[0] for c in rn.candidates()} == {"b1", "b2"} and {c[1] for c in rn.candidates()} == {"a", "m"}
    assert "b0_empty" in rn.BIN_NAMES and not rn.contigs_of("b0_empty")
    for c in rn.candidates():                                             # every candidate has mod and nomod runs
        t = rn.expected_table(c, 16, False)
        assert (t[:, :2, 0].sum(axis=0) > 0).all(), c


def test_every_planted_case_is_present():
    # ---- borders a run crosses: consecutive elements on 31 | 32, 127 | 128, 8191 | 8192
    for cand in (GATC1, A1):
        for a in (31, 127, CHUNK - 1):
            assert len(run_over(cand, "long", a, a + 1)) == 1, (cand, a)
    # a run over three chunks with the middle chunk uniform: chunk 1 has elements, all in one run that began before and goes on after
    for cand in A_CANDS_1 + (C1,):
        over = [r for r in runs(cand, "long") if r[2] < CHUNK and r[3] >= 2 * CHUNK]
        inside = [p for p, _ in elements(cand, "long") if CHUNK <= p < 2 * CHUNK]
        assert len(over) == 1 and over[0][0] == 1 and len(inside) >= 1 and all(over[0][2] < p < over[0][3] for p in inside), cand
    # a run that starts as a chunk's only element and ends as the next chunk's head
    for cand, p in ((GATC2, rn.ONLY[1] + 1), (A2, rn.ONLY[1] + 1), (C2, rn.ONLY[1] + 3)):
        el = elements(cand, "p3")
        assert [q for q, _ in el if CHUNK <= q < 2 * CHUNK] == [p], cand
        mine = [r for r in runs(cand, "p3") if r[2] == p]
        assert len(mine) == 1 and mine[0][3] >= 2 * CHUNK and mine[0][1] >= 2 and len(rn.sites_of(cand)) > 1, cand
    # ---- chunks without elements
    for cand in A_CANDS_2:
        for contig in ("j3", "d3"):                                       # no occurrence at all in chunk 1
            assert not [1 for n, p, _, _ in rn.sites_of(cand) if n == contig and CHUNK <= p < 2 * CHUNK], (cand, contig)
        assert len([r for r in runs(cand, "j3") if r[2] < CHUNK and r[3] >= 2 * CHUNK]) == 1, cand          # same state either side: they join
        before, after = [e for e in elements(cand, "d3") if e[0] < CHUNK][-1], [e for e in elements(cand, "d3") if e[0] >= 2 * CHUNK][0]
        assert (before[1], after[1]) == (0, 1), cand                      # different states: a run ends, another begins
        # nocall sites only in chunk 1: joins by default, breaks under nocall_breaks
        inside = [st for n, p, _, st in rn.sites_of(cand) if n == "n3" and CHUNK <= p < 2 * CHUNK]
        assert len(inside) >= 1 and set(inside) == {2}, cand
        assert len([r for r in runs(cand, "n3") if r[2] < CHUNK and r[3] >= 2 * CHUNK]) == 1, cand
        nb = runs(cand, "n3", True)
        assert not [r for r in nb if r[2] < CHUNK and r[3] >= 2 * CHUNK] and [r for r in nb if r[0] == 2 and CHUNK <= r[2] and r[3] < 2 * CHUNK], cand
    # ---- contig borders and small contigs
    names = rn.contigs_of("b1")
    assert names.index("odd") == names.index("one") + 1
    for cand in (GATC1, A1, C1, G2_1):
        assert runs(cand, "one")[-1][0] == runs(cand, "odd")[0][0] == 0, cand       # one state either side of a contig border
    assert len([1 for n, _, _, _ in rn.sites_of(G2_1) if n == "small"]) == 1 and len([1 for n, _, _, _ in rn.sites_of(A1) if n == "small"]) == 1
    assert runs(G2_1, "small") == [(0, 1, 10, 10)]
    for cand in A_CANDS_1:
        assert not [1 for n, _, _, _ in rn.sites_of(cand) if n == "bare"], cand     # a contig without a site
    assert [1 for n, _, _, _ in rn.sites_of(C1) if n == "bare"]
    assert any(r[2] < CHUNK <= r[3] for r in runs(A1, "odd"))             # into the last chunk of 21 bp
    # ---- dense sequences
    n, s, e = rn.POLY_MOD
    poly = [r for r in runs(A1, n) if r[2] <= s and r[3] >= e - 1]
    assert len(poly) == 1 and poly[0][0] == 0 and poly[0][1] >= 300 and s < 3072 < 3200 < e       # over two lane borders
    n, s, e = rn.POLY_ALT
    alt = [r for r in runs(A1, n) if s <= r[2] < e]
    assert len(alt) == 300 and all(r[1] == 1 for r in alt) and len([r for r in alt if 27 * 128 <= r[2] < 28 * 128]) == 128
    n, s, e = rn.GATC_ARRAY
    arr = [(p, strand) for c, p, strand, _ in rn.sites_of(GATC1) if c == n and s <= p < e]
    assert len(arr) == 200 and all(arr[2 * j] == (s + 4 * j + 1, 0) and arr[2 * j + 1] == (s + 4 * j + 2, 1) for j in range(100))
    assert len({st for c, p, _, st in rn.sites_of(GATC1) if c == n and s <= p < e}) == 3
    # ---- run lengths at the bucket and record thresholds: R - 1, R, R + 1 for R = 2, 16, 64; min_run - 1, min_run
    in_a = [r[1] for r in runs(A1, "one") if r[0] == 0 and rn.LENGTH_A[1] <= r[2] < rn.LENGTH_A[1] + sum(rn.RUN_LENGTHS) + 8]
    assert in_a == list(rn.RUN_LENGTHS) and {2, 3} <= set(in_a)
    in_g = [r[1] for r in runs(GATC1, "one") if r[0] == 0 and rn.LENGTH_GATC[1] <= r[2] < rn.LENGTH_GATC[1] + 520]
    assert in_g == list(rn.RUN_LENGTHS[3:])
    # ---- a position called both ways is mod
    _, piles = rn.geometry()
    for mt, cand in (("a", A1), ("m", C1)):
        rows = piles[(mt, "one")]
        both = {(p, s) for p, s, f in rows if f >= 0.7} & {(p, s) for p, s, f in rows if f <= 0.3}
        assert {p for p, _ in both} == {p for _, p in rn.BOTH_WAYS}
        hit = [st for n, p, s, st in rn.sites_of(cand) if n == "one" and (p, s) in both]
        assert len(hit) >= 5 and set(hit) == {0}, cand
    # ---- the record order head, interior, tail: a qualifying run (nomod, >= 3 sites) that starts in chunk 0 and ends in chunk 2, with
    # qualifying runs before it in the chunk it starts in and after it in the chunk it ends in
    for cand in (A1, GATC1):
        q = [r for r in runs(cand, "long") if r[0] == 1 and r[1] >= 3]
        big = [r for r in q if r[2] < CHUNK and r[3] >= 2 * CHUNK][0]
        assert [r for r in q if r[3] < big[2]] and [r for r in q if r[2] > big[3] and r[2] < 3 * CHUNK], cand


# ------------------------------------------------------------------------------------------------ 2. the runs test
def test_runs_test_on_hand_computed_sequences():
    # MMMMUUUU: n1 = n2 = 4, mu = 1 + 2 * 16 / 8 = 5, var = 2 * 16 * (32 - 8) / (64 * 7) = 12 / 7; R = 2: z = -3 / sqrt(12 / 7) = -2.291288
    assert mr.runs_terms(4, 4) == (5.0, pytest.approx(12 / 7, abs=1e-12))
    assert mr.runs_z(4, 4, 2) == pytest.approx(-2.2912878, abs=1e-6)
    # MUMUMUMU: R = 8, z = +2.291288
    assert mr.runs_z(4, 4, 8) == pytest.approx(2.2912878, abs=1e-6)
    assert mr.runs_terms(5, 0) == mr.runs_terms(0, 3) == mr.runs_terms(0, 0) == (0.0, 0.0) and mr.runs_z(5, 0, 1) == 0.0
    # two contigs MMMMUUUU and one of a single outcome, which is left out: (4 - 10) / sqrt(24 / 7) = -3.240370
    assert mr.runs_z_within([(4, 4, 2), (5, 0, 1), (4, 4, 2)]) == pytest.approx(-3.2403703, abs=1e-6)
    assert mr.runs_z_within([(5, 0, 1), (0, 7, 1)]) == 0.0 and mr.runs_z_within([]) == 0.0
    # a contaminant contig of another methylation level: pooled as one sequence it looks clustered, within the contigs it does not
    rows = [(50, 50, 51), (100, 0, 1)]
    assert mr.runs_z(150, 50, 52) < -3.0 and abs(mr.runs_z_within(rows)) < 0.1


def test_each_flag_and_the_thresholds_themselves():
    assert mr.flag_of(19, -9.0) == "few_sites" and mr.flag_of(20, -9.0) == "clustered" and mr.flag_of(20, 9.0) == "alternating"
    assert mr.flag_of(20, -5.0) == "clustered" and mr.flag_of(20, 5.0) == "alternating"          # exactly on the threshold
    assert mr.flag_of(20, -4.999) == mr.flag_of(20, 4.999) == mr.flag_of(20, 0.0) == "none"
    assert mr.flag_of(30, -3.0, min_called=31) == "few_sites" and mr.flag_of(30, -3.0, min_z=3.0) == "clustered"
    assert mr.FLAGS == ("none", "clustered", "alternating", "few_sites")


def row(mod, nomod, nocall=(0, 0, 0), hist=None, r=4):
    """int64[3, 3 + r] from (runs, sites, longest) per state and {(state, length): runs}."""
    t = np.zeros((3, 3 + r), dtype=np.int64)
    for s, v in enumerate((mod, nomod, nocall)):
        t[s, :3] = v
    for (s, length), n in (hist or {}).items():
        t[s, 3 + min(length, r) - 1] += n
    return t


# ------------------------------------------------------------------------------------------------ 3. the files
def test_the_four_files_byte_for_byte():
    cands = [SiteCandidate("b1", "GATC", "a", 1), SiteCandidate("b1", "CCWGG", "m", 1)]
    names = ["k1", "k2\x00b1"]
    # GATC: k1 = 30 M then 30 U (2 runs), k2 = 5 M; CCWGG: MUMU on k1
    t0 = np.stack([row((1, 30, 30), (1, 30, 30), (0, 4, 0), {(0, 30): 1, (1, 30): 1}), row((1, 5, 5), (0, 0, 0), hist={(0, 5): 1})])
    t1 = np.stack([row((2, 2, 1), (2, 2, 1), hist={(0, 1): 2, (1, 1): 2}), row((0, 0, 0), (0, 0, 0))])
    bg = np.stack([row((100, 200, 7), (100, 200, 9), (0, 50, 0), {(0, 2): 100, (1, 2): 100}), row((3, 4, 2), (2, 2, 1), hist={(0, 1): 2, (0, 2): 1, (1, 1): 2})])
    main, per_contig, hist, per_bin = mr.format_files(cands, [(names, t0), (names, t1)], [("b1", "a")], [(names, bg)])
    z = lambda a, b, c: "%.3f" % mr.runs_z(a, b, c)
    p = lambda zz: "%.3e" % math.erfc(abs(zz) / math.sqrt(2.0))
    # k1 by hand: mu = 1 + 2 * 900 / 60 = 31, var = 1800 * 1740 / (3600 * 59) = 14.745763, z = -29 / 3.840021 = -7.552
    zk1 = mr.runs_z(30, 30, 2)
    assert "%.3f" % zk1 == "-7.552"
    bgz = "%.3f" % mr.runs_z_within([(200, 200, 200), (4, 2, 5)])
    head = ("bin\tmotif\tmod_type\tmod_position\tn_mod\tn_nomod\tn_nocall\tfrac_mod\truns_mod\truns_nomod\tlongest_mod\tlongest_nomod\tmean_run_mod\tmean_run_nomod\t"
            "expected_runs\truns_z\truns_z_within\truns_p\tbg_runs_z_within\tflag\n")
    assert main == head + (
        f"b1\tGATC\ta\t1\t35\t30\t4\t0.538462\t2\t1\t30\t30\t17.500\t30.000\t{'%.3f' % (1 + 2 * 35 * 30 / 65)}\t{z(35, 30, 3)}\t-7.552\t{p(zk1)}\t{bgz}\tclustered\n"
        f"b1\tCCWGG\tm\t1\t2\t2\t0\t0.500000\t2\t2\t1\t1\t1.000\t1.000\t3.000\t{z(2, 2, 4)}\t{z(2, 2, 4)}\t{p(mr.runs_z(2, 2, 4))}\t\tfew_sites\n")
    chead = head.replace("mod_position\t", "mod_position\tcontig\t")
    assert per_contig == chead + (
        f"b1\tGATC\ta\t1\tk1\t30\t30\t4\t0.500000\t1\t1\t30\t30\t30.000\t30.000\t31.000\t-7.552\t-7.552\t{p(zk1)}\t{bgz}\tclustered\n"
        f"b1\tGATC\ta\t1\tk2\t5\t0\t0\t1.000000\t1\t0\t5\t0\t5.000\t\t0.000\t0.000\t0.000\t1.000e+00\t{bgz}\tfew_sites\n"
        f"b1\tCCWGG\tm\t1\tk1\t2\t2\t0\t0.500000\t2\t2\t1\t1\t1.000\t1.000\t3.000\t{z(2, 2, 4)}\t{z(2, 2, 4)}\t{p(mr.runs_z(2, 2, 4))}\t\tfew_sites\n"
        "b1\tCCWGG\tm\t1\tk2\t0\t0\t0\t\t0\t0\t0\t0\t\t\t0.000\t0.000\t0.000\t1.000e+00\t\tfew_sites\n")
    assert hist == ("bin\tmotif\tmod_type\tmod_position\tstate\trun_length\truns\n"
                    "b1\tGATC\ta\t1\tmod\t4+\t2\nb1\tGATC\ta\t1\tnomod\t4+\t1\nb1\tCCWGG\tm\t1\tmod\t1\t2\nb1\tCCWGG\tm\t1\tnomod\t1\t2\n")
    assert per_bin == head + f"b1\tA\ta\t0\t204\t202\t50\t0.502463\t103\t102\t7\t9\t1.981\t1.980\t{'%.3f' % (1 + 2 * 204 * 202 / 406)}\t{z(204, 202, 205)}\t{bgz}\t{p(mr.runs_z_within([(200, 200, 200), (4, 2, 5)]))}\t\tnone\n"
    assert mr.format_files(cands, [(names, t0), (names, t1)], [("b1", "a")], [(names, bg)]) == (main, per_contig, hist, per_bin)      # pure


def test_bed_text():
    from nanomotif_amd.engine import RUN_DTYPE
    rec = np.array([(0, 1, 7, 1, 40, 3), (1, 0, 0, 0, 0, 1), (1, 0, 9, 2, 12, 2)], dtype=RUN_DTYPE)
    cands = [SiteCandidate("b1", "GATC", "a", 1), SiteCandidate("b2", "CCWGG", "m", 1)]
    assert mr.format_runs(rec, cands, ["k0", "k1"]) == ("k1\t7\t41\tGATC_a_1\t3\t.\tnomod\tb1\nk0\t0\t1\tCCWGG_m_1\t1\t.\tmod\tb2\nk0\t9\t13\tCCWGG_m_1\t2\t.\tnocall\tb2\n")
    assert mr.format_runs(rec[:0], cands, ["k0", "k1"]) == ""


# ------------------------------------------------------------------------------------------------ 4. the parsers, the bindings
def test_parsers_and_their_refusals():
    from nanomotif_amd import engine
    assert mr.parse_max_run("2") == 2 and mr.parse_max_run(" 64 ") == 64 and mr.parse_min_run("1") == 1 and mr.parse_min_run("1000") == 1000
    for bad in ("1", "65", "x", "3.5"):
        with pytest.raises(ValueError, match="--max_run"):
            mr.parse_max_run(bad)
    for bad in ("0", "-1", "x"):
        with pytest.raises(ValueError, match="--min_run"):
            mr.parse_min_run(bad)
    assert mr.parse_run_states("nomod, mod") == ("mod", "nomod")
    with pytest.raises(ValueError):
        mr.parse_run_states("x")
    assert engine.run_state_set(("nomod",)) == 2 and engine.run_state_set(("mod", "nomod", "nocall"), True) == 7
    with pytest.raises(ValueError, match="nocall_breaks"):
        engine.run_state_set(("nocall",))
    for bad in ((), ("x",)):
        with pytest.raises(ValueError):
            engine.run_state_set(bad, True)
    assert engine.run_length_limit(2) == 2 and engine.run_length_limit(64) == 64
    for bad in (1, 65, 2.5):
        with pytest.raises(ValueError):
            engine.run_length_limit(bad)


def test_parser_spec_of_motif_runs(capsys):
    sub = create_parser()._subparsers._group_actions[0].choices
    p = sub["motif_runs"]
    spec = {a.dest: (list(a.option_strings), a.default, a.required, type(a).__name__) for a in p._actions}
    assert [a.dest for a in p._actions if not a.option_strings] == ["assembly", "pileup"]
    assert [[g.required, [a.dest for a in g._group_actions]] for g in p._mutually_exclusive_groups] == [[True, ["contig_bin", "files", "directory"]]]
    assert spec["bin_motifs"][2] is True and spec["max_run"][1] == 16 and spec["min_run"][1] == 3 and spec["states"][1] == ("nomod",)
    assert (spec["min_called"][1], spec["min_z"][1]) == (20, 5.0)
    assert spec["runs"][3] == spec["nocall_breaks"][3] == "_StoreTrueAction"
    gc = {a.dest for a in sub["motif_gc"]._actions} - {"half", "gc_bins", "min_delta"}
    assert gc <= set(spec)                                                # everything the export commands share
    base = ["motif_runs", "a.fa", "p.bed", "-c", "cb.tsv", "--bin_motifs", "m.tsv", "n.tsv"]
    args = create_parser().parse_args(base + ["--max_run", "64", "--nocall_breaks", "--runs", "--states", "nocall,mod", "--min_run", "1"])
    assert (args.max_run, args.nocall_breaks, args.runs, args.states, args.min_run, args.bin_motifs) == (64, True, True, ("mod", "nocall"), 1, ["m.tsv", "n.tsv"])
    args = create_parser().parse_args(base)
    assert (args.max_run, args.nocall_breaks, args.runs, args.states, args.min_run) == (16, False, False, ("nomod",), 3)
    for bad in (base + ["--max_run", "1"], base + ["--max_run", "65"], base + ["--min_run", "0"], base + ["--states", "x"], base[:5]):
        with pytest.raises(SystemExit):
            create_parser().parse_args(bad)
    capsys.readouterr()


def test_exports_are_declared_bound_and_built():
    from nanomotif_amd import _lib, build, engine
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    for name in ("nm_motif_runs_count", "nm_motif_runs_sites"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS
    assert "#define NM_RUNS_MIN_MAX_RUN 2" in header and "#define NM_RUNS_MAX_MAX_RUN 64" in header
    assert (engine.RUNS_MIN_MAX_RUN, engine.RUNS_MAX_MAX_RUN) == (2, 64)
    assert any(os.path.basename(s) == "nmruns.hip" for s in build.SRC_HIP)
    assert engine.RUN_DTYPE.names == engine.SITE_DTYPE.names + ("last", "n_sites") and engine.RUN_DTYPE.itemsize == engine.SITE_DTYPE.itemsize + 8
    assert "nm_abi_version" in header
