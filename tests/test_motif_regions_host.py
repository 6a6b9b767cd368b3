"""Host side of ``motif_regions`` (no GPU): the conditions on the geometry input of ``regions_geometry``, the BED / GFF3 readers of
``nanomotif_amd/regions.py``, the piece cuts of the rasteriser restated, ``motif_regions.format_files`` byte for byte on hand-made tables
with the flag rule at its four outcomes and on its thresholds, the interval join against a per-interval brute force, and the command's
parser spec."""
import gzip
import math
import os

import numpy as np
import pytest

import regions_geometry as rg
from nanomotif_amd import motif_regions as mr
from nanomotif_amd import regions
from nanomotif_amd.argparser import create_parser
from nanomotif_amd.motif_sites import SiteCandidate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the input
def test_the_input_is_not_degenerate():
    seqs, piles, planted = rg.geometry()
    assert [len(seqs[n]) for n in rg.NAMES] == [92, 8192, 8213, 700, 16684] and rg.LONG % 32 != 0
    assert rg.INTERVALS != sorted(rg.INTERVALS) and sorted(rg.INTERVALS) == sorted(rg._ORDERED)          # given unsorted
    listed = {(0, 1), (31, 32), (31, 33), (32, 33), (0, 32), (0, 33), (127, 129), (8191, 8193), (8192, 16384), (rg.LONG - 1, rg.LONG)}
    assert listed <= {(s, e) for n, s, e, _ in rg.INTERVALS if n == "long"}
    assert {("small", 0, 92), ("one", 0, 8192), ("odd", 0, 8213)} <= {(n, s, e) for n, s, e, _ in rg.INTERVALS}
    assert not any(n == "gap" for n, _, _, _ in rg.INTERVALS) and rg.NAMES.index("odd") < rg.NAMES.index("gap") < rg.NAMES.index("long")
    five = [(s, e) for n, s, e, c in rg._ORDERED if c == 5 and n == "long"]
    assert five.count((300, 400)) == 2 and (500, 700) in five and (550, 600) in five and (800, 900) in five and (850, 950) in five
    assert (1000, 1100) in five and (1100, 1200) in five
    ones = [(s, e) for s, e in five if e - s == 1 and 1280 <= s < 1312]
    assert len(ones) == 200 and len(set(ones)) == 11 and len({s // 32 for s, _ in ones}) == 1
    sets = rg.class_sets(*rg.region_set(8))
    assert all(4000 in sets[("long", c)] for c in range(8)) and sets[("long", 6)] >= set(range(2000, 2100)) <= sets[("long", 7)]
    assert any(s < rg.CHUNK and e > 2 * rg.CHUNK for n, s, e, _ in rg.INTERVALS)      # one interval over all three chunks of a contig
    sets3 = rg.class_sets(*rg.region_set(3))
    assert not any(sets3[(n, 2)] for n in rg.NAMES) and any(sets3[(n, 1)] for n in rg.NAMES)           # a declared class without an interval
    # the planted GATC sites: every border kind on both strands in all three states, each where it was meant to be
    gatc = {(n, p, s): st for n, p, s, st in rg.sites_of(("b1", "a", "GATC", 1))}
    assert len(planted) == 24 and len(set(planted)) == 24
    for (kind, strand, state, q), (_, s, e, _) in zip(planted, rg.PLANTED):
        assert gatc[("one", q, strand)] == state and q == {"first": s, "last": e - 1, "before": s - 1, "end": e}[kind]
        assert (q in sets[("one", rg.PLANT_CLASS)]) == (kind in ("first", "last"))
    assert {(k, s, st) for k, s, st, _ in planted} == {(k, s, st) for k in rg.KINDS for s in (0, 1) for st in (0, 1, 2)}
    # every motif has sites on both strands in all three states, inside a class and outside all of them; the G = 2 and G = 3 motifs
    # reach over a chunk border
    for cand in rg.candidates():
        t = rg.expected_table(cand, sets, 8)
        assert (t[:, :8].sum(axis=(0, 1)) > 0).all() and (t[:, 8].sum(axis=0) > 0).all() or cand[0] == "b2" and cand[2] in ("GATC", "CC[AT]GG"), cand
    # with a background every position of a class is a site
    a, c = rg.sites_of(("b1", "a", "A", 0)), rg.sites_of(("b1", "m", "C", 0))
    assert {(n, p) for n, p, _, _ in a + c} == {(n, p) for n in rg.contigs_of("b1") for p in range(rg.LENGTHS[n])}


# the states a listed border of ``long`` sees at its positions s - 1, s, e - 1, e: all three wherever three positions allow it
BORDER_STATES = {(0, 1): {0, 1}, (31, 32): {0, 1, 2}, (31, 33): {0, 1, 2}, (32, 33): {0, 1, 2}, (0, 32): {0, 1}, (0, 33): {0, 1, 2}, (127, 129): {0, 1, 2},
                 (8191, 8193): {0, 1, 2}, (8192, 16384): {0, 1, 2}, (rg.LONG - 1, rg.LONG): {0, 1}}


@pytest.mark.parametrize("border", sorted(BORDER_STATES))
def test_every_listed_border_is_hit_by_sites_of_its_states(border):
    """Per listed border [s, e) of ``long``: each of s - 1, s, e - 1, e inside the contig carries exactly ONE site of the one-letter
    backgrounds (a position holds one letter, so one (mod type, strand) and one state), in the state ``regions_geometry.FORCED`` gives
    it, the base before and the base ``end`` are outside the interval's class and its first and last base inside, and the states seen
    are exactly those written above.  Three states at one border need three positions: [0,1) and [L-1,L) have two; and as [32,33)
    takes 31, 32, 33 in three different states, position 0 cannot differ from 31 and 32 AND from 32 and 33 — [0,32) sees two states,
    [0,33) three."""
    s, e = border
    sets = rg.class_sets(*rg.region_set(8))
    cls = next(c for n, s0, e0, c in rg.SPECIAL if (n, s0, e0) == ("long", s, e))
    by_pos = {}
    for cand in (("b1", "a", "A", 0), ("b1", "m", "C", 0)):
        for n, p, strand, state in rg.sites_of(cand):
            if n == "long":
                by_pos.setdefault(p, []).append((cand[1], strand, state))
    positions = sorted({p for p in (s - 1, s, e - 1, e) if 0 <= p < rg.LONG})
    seqs, _, _ = rg.geometry()
    for p in positions:
        assert by_pos[p] == [rg.SITE_OF_LETTER[seqs["long"][p]] + (rg.FORCED[p],)], (border, p)
        assert (p in sets[("long", cls)]) == (s <= p < e), (border, p)       # first and last base inside the class, the two beside them outside
    assert {by_pos[p][0][2] for p in positions} == BORDER_STATES[border]
    assert len(positions) == (2 if border in ((0, 1), (rg.LONG - 1, rg.LONG)) else 3 if border in ((31, 32), (32, 33), (0, 32), (0, 33)) else 4)


# ------------------------------------------------------------------------------------------------ 2. the readers
INDEX = {"c1": 0, "c2": 1, "c3\x00binB": 2, "c3": 3}
LENGTH = [1000, 50, 300, 300]


def write(tmp_path, name, text):
    path = str(tmp_path / name)
    with (gzip.open(path, "wt") if name.endswith(".gz") else open(path, "w")) as f:
        f.write(text)
    return path


def as_rows(r):
    return list(zip(r.contig.tolist(), r.start.tolist(), r.end.tolist(), [r.class_names[c] for c in r.cls.tolist()], r.strand, r.names))


def test_bed_with_three_four_and_six_columns(tmp_path):
    r = regions.read_regions(write(tmp_path, "a.bed", "track name=x\n#c\nc1\t0\t10\nc2\t5\t50\n\n"), INDEX, LENGTH)
    assert r.class_names == ["region"] and as_rows(r) == [(0, 0, 10, "region", ".", "c1:0-10"), (1, 5, 50, "region", ".", "c2:5-50")]
    r = regions.read_regions(write(tmp_path, "b.bed", "c1\t0\t10\tphage\nc1\t7\t9\tgene\nc1\t20\t30\tphage\n"), INDEX, LENGTH)
    assert r.class_names == ["phage", "gene"] and r.cls.tolist() == [0, 1, 0] and r.strand == [".", ".", "."]
    r = regions.read_regions(write(tmp_path, "c.bed", "c1\t0\t10\tg\t0\t-\nc3\t1\t2\tg\t0\t+\n"), INDEX, LENGTH)
    # a contig placed in two bins takes the interval on both placements
    assert as_rows(r) == [(0, 0, 10, "g", "-", "c1:0-10"), (2, 1, 2, "g", "+", "c3:1-2"), (3, 1, 2, "g", "+", "c3:1-2")]
    assert r.contig.dtype == np.uint32 and r.start.dtype == r.end.dtype == np.uint64 and r.cls.dtype == np.uint8 and len(r) == 3


def test_only_keyword_lines_are_skipped_in_bed(tmp_path):
    index, length = {"track_12": 0, "browser2": 1, "c1": 2}, [100, 100, 100]
    text = "track name=x\nbrowser position c1:1-5\ntrack\ttype=bed\ntrack_12\t0\t10\nbrowser2\t1\t2\nc1\t3\t4\n"
    r = regions.read_regions(write(tmp_path, "t.bed", text), index, length)
    assert as_rows(r) == [(0, 0, 10, "region", ".", "track_12:0-10"), (1, 1, 2, "region", ".", "browser2:1-2"), (2, 3, 4, "region", ".", "c1:3-4")]


def test_the_command_refuses_its_annotation_before_anything_is_loaded(tmp_path, monkeypatch, caplog):
    import argparse

    def opened(*a, **k):
        raise AssertionError("the engine was opened before the annotation was read")
    monkeypatch.setattr(mr, "open_run", opened)
    base = dict(states=("mod",), classes=None, upstream=0, inside=None)
    nine = "".join(f"c1\t{k}\t{k + 1}\tk{k}\n" for k in range(9))
    for name, text, more, what in (("bad.bed", "c1\t5\t5\n", {}, "bad.bed:1: end 5 <= start 5"), ("nine.bed", nine, {}, "9 region classes"),
                                   ("ok.bed", "c1\t0\t5\tg\n", {"inside": ("h",)}, "classes: a non-empty selection of g, outside"),
                                   ("missing.bed", None, {}, "missing.bed")):
        path = write(tmp_path, name, text) if text is not None else str(tmp_path / name)
        caplog.clear()
        with caplog.at_level("ERROR"):
            assert mr.run(argparse.Namespace(regions=path, **{**base, **more})) == 2
        assert len(caplog.records) == 1 and what in caplog.records[0].getMessage(), name


def test_gff3_coordinates_names_and_gz(tmp_path):
    text = "##gff-version 3\nc1\tsrc\tgene\t1\t10\t.\t+\t.\tID=g1;Name=x\nc1\tsrc\tCDS\t11\t11\t.\t-\t0\tParent=g1\n##FASTA\n>c1\nACGT\n"
    for name in ("x.gff3", "x.gff.gz", "noext.txt", "y.gff"):
        r = regions.read_regions(write(tmp_path, name, text if name != "y.gff" else text.split("\n", 1)[1]), INDEX, LENGTH)
        assert as_rows(r) == [(0, 0, 10, "gene", "+", "g1"), (0, 10, 11, "CDS", "-", "c1:10-11")], name
    assert regions.is_gff("a.gff3.gz") and regions.is_gff("a.bed", "##gff-version 3") and not regions.is_gff("a.bed.gz", "c1\t0\t1")


def test_classes_select_and_order_and_nine_are_refused(tmp_path):
    nine = "".join(f"c1\t{10 * k}\t{10 * k + 5}\tk{k}\n" * (k + 1) for k in range(9))
    path = write(tmp_path, "nine.bed", nine)
    with pytest.raises(ValueError) as e:
        regions.read_regions(path, INDEX, LENGTH)
    assert "9 region classes, at most 8 fit" in str(e.value) and all(f"k{k} ({k + 1})" in str(e.value) for k in range(9))
    r = regions.read_regions(path, INDEX, LENGTH, classes=("k7", "k2", "absent"))
    assert r.class_names == ["k7", "k2", "absent"] and sorted(r.cls.tolist()) == [0] * 8 + [1] * 3
    assert regions.read_regions(path, INDEX, LENGTH, classes=[f"k{k}" for k in range(8)]).class_names == [f"k{k}" for k in range(8)]
    with pytest.raises(ValueError) as e:                                   # the added class counts against the eight
        regions.read_regions(path, INDEX, LENGTH, classes=[f"k{k}" for k in range(8)], upstream=5)
    assert "upstream (0)" in str(e.value)
    assert regions.parse_classes("b, a") == ("b", "a")
    for bad in ("", ",", "a,a"):
        with pytest.raises(ValueError):
            regions.parse_classes(bad)
    assert regions.parse_upstream("0") == 0 and regions.parse_upstream("50") == 50
    with pytest.raises(ValueError):
        regions.parse_upstream("-1")


@pytest.mark.parametrize("name, text, line, what", [
    ("a.bed", "c1\t0\t10\nc1\tx\t10\n", 2, "coordinate 'x'"), ("a.bed", "c1\t-1\t10\n", 1, "coordinate '-1'"), ("a.bed", "c1\t1.5\t10\n", 1, "coordinate"),
    ("a.bed", "c1\t0\t10\n\nc1\t10\t10\n", 3, "end 10 <= start 10"), ("a.bed", "c1\t12\t10\n", 1, "end 10 <= start 12"),
    ("a.bed", "c1\t0\t10\nc2\t0\t51\n", 2, "past the 50 positions of contig c2"), ("a.bed", "c1\t0\n", 1, "2 columns"),
    ("a.gff", "c1\ts\tgene\t0\t10\t.\t+\t.\tID=a\n", 1, "1-based"), ("a.gff", "##gff-version 3\nc1\ts\tgene\t5\t4\t.\t+\t.\tID=a\n", 2, "end 4 <= start 4"),
    ("a.gff", "c1\ts\tgene\t5\t1001\t.\t+\t.\tID=a\n", 1, "past the 1000 positions"), ("a.gff", "c1\ts\tgene\t5\n", 1, "4 columns")])
def test_bad_rows_name_file_and_line(tmp_path, name, text, line, what):
    path = write(tmp_path, name, text)
    with pytest.raises(ValueError) as e:
        regions.read_regions(path, INDEX, LENGTH)
    assert str(e.value).startswith(f"{path}:{line}: ") and what in str(e.value)


def test_dropped_contigs_give_one_warning_line(tmp_path, caplog):
    path = write(tmp_path, "d.bed", "zz\t0\t10\tg\nc1\t0\t10\tg\nzz\t5\t9999\tg\nyy\t1\t2\tg\n")
    with caplog.at_level("WARNING"):
        r = regions.read_regions(path, INDEX, LENGTH)
    assert len(r) == 1 and r.dropped == 3
    assert [rec.getMessage() for rec in caplog.records] == [f"{path}: 3 intervals on 2 contigs the assembly's bins do not hold; dropped"]


def test_upstream_on_both_strands_clipped_and_skipped(tmp_path):
    text = "c1\t100\t200\tg\t0\t+\nc1\t300\t400\tg\t0\t-\nc1\t20\t30\tg\t0\t+\nc1\t900\t980\tg\t0\t-\nc1\t500\t600\tg\t0\t.\nc1\t0\t5\tg\t0\t+\nc1\t990\t1000\tg\t0\t-\n" \
           "c1\t700\t710\tother\t0\t+\n"
    r = regions.read_regions(write(tmp_path, "u.bed", text), INDEX, LENGTH, classes=("g",), upstream=50)
    assert r.class_names == ["g", "upstream"]
    up = [(s, e, st, n) for _, s, e, c, st, n in as_rows(r) if c == "upstream"]
    assert up == [(50, 100, "+", "c1:100-200"), (400, 450, "-", "c1:300-400"), (0, 20, "+", "c1:20-30"), (980, 1000, "-", "c1:900-980")]
    assert sum(1 for x in as_rows(r) if x[3] == "g") == 7                 # the unstranded one, and the two at the contig's ends, add nothing
    assert regions.upstream_of(10, 20, ".", 100, 5) is None and regions.upstream_of(0, 20, "+", 100, 5) is None
    assert regions.read_regions(write(tmp_path, "v.bed", text), INDEX, LENGTH, upstream=0).class_names == ["g", "other"]


# ------------------------------------------------------------------------------------------------ 3. the piece cuts
def brute_pieces(s, e, p):
    """The plane words [s // 32, (e - 1) // 32] grouped by word // p: one piece per group."""
    return len({w // p for w in range(s // 32, (e - 1) // 32 + 1)})


def test_piece_cuts_restated():
    iv = rg._ORDERED
    for p in (1, 64, 2048):
        want = sum(brute_pieces(s, e, p) for _, s, e, _ in iv)
        assert regions.piece_count([s for _, s, _, _ in iv], [e for _, _, e, _ in iv], p) == want
    assert regions.piece_count([0], [1], 1) == 1 and regions.piece_count([31], [33], 1) == 2 and regions.piece_count([0], [8192], 64) == 4
    assert regions.piece_count([65535], [65537], 2048) == 2 and regions.piece_count([0], [65536], 2048) == 1
    counts = [regions.piece_count([s for _, s, _, _ in iv], [e for _, _, e, _ in iv], p) for p in (1, 64, 2048)]
    assert counts[0] > counts[1] > counts[2] == len(iv)                   # no contig of the input reaches a default piece border
    assert regions.PIECE_MAX_WORDS == 2048 and regions.MAX_CLASSES == 8


# ------------------------------------------------------------------------------------------------ 4. the files
def table(cells):
    """int64[1, K + 1, 2, 3] with the per-class (mod, nomod, nocall) on the forward strand."""
    t = np.zeros((1, len(cells), 2, 3), dtype=np.int64)
    t[0, :, 0, :] = cells
    return t


def test_two_proportion_z_by_hand():
    # 10 / 50 against 90 / 100: p = 100 / 150, var = (2 / 9) (1 / 50 + 1 / 100) = 1 / 150
    assert mr.two_proportion_z(10, 50, 90, 100) == pytest.approx((0.2 - 0.9) * math.sqrt(150), abs=1e-12)
    assert mr.two_proportion_z(0, 0, 5, 10) == 0.0 and mr.two_proportion_z(5, 10, 0, 0) == 0.0
    assert mr.two_proportion_z(10, 10, 20, 20) == 0.0 and mr.two_proportion_z(0, 10, 0, 20) == 0.0


def test_each_flag_and_the_thresholds_themselves():
    assert mr.flag_of(19, 100, 9.0, -0.5) == mr.flag_of(100, 19, 9.0, -0.5) == "few_sites"
    assert mr.flag_of(20, 20, -9.0, -0.5) == "depleted" and mr.flag_of(20, 20, 9.0, 0.5) == "enriched"
    assert mr.flag_of(20, 20, 4.999, 0.5) == mr.flag_of(20, 20, 9.0, 0.199) == mr.flag_of(20, 20, 9.0, None) == "none"
    assert mr.flag_of(20, 20, 5.0, 0.2) == "enriched" and mr.flag_of(20, 20, -5.0, -0.2) == "depleted"      # exactly on the thresholds
    assert mr.flag_of(30, 30, 3.0, 0.1, min_called=31) == "few_sites" and mr.flag_of(30, 30, 3.0, 0.1, min_z=3.0, min_delta=0.1) == "enriched"
    assert mr.FLAGS == ("none", "depleted", "enriched", "few_sites")


def test_the_three_files_byte_for_byte():
    cands = [SiteCandidate("b1", "GATC", "a", 1), SiteCandidate("b1", "CCWGG", "m", 1)]
    # classes island, gene; outside last.  GATC: island 10 / 50 called, everything else methylated
    t0 = np.concatenate([table([(10, 40, 5), (30, 0, 1), (60, 10, 2)]), table([(0, 0, 0), (0, 0, 0), (3, 1, 0)])])
    t0[0, 0, 1] = (0, 0, 2)
    six0 = np.array([[100, 50, 8, 0, 0, 2], [3, 1, 0, 0, 0, 0]])
    t1 = np.concatenate([table([(1, 1, 0), (0, 0, 0), (5, 5, 5)]), table([(0, 0, 0), (0, 0, 0), (0, 0, 0)])])
    six1 = np.array([[6, 6, 5, 0, 0, 0], [0, 0, 0, 0, 0, 0]])
    bg = np.concatenate([table([(100, 300, 10), (50, 50, 0), (500, 100, 0)]), table([(0, 0, 0), (0, 0, 0), (7, 3, 1)])])
    names = ["k1", "k2\x00b1"]
    covered = {"k1": np.array([2000, 500]), "k2\x00b1": np.array([0, 0])}
    main, per_contig, per_bin = mr.format_files(cands, [(names, t0), (names, t1)], [(names, six0), (names, six1)], [("b1", "a")], [(names, bg)], ["island", "gene"],
                                                covered, {"k1": 9000, "k2\x00b1": 1000})
    z = lambda a, b, c, d: "%.3f" % mr.two_proportion_z(a, b, c, d)
    p = lambda a, b, c, d: "%.3e" % math.erfc(abs(mr.two_proportion_z(a, b, c, d)) / math.sqrt(2.0))
    # island against the rest by hand: 0.2 - 93 / 104 = -0.694231; p = 103 / 154, var = p (1 - p) (1 / 50 + 1 / 104) = 0.0065596; z = -8.572
    assert z(10, 50, 93, 104) == "-8.572"
    head = "bin\tmotif\tmod_type\tmod_position\tclass\tn_mod\tn_nomod\tn_nocall\tfrac_mod\tfrac_mod_rest\tdelta\tz\tp\tbg_frac_mod\tsites_per_kbp\tflag\n"
    assert main == head + (
        f"b1\tGATC\ta\t1\tisland\t10\t40\t7\t0.200000\t0.894231\t-0.694231\t{z(10, 50, 93, 104)}\t{p(10, 50, 93, 104)}\t0.250000\t28.500\tdepleted\n"
        f"b1\tGATC\ta\t1\tgene\t30\t0\t1\t1.000000\t0.588710\t0.411290\t{z(30, 30, 73, 124)}\t{p(30, 30, 73, 124)}\t0.500000\t62.000\tnone\n"
        f"b1\tGATC\ta\t1\toutside\t63\t11\t2\t0.851351\t0.500000\t0.351351\t{z(63, 74, 40, 80)}\t{p(63, 74, 40, 80)}\t0.831148\t\tnone\n"
        "b1\tCCWGG\tm\t1\tisland\t1\t1\t0\t0.500000\t0.500000\t0.000000\t0.000\t1.000e+00\t\t1.000\tfew_sites\n"
        "b1\tCCWGG\tm\t1\tgene\t0\t0\t0\t\t0.500000\t\t0.000\t1.000e+00\t\t0.000\tfew_sites\n"
        "b1\tCCWGG\tm\t1\toutside\t5\t5\t5\t0.500000\t0.500000\t0.000000\t0.000\t1.000e+00\t\t\tfew_sites\n")
    assert float(z(30, 30, 73, 124)) < 5.0 < abs(float(z(10, 50, 93, 104))) and float(z(63, 74, 40, 80)) < 5.0
    chead = "bin\tmotif\tmod_type\tmod_position\tcontig\tclass\tfwd_mod\tfwd_nomod\tfwd_nocall\trev_mod\trev_nomod\trev_nocall\n"
    assert per_contig.startswith(chead + "b1\tGATC\ta\t1\tk1\tisland\t10\t40\t5\t0\t0\t2\nb1\tGATC\ta\t1\tk1\tgene\t30\t0\t1\t0\t0\t0\n")
    assert "b1\tGATC\ta\t1\tk2\toutside\t3\t1\t0\t0\t0\t0\n" in per_contig and per_contig.count("\n") == 1 + 2 * 2 * 3
    assert per_bin == ("bin\tmotif\tmod_type\tmod_position\tclass\tn_mod\tn_nomod\tn_nocall\tfrac_mod\tcovered_bp\tcovered_share\n"
                       "b1\tA\ta\t0\tisland\t100\t300\t10\t0.250000\t2000\t0.200000\nb1\tA\ta\t0\tgene\t50\t50\t0\t0.500000\t500\t0.050000\n"
                       "b1\tA\ta\t0\toutside\t507\t103\t1\t0.831148\t\t\n")
    # pure: the same arguments give the same text, and none was changed
    again = mr.format_files(cands, [(names, t0), (names, t1)], [(names, six0), (names, six1)], [("b1", "a")], [(names, bg)], ["island", "gene"], covered,
                            {"k1": 9000, "k2\x00b1": 1000})
    assert again == (main, per_contig, per_bin) and t0[0, 0, 1].tolist() == [0, 0, 2]


def test_sites_text_and_class_names():
    assert mr.class_text(0, ["a", "b", "c"]) == "outside" and mr.class_text(5, ["a", "b", "c"]) == "a,c"
    rec = np.array([(0, 1, 7, 0, 3), (0, 1, 7, 6, 0), (1, 0, 0, 1, 2)], dtype=[("candidate", "u4"), ("contig", "u4"), ("pos", "u4"), ("code", "u1"), ("classes", "u1")])
    cands = [SiteCandidate("b1", "GATC", "a", 1), SiteCandidate("b2", "CCWGG", "m", 1)]
    assert mr.format_sites(rec, cands, ["k0", "k1"], ["x", "y"]) == ("k1\t7\t8\tGATC_a_1\t0\t+\tmod\tb1\tx,y\nk1\t7\t8\tGATC_a_1\t0\t-\tnocall\tb1\toutside\n"
                                                                     "k0\t0\t1\tCCWGG_m_1\t0\t+\tnomod\tb2\ty\n")
    assert mr.parse_inside("b, outside") == ("b", "outside")
    with pytest.raises(ValueError):
        mr.parse_inside("a,a")


# ------------------------------------------------------------------------------------------------ 5. the interval join
def test_interval_join_equals_a_per_interval_brute_force():
    iv, k = rg.region_set(8)
    sets = rg.class_sets(iv, k)
    cands = rg.candidates()[:8]
    rec = rg.expected_records(cands, sets, k)                             # all states, inside any class
    dtype = [("candidate", "u4"), ("contig", "u4"), ("pos", "u4"), ("code", "u1"), ("classes", "u1")]
    rs = regions.RegionSet([f"c{c}" for c in range(k)], *rg.interval_arrays(iv), ["."] * len(iv), [f"i{j}" for j in range(len(iv))])
    sc = [SiteCandidate(b, m, mt, i) for b, mt, m, i in cands]
    got = mr.interval_rows(rs, np.array(rec, dtype=dtype), sc, rg.NAMES)
    want = []
    for j, (n, s, e, c) in enumerate(iv):                                 # interval by interval, candidate by candidate, site by site
        for cand in cands:
            hit = [x for x in rg.sites_of(cand) if x[0] == n and s <= x[1] < e]
            if hit:
                want.append([f"c{c}", f"i{j}", n, s, e, cand[0], cand[2], cand[1], cand[3]] + [sum(1 for x in hit if x[2] == st and x[3] == state) for st in (0, 1) for state in (0, 1, 2)])
    assert got == want and len(want) > 100
    assert mr.interval_rows(rs, np.zeros(0, dtype=dtype), sc, rg.NAMES) == []


# ------------------------------------------------------------------------------------------------ 6. the parser, the bindings
def test_parser_spec_of_motif_regions(capsys):
    sub = create_parser()._subparsers._group_actions[0].choices
    p = sub["motif_regions"]
    spec = {a.dest: (list(a.option_strings), a.default, a.required, type(a).__name__) for a in p._actions}
    assert [a.dest for a in p._actions if not a.option_strings] == ["assembly", "pileup"]
    assert [[g.required, [a.dest for a in g._group_actions]] for g in p._mutually_exclusive_groups] == [[True, ["contig_bin", "files", "directory"]]]
    assert spec["regions"] == (["--regions"], None, True, "_StoreAction") and spec["bin_motifs"][2] is True
    assert spec["classes"][1] is None and spec["upstream"][1] == 0 and spec["inside"][1] is None
    assert (spec["min_called"][1], spec["min_z"][1], spec["min_delta"][1]) == (20, 5.0, 0.2)
    assert spec["region_sites"][3] == spec["intervals"][3] == "_StoreTrueAction" and spec["states"][1] == ("mod", "nomod", "nocall")
    gc = {a.dest for a in sub["motif_gc"]._actions} - {"half", "gc_bins"}
    assert gc <= set(spec)                                                # everything the export commands share
    base = ["motif_regions", "a.fa", "p.bed", "-c", "cb.tsv", "--bin_motifs", "m.tsv"]
    args = create_parser().parse_args(base + ["--regions", "r.gff", "--classes", "gene,CDS", "--upstream", "50", "--inside", "gene,outside", "--states", "nomod"])
    assert (args.classes, args.upstream, args.inside, args.states, args.region_sites, args.intervals) == (("gene", "CDS"), 50, ("gene", "outside"), ("nomod",), False, False)
    for bad in (base, base + ["--regions", "r", "--upstream", "-3"], base + ["--regions", "r", "--classes", "a,a"], base + ["--regions", "r", "--states", "x"]):
        with pytest.raises(SystemExit):
            create_parser().parse_args(bad)
    capsys.readouterr()


def test_exports_are_declared_bound_and_built():
    from nanomotif_amd import _lib, build, engine
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    for name in ("nm_regions_create", "nm_regions_destroy", "nm_regions_covered", "nm_regions_plane", "nm_motif_regions_count", "nm_motif_regions_sites"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS
    assert "#define NM_REGION_MAX_CLASSES 8" in header and engine.REGION_MAX_CLASSES == regions.MAX_CLASSES == 8
    assert any(os.path.basename(s) == "nmregions.hip" for s in build.SRC_HIP)
    assert engine.REGION_DTYPE.names == engine.SITE_DTYPE.names + ("classes",) and engine.REGION_DTYPE["classes"] == np.uint8
    assert engine.region_class_set(["a", "b", "c"], None) == (7, False) and engine.region_class_set(["a", "b", "c"], ["c", "outside"]) == (4, True)
    assert engine.region_class_set(["a"], "outside") == (0, True)
    for bad in (["x"], []):
        with pytest.raises(ValueError):
            engine.region_class_set(["a", "b"], bad)
