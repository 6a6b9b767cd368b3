"""Host side of ``motif_pileup`` (no GPU): the brute force ``tests/test_gpu_motif_pileup.py`` compares nm_motif_pileup_count /
nm_motif_pileup_sites (csrc/nmpileup.hip) and the command against — built from ``site_positions`` and ``kept_mask`` of
tests/test_read_methylation_host.py and ``dense_records`` of tests/test_motif_fractions_host.py, nothing shared with the device —, the
conditions that make its input worth running (counted, not assumed), the text of nm_motif_pileup_text against a Python formatter, the
parser, the two files on a hand table, the loader's refusal and the build list.

The brute force is the definition.  Per candidate, per contig of its bin in bin order, the occurrences of the stripped motif on '+' and
of its reverse complement on '-' in ascending position, '+' before '-'; an occurrence whose modified base carries a kept record of the
candidate's code on its strand is a SITE and carries that record's (n_valid_cov, n_modified), any other is BARE and carries 0 / 0;
code = 4 on '-' | 1 for a bare occurrence.

The input is the geometry input of tests/test_read_methylation_host.py in the three bins of tests/test_motif_fractions_host.BINS_OF with
the candidates of tests/test_gpu_motif_fractions.candidates().  One case the issue asks for is absent from that list — a candidate with
no record at all between two that have some: every candidate of the list occurs in its bin.  ``candidates()`` below therefore inserts
ONE more candidate, ``EMPTY``, a 13-letter motif that does not occur on `big`; the input itself is unchanged."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import test_motif_fractions_host as F
import test_read_methylation_host as H
from nanomotif_amd import fasta
from nanomotif_amd.motif import iupac_to_regex

MINUS_BIT, BARE_BIT = 4, 1
SELECTS = (("site",), ("bare",), ("site", "bare"))
EMPTY = ("GATCGATCGATCA", "a", 1, "b0")
EMPTY_AT = 20
CHUNK, LANE, WORD, BLOCK = 8192, 128, 32, 512        # a wave's chunk, a lane's span, a word, a rank block (four lanes), in bp
RECORD = np.dtype([("candidate", np.uint32), ("contig", np.uint32), ("pos", np.uint32), ("code", np.uint8), ("n_valid", np.uint32), ("n_mod", np.uint32)])


# ------------------------------------------------------------------------------------------------ the brute force
def candidates():
    from test_gpu_motif_fractions import candidates as fraction_candidates
    out = fraction_candidates()
    out.insert(EMPTY_AT, EMPTY)
    return out


def contig_records(seq, dense, motif, pos, sites_cache, key):
    """(pos, code, n_valid, n_mod) of every occurrence of one candidate on one contig, in output order.  ``dense``: (cov, mod) of the
    contig under the candidate's code (``F.dense_records``), or None."""
    if key not in sites_cache:
        sites_cache[key] = H.site_positions(seq, iupac_to_regex(motif), pos)
    fwd, rev = sites_cache[key]
    at = np.concatenate([fwd, rev]).astype(np.int64)
    strand = np.concatenate([np.zeros(len(fwd), np.int64), np.ones(len(rev), np.int64)])
    order = np.lexsort((strand, at))
    at, strand = at[order], strand[order]
    if dense is None:
        cov, mod = np.full(len(at), -1, np.int64), np.zeros(len(at), np.int64)
    else:
        cov, mod = dense[0][strand, at], dense[1][strand, at]
    site = cov >= 0
    return at, strand * MINUS_BIT + np.where(site, 0, BARE_BIT), np.where(site, cov, 0), np.where(site, mod, 0)


def brute_records(names, seqs, records, bins_of, cands, min_cov=H.MIN_COV, min_frac=H.MIN_FRAC):
    """RECORD[]: every occurrence of every candidate (IUPAC motif, code, mod position, bin) in output order; ``contig`` indexes ``names``."""
    dense = F.dense_records(seqs, records, min_cov, min_frac)
    cache, parts = {}, []
    for k, (motif, code, pos, b) in enumerate(cands):
        for name in bins_of[b]:
            at, c, nv, nm = contig_records(seqs[name], dense.get((name, code)), motif, pos, cache, (motif, pos, name))
            rec = np.zeros(len(at), dtype=RECORD)
            rec["candidate"], rec["contig"], rec["pos"], rec["code"], rec["n_valid"], rec["n_mod"] = k, names.index(name), at, c, nv, nm
            parts.append(rec)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=RECORD)


def selected(rec, select):
    """The records of ``brute_records`` under ``select`` (a selection of "site", "bare")."""
    bare = (rec["code"] & BARE_BIT) != 0
    return rec[(bare & ("bare" in select)) | (~bare & ("site" in select))]


def count_table(rec, names, bins_of, cands):
    """[int64[n_contigs, 4]] per candidate: fwd site, fwd bare, rev site, rev bare."""
    out = []
    for k, c in enumerate(cands):
        mine = rec[rec["candidate"] == k]
        t = np.zeros((len(bins_of[c[3]]), 4), dtype=np.int64)
        for i, name in enumerate(bins_of[c[3]]):
            code = mine["code"][mine["contig"] == names.index(name)]
            t[i] = [int((code == x).sum()) for x in (0, BARE_BIT, MINUS_BIT, MINUS_BIT | BARE_BIT)]
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def geometry():
    """(names, seqs, records, candidates, RECORD[] of every occurrence) on the geometry input: computed once, shared with the GPU suite."""
    names, seqs, records = H.meth_input()
    cands = candidates()
    rec = brute_records(names, seqs, records, F.BINS_OF, cands)
    rec.setflags(write=False)
    return names, seqs, records, cands, rec


# ------------------------------------------------------------------------------------------------ the Python formatter
def bed_text(rec, cands, names) -> str:
    from nanomotif_amd.motif_pileup import percent_text
    lines = []
    for r in rec.tolist():
        k, contig, pos, code, nv, nm = r
        m, mt, mp, b = cands[k]
        pct = "" if code & BARE_BIT else percent_text(nm, nv)
        lines.append("\t".join([fasta.original_name(names[contig]), str(pos), str(pos + 1), f"{m}_{mt}_{mp}", str(nv), "-" if code & MINUS_BIT else "+", str(nm), pct, b]))
    return "".join(line + "\n" for line in lines)


def native_text(rec, cands, names) -> bytes:
    from nanomotif_amd.motif_pileup import format_pileup
    seg_begin = np.searchsorted(rec["candidate"], np.arange(len(cands) + 1))
    return format_pileup(rec["contig"], rec["pos"], rec["code"], rec["n_valid"], rec["n_mod"], seg_begin, [f"{m}_{mt}_{mp}" for m, mt, mp, _ in cands],
                         [c[3] for c in cands], [fasta.original_name(n) for n in names])


# ------------------------------------------------------------------------------------------------ the tests
def test_the_brute_force_on_a_hand_case():
    """GATC x 3 ('+' A at 1, 5, 9; '-' A at 2, 6, 10) with the records of the hand case of test_read_methylation_host: kept (1 +) 10/4,
    (2 -) 5/5, (5 +) 8/2; dropped (6 -) and (9 +).  The second contig has one occurrence per strand and no record."""
    col = lambda *x: np.array(x, dtype=np.int64)
    rec = {("c", "a"): dict(position=col(1, 2, 3, 5, 6, 9), strand=np.frombuffer(b"+-++-+", np.uint8), n_valid=col(10, 5, 9, 8, 2, 8),
                            n_mod=col(4, 5, 9, 2, 1, 8), n_diff=col(0, 0, 0, 2, 0, 3))}
    seqs = {"c": "GATC" * 3, "d": "TTGATC"}
    cands = [("GATC", "a", 1, "b")]
    got = brute_records(["c", "d"], seqs, rec, {"b": ["c", "d"]}, cands)
    assert got.tolist() == [(0, 0, 1, 0, 10, 4), (0, 0, 2, 4, 5, 5), (0, 0, 5, 0, 8, 2), (0, 0, 6, 5, 0, 0), (0, 0, 9, 1, 0, 0), (0, 0, 10, 5, 0, 0),
                            (0, 1, 3, 1, 0, 0), (0, 1, 4, 5, 0, 0)]
    assert selected(got, ("site",))["pos"].tolist() == [1, 2, 5] and selected(got, ("bare",))["pos"].tolist() == [6, 9, 10, 3, 4]
    assert len(selected(got, ("site", "bare"))) == 8
    (t,) = count_table(got, ["c", "d"], {"b": ["c", "d"]}, cands)
    assert t.tolist() == [[2, 1, 1, 2], [0, 1, 0, 1]]
    # the same numbers the fractions brute force holds: occurrences 3 / 3, sums 18 / 6 on '+' and 5 / 5 on '-'
    (f,) = F.expected_table(seqs, rec, {"b": ["c", "d"]}, cands, 4)
    assert f[0, :, 4:].tolist() == [[3, 18, 6], [3, 5, 5]]


def test_the_input_holds_every_case_the_kernel_can_get_wrong():
    """By count, on the expected output: what the fill pass of pileup_kernel can only get right by computing it."""
    names, seqs, records, cands, rec = geometry()
    dense = F.dense_records(seqs, records)
    site = rec[(rec["code"] & BARE_BIT) == 0]
    n = dict(both_strands_in_a_word=0, popcount_inside_the_word=0, bits_in_an_earlier_word=0, lane=[0, 0, 0, 0], first_word=0, last_word=0, at_8191=0, at_8192=0)
    seen_lane = set()
    word_strands = {}
    for k, contig, pos, code, _, _ in site.tolist():
        s = 1 if code & MINUS_BIT else 0
        word_strands.setdefault((k, contig, pos // WORD), set()).add(s)
        present = dense[(names[contig], cands[k][1])][0][s] >= 0
        lane0, word0, block0 = pos // LANE * LANE, pos // WORD * WORD, pos // BLOCK * BLOCK
        if (k, contig, s, lane0) not in seen_lane:                          # the lane's first site on this strand
            seen_lane.add((k, contig, s, lane0))
            n["popcount_inside_the_word"] += bool(present[word0:pos].any())
        n["bits_in_an_earlier_word"] += bool(present[lane0:word0].any())
        q = (pos - block0) // LANE
        n["lane"][q] += bool(q == 0 or present[block0:lane0].any())         # records in the lanes before it: the shuffles carry something
        n["first_word"] += pos % CHUNK < WORD
        n["last_word"] += pos % CHUNK >= CHUNK - WORD
        n["at_8191"] += pos == CHUNK - 1
        n["at_8192"] += pos == CHUNK
    n["both_strands_in_a_word"] = sum(len(v) == 2 for v in word_strands.values())
    tables = count_table(rec, names, F.BINS_OF, cands)
    bare_only = [(cands[k][:3], name) for k, t in enumerate(tables) for name, row in zip(F.BINS_OF[cands[k][3]], t) if row[[1, 3]].sum() and not row[[0, 2]].sum()]
    per_cand = [int(t.sum()) for t in tables]
    print(n, "contigs with bare records only:", len(bare_only), "records per candidate:", per_cand)
    assert n["both_strands_in_a_word"] > 100 and n["popcount_inside_the_word"] > 100 and n["bits_in_an_earlier_word"] > 100
    assert min(n["lane"][1:]) > 100 and n["first_word"] > 10 and n["last_word"] > 10 and n["at_8191"] >= 1 and n["at_8192"] >= 1
    assert {name for _, name in bare_only} >= {"norec", "tiny3"} and len(bare_only) >= 5
    assert per_cand[EMPTY_AT] == 0 and cands[EMPTY_AT] == EMPTY and all(x > 0 for i, x in enumerate(per_cand) if i != EMPTY_AT)
    # what the issue names of the input itself, seen in the records: GATC on the last bit of a rank block and either side of the carry
    gatc = cands.index(("GATC", "a", 1, "b2"))
    mine = site[(site["candidate"] == gatc) & (site["contig"] == names.index("long"))]
    got = {(int(p), int(c)): (int(v), int(m)) for p, c, v, m in zip(mine["pos"], mine["code"], mine["n_valid"], mine["n_mod"])}
    for (_, pos, strand), want in H.PLANTED.items():
        if ("long", pos, strand) in H.PLANTED_SITES:
            assert got[(pos, MINUS_BIT if strand == H.MINUS else 0)] == want
    # all three selections differ, the duplicated candidate yields its records twice, both codes and the three reach classes are there
    assert 0 < len(selected(rec, ("site",))) < len(rec) and len(selected(rec, ("site",))) + len(selected(rec, ("bare",))) == len(rec)
    twice = [k for k, c in enumerate(cands) if c == cands[2]]
    assert len(twice) == 2 and np.array_equal(rec[rec["candidate"] == twice[0]][["contig", "pos", "code", "n_valid", "n_mod"]],
                                              rec[rec["candidate"] == twice[1]][["contig", "pos", "code", "n_valid", "n_mod"]])
    # the order is the contract: candidate, contig in bin order, position, '+' before '-'
    order = np.lexsort((rec["code"] >> 2, rec["pos"], rec["contig"], rec["candidate"]))
    assert np.array_equal(order, np.arange(len(rec)))                     # (the engine's contig ids ascend in bin order on this input)
    assert 100_000 < len(rec) < 400_000


def test_the_brute_force_sums_are_the_fraction_tables():
    """Per (candidate, contig, strand): sites, occurrences and the two sums equal the fractions brute force's."""
    names, seqs, records, cands, rec = geometry()
    tables = F.expected_table(seqs, records, F.BINS_OF, cands, 20)
    counts = count_table(rec, names, F.BINS_OF, cands)
    for k, (c, f, t) in enumerate(zip(cands, tables, counts)):
        mine = rec[rec["candidate"] == k]
        for i, name in enumerate(F.BINS_OF[c[3]]):
            here = mine[mine["contig"] == names.index(name)]
            for s in (0, 1):
                on = here[(here["code"] >> 2) == s]
                assert [int(t[i, 2 * s]), int(t[i, 2 * s] + t[i, 2 * s + 1]), int(on["n_valid"].sum()), int(on["n_mod"].sum())] == \
                       [int(f[i, s, :20].sum())] + [int(x) for x in f[i, s, 20:]], (c, name, s)


HAND_CANDS = [("GATC", "a", 1, "binA"), ("CCWGG", "m", 1, "binA"), ("A", "a", 0, "binB")]
HAND_NAMES = ["c1", "c2" + fasta.ALIAS_SEP + "binB", "a_rather_long_contig_name"]
HAND_RECORDS = [  # candidate, contig, pos, code, n_valid, n_mod
    (0, 0, 0, 0, 7, 0), (0, 0, 9, 4, 3, 1), (0, 0, 10, 0, 3, 2), (0, 0, 99, 5, 0, 0), (0, 0, 100, 4, 12, 12), (0, 2, 4_294_967_294, 1, 0, 0),
    (2, 1, 5, 0, 6, 1), (2, 1, 5, 4, 4_000_000_000, 3_999_999_999), (2, 1, 999_999, 0, 200, 1), (2, 1, 1_000_000, 4, 8, 7), (2, 2, 0, 5, 0, 0)]
HAND_BED = "\n".join([
    "c1\t0\t1\tGATC_a_1\t7\t+\t0\t0.00\tbinA",
    "c1\t9\t10\tGATC_a_1\t3\t-\t1\t33.33\tbinA",
    "c1\t10\t11\tGATC_a_1\t3\t+\t2\t66.67\tbinA",
    "c1\t99\t100\tGATC_a_1\t0\t-\t0\t\tbinA",
    "c1\t100\t101\tGATC_a_1\t12\t-\t12\t100.00\tbinA",
    "a_rather_long_contig_name\t4294967294\t4294967295\tGATC_a_1\t0\t+\t0\t\tbinA",
    "c2\t5\t6\tA_a_0\t6\t+\t1\t16.67\tbinB",
    "c2\t5\t6\tA_a_0\t4000000000\t-\t3999999999\t100.00\tbinB",
    "c2\t999999\t1000000\tA_a_0\t200\t+\t1\t0.50\tbinB",
    "c2\t1000000\t1000001\tA_a_0\t8\t-\t7\t87.50\tbinB",
    "a_rather_long_contig_name\t0\t1\tA_a_0\t0\t-\t0\t\tbinB"]) + "\n"


def test_the_percentage_is_computed_in_integers():
    from nanomotif_amd.motif_pileup import percent_text
    assert [percent_text(m, v) for m, v in ((0, 7), (1, 3), (2, 3), (12, 12), (1, 6), (1, 200), (7, 8), (1, 8), (1, 16), (3, 16))] == \
           ["0.00", "33.33", "66.67", "100.00", "16.67", "0.50", "87.50", "12.50", "6.25", "18.75"]
    assert percent_text(1, 32) == "3.13" and percent_text(3, 32) == "9.38"                   # 3.125 and 9.375: half up, not half to even
    assert percent_text(3_999_999_999, 4_000_000_000) == "100.00" and percent_text(1, 4_000_000_000) == "0.00"


@pytest.mark.parametrize("threads", ["1", "4"])
def test_the_native_text_is_the_python_formatters(threads, monkeypatch):
    """nm_motif_pileup_text on the hand records (the percentages 0, 1/3, 2/3 and 1 among them; a middle candidate without a record) and on
    the first 3 000 and the last 3 000 records of the geometry input: more than a thread's minimum share each, whatever NM_POST_THREADS."""
    monkeypatch.setenv("NM_POST_THREADS", threads)
    hand = np.array(HAND_RECORDS, dtype=RECORD)
    assert bed_text(hand, HAND_CANDS, HAND_NAMES) == HAND_BED
    assert native_text(hand, HAND_CANDS, HAND_NAMES) == HAND_BED.encode()
    assert native_text(hand[:0], HAND_CANDS, HAND_NAMES) == b""
    names, _, _, cands, rec = geometry()
    for part in (rec[:3_000], rec[-3_000:], selected(rec, ("site",))[5_000:9_000]):
        assert native_text(part, cands, names) == bed_text(part, cands, names).encode()


def test_the_native_text_refuses_what_it_cannot_write():
    from nanomotif_amd import _lib
    from nanomotif_amd._lib import NmScanError
    hand = np.array(HAND_RECORDS, dtype=RECORD)
    for field, value, match in (("contig", 3, "contig >= 3"), ("code", 2, "code"), ("code", 8, "code"), ("n_valid", 0, "n_valid_cov"), ("n_mod", 8, "n_valid_cov")):
        bad = hand.copy()
        bad[field][0] = value
        with pytest.raises(NmScanError, match=match) as e:
            native_text(bad, HAND_CANDS, HAND_NAMES)
        assert e.value.code == -1
    lib = _lib.load()
    size = C.c_uint64(7)
    assert lib.nm_motif_pileup_text(0, None, None, None, None, None, 0, None, None, None, 0, None, None, None, 0, C.byref(size)) == 0 and size.value == 0
    assert lib.nm_motif_pileup_text(1, None, None, None, None, None, 0, None, None, None, 0, None, None, None, 0, C.byref(size)) == -1
    assert lib.nm_motif_pileup_text(0, None, None, None, None, None, 0, None, None, None, 0, None, None, None, 0, None) == -1
    assert native_text(hand, HAND_CANDS, HAND_NAMES) == HAND_BED.encode()


HAND_SUMMARY = "\n".join(["\t".join(x) for x in [
    ["bin", "contig", "motif", "mod_type", "mod_position", "n_occurrences_fwd", "n_occurrences_rev", "n_sites_fwd", "n_sites_rev", "sum_valid_cov",
     "sum_modified", "mean_read_cov", "weighted_mean"],
    ["binA", "c1", "GATC", "a", "1", "2", "3", "2", "2", "25", "15", "6.250000", "0.600000"],
    ["binA", "a_rather_long_contig_name", "GATC", "a", "1", "1", "0", "0", "0", "0", "0", "", ""],
    ["binB", "c2", "A", "a", "0", "2", "2", "2", "2", "4000000214", "4000000008", "1000000053.500000", "1.000000"],
    ["binB", "a_rather_long_contig_name", "A", "a", "0", "0", "1", "0", "0", "0", "0", "", ""]]]) + "\n"


class FakeEngine:
    """What ``export_pileup`` asks of an engine: the contig names and ``motif_pileup`` — here the hand records in windows of four."""

    def __init__(self):
        self.contig_names = HAND_NAMES
        self.asked = None

    def motif_pileup(self, candidates, select, max_records):
        from nanomotif_amd.engine import SiteBatch
        self.asked = (len(candidates), select, max_records)
        rec = selected(np.array(HAND_RECORDS, dtype=RECORD), select)
        bins_of = {"binA": [HAND_NAMES[0], HAND_NAMES[2]], "binB": [HAND_NAMES[1], HAND_NAMES[2]]}
        counts = [(bins_of[c[3]], t) for c, t in zip(HAND_CANDS, count_table(np.array(HAND_RECORDS, dtype=RECORD), HAND_NAMES, bins_of, HAND_CANDS))]
        for first in range(0, len(rec), 4):
            yield SiteBatch(0, 3, first, len(rec), rec[first:first + 4], counts if first == 0 else None)


def test_both_files_on_a_hand_table(tmp_path):
    from nanomotif_amd import motif_pileup as mp
    from nanomotif_amd.motif_sites import SiteCandidate
    cands = [SiteCandidate(b, m, mt, pos) for m, mt, pos, b in HAND_CANDS]
    for all_occurrences in (True, False):
        eng = FakeEngine()
        with open(tmp_path / "p.bed", "wb") as f:
            summary, _ = mp.export_pileup(eng, cands, all_occurrences, f)
        assert eng.asked == (3, ("site", "bare") if all_occurrences else ("site",), None)
        lines = HAND_BED.splitlines(keepends=True)
        assert open(tmp_path / "p.bed").read() == "".join(x for x in lines if all_occurrences or "\t\t" not in x)
        assert mp.format_summary(summary) == HAND_SUMMARY                 # the summary does not depend on --all_occurrences
    assert mp.SUMMARY_HEADER == HAND_SUMMARY.splitlines()[0].split("\t") and (mp.BED_NAME, mp.SUMMARY_NAME) == ("motif-pileup.bed", "motif-pileup-summary.tsv")


def test_the_parser_has_the_defaults_and_refuses_unknown_options(capsys):
    from nanomotif_amd.argparser import create_parser
    base = ["motif_pileup", "a.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "m.tsv"]
    args = create_parser().parse_args(base)
    assert (args.command, args.assembly, args.pileup, args.contig_bin, args.bin_motifs, args.out, args.all_occurrences, args.min_valid_read_coverage,
            args.min_valid_cov_to_diff_fraction, args.device) == ("motif_pileup", "a.fasta", "p.bed", "cb.tsv", ["m.tsv"], "nanomotif", False, 5, 0.8, None)
    args = create_parser().parse_args(base + ["n.tsv", "--all_occurrences", "--min_valid_read_coverage", "3", "--min_valid_cov_to_diff_fraction", "0.5", "--device", "1"])
    assert (args.bin_motifs, args.all_occurrences, args.min_valid_read_coverage, args.min_valid_cov_to_diff_fraction, args.device) == (["m.tsv", "n.tsv"], True, 3, 0.5, 1)
    for bad in (["--bins", "20"], ["--min_sites", "5"], ["--methylation_threshold_low", "0.2"], ["--states", "mod"]):      # no histogram options
        with pytest.raises(SystemExit) as e:
            create_parser().parse_args(base + bad)
        assert e.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        create_parser().parse_args(base[:5])                              # --bin_motifs is required
    assert "motif_pileup" in create_parser().format_help()


def test_the_command_refuses_a_contig_listed_under_two_bins_before_an_engine_exists(tmp_path, monkeypatch, caplog):
    from nanomotif_amd import loading, motif_pileup as mp
    from nanomotif_amd.argparser import create_parser

    def no_engine(*a, **kw):                                          # pragma: no cover - the refusal comes first
        raise AssertionError("an engine was created")
    monkeypatch.setattr(loading, "ScanEngine", no_engine)
    monkeypatch.setenv("WORLD_SIZE", "1")
    (tmp_path / "cb.tsv").write_text("c1\tbin_a\nc2\tbin_a\nc2\tbin_b\n")
    (tmp_path / "m.tsv").write_text("reference\tmotif\tmod_position\tmod_type\nbin_a\tGATC\t1\ta\n")
    args = create_parser().parse_args(["motif_pileup", str(tmp_path / "a.fasta"), str(tmp_path / "p.bed"), "-c", str(tmp_path / "cb.tsv"),
                                       "--bin_motifs", str(tmp_path / "m.tsv"), "--out", str(tmp_path / "out")])
    with caplog.at_level("ERROR"):
        assert mp.run(args) == 2
    assert "motif_pileup" in caplog.text and "listed under several bins (e.g. c2)" in caplog.text
    assert not os.path.exists(tmp_path / "out" / mp.BED_NAME)
    monkeypatch.setenv("WORLD_SIZE", "2")                              # the multi-rank refusal comes before anything is read
    assert mp.run(args) == 2


def test_the_unit_is_built_and_bound():
    from nanomotif_amd import _lib, build
    from nanomotif_amd.engine import PILEUP_DTYPE, PILEUP_RECORD_BYTES, pileup_select
    assert os.path.join("csrc", "nmpileup.hip") in [os.path.relpath(s, os.path.dirname(build.__file__)) for s in build.SRC_HIP]
    assert {"nm_motif_pileup_count", "nm_motif_pileup_sites", "nm_motif_pileup_text"} <= set(_lib.SYMBOLS)
    assert PILEUP_DTYPE == RECORD and PILEUP_RECORD_BYTES == 17 == sum(PILEUP_DTYPE[f].itemsize for f in PILEUP_DTYPE.names if f != "candidate")
    assert [pileup_select(s) for s in SELECTS] == [1, 2, 3]
    for bad in ((), ("mod",)):
        with pytest.raises(ValueError):
            pileup_select(bad)
    lib = _lib.load()                                                 # refusals that need no device: NULLs, the selection, the context
    u64 = (C.c_uint64 * 2)()
    for select, text in ((0, b"select 0"), (4, b"select 4"), (7, b"select 7")):
        assert lib.nm_motif_pileup_count(None, 0, None, None, None, None, None, None, select, u64, None, None) == -1 and text in lib.nm_last_error()
    assert lib.nm_motif_pileup_count(None, 0, None, None, None, None, None, None, 3, None, None, None) == -1 and b"NULL" in lib.nm_last_error()
    assert lib.nm_motif_pileup_count(None, 0, None, None, None, None, None, None, 3, u64, None, None) == -1 and b"ctx" in lib.nm_last_error()
    assert lib.nm_motif_pileup_sites(None, 0, None, None, None, None, None, None, 1, 0, 0, None, None, None, None, None, u64, u64) == -1 and b"ctx" in lib.nm_last_error()
    assert lib.nm_motif_pileup_sites(None, 0, None, None, None, None, None, None, 1, 0, 0, None, None, None, None, None, None, u64) == -1 and b"NULL" in lib.nm_last_error()

