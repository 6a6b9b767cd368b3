"""Host side of ``motif_fractions`` (no GPU): the brute force ``tests/test_gpu_motif_fractions.py`` compares nm_motif_fractions_count
(csrc/nmfractions.hip) and the command against — built from ``site_positions`` and ``kept_mask`` of tests/test_read_methylation_host.py and
dense per-position tables — the conditions that make its input worth running, the bin, quantile, edge and flag rules on hand cases, the text
of the three files, the refusals of the parser and of the loader.

The brute force is the definition.  Per (candidate, contig of its bin) and strand: ``occurrences`` = the positions of the modified base of
the stripped motif on '+' (strand 0) / of its reverse complement on '-' (strand 1); a site = an occurrence with a kept record of the
candidate's code on that strand; its bin = min(B - 1, n_mod * B // n_valid); ``sum_valid`` / ``sum_mod`` run over the sites."""
import argparse
import functools

import numpy as np
import pytest

from nanomotif_amd import fasta, motif_fractions as mf
from nanomotif_amd.motif import iupac_to_regex
from nanomotif_amd.motif_sites import SiteCandidate
from test_read_methylation_host import MIN_COV, MIN_FRAC, MINUS, PLANTED, PLANTED_SITES, PLUS, expected, kept_mask, meth_input, request, site_positions

EXTRA = 3
# no bin starts at chunk 0 alone; `norec` (sites, no records) shares a bin with contigs that have records
BINS_OF = {"b0": ["big"], "b1": ["tiny1", "tiny2", "tiny3", "small", "edge", "mid"], "b2": ["long", "norec", "endGA", "startTC"]}


# ------------------------------------------------------------------------------------------------ the brute force
def dense_records(seqs, records, min_cov=MIN_COV, min_frac=MIN_FRAC):
    """{(contig, code): (cov int64[2, L] with -1 where no kept record sits, mod int64[2, L])}."""
    dense = {}
    for (name, code), r in records.items():
        keep = kept_mask(r, min_cov, min_frac)
        cov = np.full((2, len(seqs[name])), -1, dtype=np.int64)
        mod = np.zeros((2, len(seqs[name])), dtype=np.int64)
        s = (r["strand"][keep] == MINUS).astype(np.int64)
        cov[s, r["position"][keep]] = r["n_valid"][keep]
        mod[s, r["position"][keep]] = r["n_mod"][keep]
        dense[(name, code)] = (cov, mod)
    return dense


def site_values(seqs, records, bins_of, cands, min_cov=MIN_COV, min_frac=MIN_FRAC):
    """Per candidate (IUPAC motif, code, mod position, bin) and contig of its bin, per strand: (occurrences, cov of the sites, mod of the
    sites).  What every number of bins is computed from."""
    dense = dense_records(seqs, records, min_cov, min_frac)
    sites = {}
    out = []
    for motif, code, pos, b in cands:
        rows = []
        for name in bins_of[b]:
            key = (motif, pos, name)
            if key not in sites:
                sites[key] = site_positions(seqs[name], iupac_to_regex(motif), pos)
            row = []
            for s, at in enumerate(sites[key]):
                if (name, code) in dense:
                    cov, mod = dense[(name, code)]
                    have = cov[s, at] >= 0
                    row.append((len(at), cov[s, at[have]], mod[s, at[have]]))
                else:
                    row.append((len(at), np.zeros(0, np.int64), np.zeros(0, np.int64)))
            rows.append(row)
        out.append(rows)
    return out


def table_of(values, B):
    """[uint64[n_contigs, 2, B + 3]] of ``site_values`` at B bins."""
    out = []
    for rows in values:
        t = np.zeros((len(rows), 2, B + EXTRA), dtype=np.uint64)
        for i, row in enumerate(rows):
            for s, (occ, cov, mod) in enumerate(row):
                for c, m in zip(cov.tolist(), mod.tolist()):
                    t[i, s, min(B - 1, m * B // c)] += 1
                t[i, s, B:] = (occ, int(cov.sum()), int(mod.sum()))
        out.append(t)
    return out


def expected_table(seqs, records, bins_of, cands, B, min_cov=MIN_COV, min_frac=MIN_FRAC):
    return table_of(site_values(seqs, records, bins_of, cands, min_cov, min_frac), B)


ONE_LETTER = [("A", "a", 0), ("C", "m", 0)]


@functools.lru_cache(maxsize=None)
def whole_values():
    """``site_values`` of A_a_0, C_m_0 and GATC_a_1 on every contig of the geometry input, in its own order (one bin)."""
    names, seqs, records = meth_input()
    return site_values(seqs, records, {"all": names}, [m + ("all",) for m in ONE_LETTER + [("GATC", "a", 1)]])


# ------------------------------------------------------------------------------------------------ the tests
def test_the_bin_rule_and_the_brute_force_on_a_hand_case():
    assert mf.site_bin(10, 20, 20) == 10 and mf.site_bin(1, 3, 3) == 1 and mf.site_bin(29, 30, 64) == 61
    for B in (2, 3, 20, 64):
        assert mf.site_bin(7, 7, B) == B - 1 and mf.site_bin(0, 7, B) == 0
    assert [mf.site_bin(m, 4, 4) for m in range(5)] == [0, 1, 2, 3, 3]                       # bin k is [k / B, (k + 1) / B); 1 is in the last
    # GATC x 3 ('+' A at 1, 5, 9; '-' A at 2, 6, 10) with the records of the hand case of test_read_methylation_host: kept (1 +) 10/4,
    # (2 -) 5/5, (5 +) 8/2; dropped (6 -) and (9 +); (3 +) sits on a C
    col = lambda *x: np.array(x, dtype=np.int64)
    rec = {("c", "a"): dict(position=col(1, 2, 3, 5, 6, 9), strand=np.frombuffer(b"+-++-+", np.uint8), n_valid=col(10, 5, 9, 8, 2, 8),
                            n_mod=col(4, 5, 9, 2, 1, 8), n_diff=col(0, 0, 0, 2, 0, 3))}
    seqs = {"c": "GATC" * 3, "d": "TTGATC"}
    (t,) = expected_table(seqs, rec, {"b": ["c", "d"]}, [("GATC", "a", 1, "b")], 4)
    assert t.shape == (2, 2, 7) and t.dtype == np.uint64
    assert t[0].tolist() == [[0, 2, 0, 0, 3, 18, 6], [0, 0, 0, 1, 3, 5, 5]]                   # 4/10 -> 1, 2/8 -> 1; 5/5 -> 3
    assert t[1].tolist() == [[0, 0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0, 0]]                   # a contig without any record: occurrences only
    (c,) = expected_table(seqs, rec, {"b": ["c", "d"]}, [("C", "a", 0, "b")], 2)
    assert c[0].tolist() == [[0, 1, 3, 9, 9], [0, 0, 3, 0, 0]]                               # '+' C at 3, 7, 11; '-' C = '+' G at 0, 4, 8
    (hi,) = expected_table(seqs, rec, {"b": ["c"]}, [("GATC", "a", 1, "b")], 4, min_cov=9)
    assert hi[0].tolist() == [[0, 1, 0, 0, 3, 10, 4], [0, 0, 0, 0, 3, 0, 0]]


def test_the_input_is_not_degenerate():
    names, seqs, records = meth_input()
    values = whole_values()
    t20, t64 = table_of(values, 20), table_of(values, 64)
    for k, name in enumerate(("A_a_0", "C_m_0", "GATC_a_1")):
        per_strand = t20[k].sum(axis=0)
        print(name, "B = 20, '+':", per_strand[0, :20].tolist(), "'-':", per_strand[1, :20].tolist())
        assert (per_strand[:, :20] > 0).all(), name
        assert (per_strand[0] != per_strand[1]).any(), name                                 # both strands differ
    a64 = t64[0].sum(axis=0)
    assert ((a64[:, :64] > 0).sum(axis=1) >= 60).all()
    # rows with occurrences and no site: tiny3 (dropped records only) and norec (no records at all)
    for k, letter in ((0, "A"),):
        for name in ("tiny3", "norec"):
            row = t20[k][names.index(name)]
            assert row[:, :20].sum() == 0 and row[:, 21:].sum() == 0 and row[0, 20] == seqs[name].count(letter) > 0 and row[1, 20] == seqs[name].count("T") > 0
    # every planted GATC site sits in the bin the rule gives, and the whole row equals the histogram of the pinned segment's values
    gatc, long_ = table_of(values, 20)[2], names.index("long")
    fwd, rev = site_positions(seqs["long"], "GATC", 1)
    for B in (2, 3, 20, 64):
        row = table_of(values, B)[2][long_]
        alone = expected_table({"long": seqs["long"]}, {("long", "a"): _only(records[("long", "a")], PLANTED_SITES)}, {"b": ["long"]},
                               [("GATC", "a", 1, "b")], B)[0][0]
        want = np.zeros((2, B), dtype=np.int64)
        for _, pos, strand in PLANTED_SITES:
            cov, mod = PLANTED[("long", pos, strand)]
            assert pos in (fwd if strand == PLUS else rev)
            want[int(strand == MINUS), mf.site_bin(mod, cov, B)] += 1
        assert alone[:, :B].tolist() == want.tolist() and (row[:, :B].astype(np.int64) >= want).all()
        seg = expected()[(request().index(("GATC", "a", 1)), "long")]
        both = np.bincount([mf.site_bin(m, c, B) for c, m in zip(seg.cov, seg.mod)], minlength=B)
        assert row[:, :B].sum(axis=0).tolist() == both.tolist() and int(row[:, B + 1].sum()) == seg.cov_sum and int(row[:, B + 2].sum()) == seg.mod_sum
    assert gatc[long_, :, 20].tolist() == [len(fwd), len(rev)]
    # the sums agree with the segments the read-methylation brute force pins
    a = request().index(("A", "a", 0))
    for i, name in enumerate(names):
        seg = expected().get((a, name))
        assert int(t20[0][i, :, :20].sum()) == (seg.n if seg else 0)


def _only(r, sites):
    """The records of one contig restricted to the (position, strand) of ``sites``."""
    keep = np.zeros(len(r["position"]), dtype=bool)
    for _, pos, strand in sites:
        keep |= (r["position"] == pos) & (r["strand"] == strand)
    assert int(keep.sum()) == len(sites)
    return {k: v[keep] for k, v in r.items()}


def test_quantiles_edges_and_flags_on_hand_histograms():
    h = [5, 0, 0, 5]                                                                        # n = 10: needs 1, 3, 5, 8, 9
    assert [mf.quantile_edge(h, q) for q in mf.QUANTILES] == [0.0, 0.0, 0.0, 0.75, 0.75]
    assert [mf.quantile_edge([0, 1, 0, 0], q) for q in (10, 90)] == [0.25, 0.25]            # max(1, .) with n = 1
    assert mf.quantile_edge([1, 1, 1, 1, 1, 1, 1, 1, 1, 1], 50) == 0.4 and mf.quantile_edge([0] * 4, 50) is None
    assert mf.quantile_edge([1] * 3, 50) == 1 / 3                                           # (50 * 3 + 99) // 100 = 2: the second bin
    # the thresholds snap to bin edges: k = floor(x B + 0.5)
    assert mf.snap_edges(0.3, 0.7, 20) == (6, 14) and mf.snap_edges(0.3, 0.7, 3) == (1, 2) and mf.snap_edges(0.3, 0.7, 64) == (19, 45)
    assert mf.snap_edges(0.3, 0.3, 2) == (1, 1)                                             # floor(0.6 + 0.5) = 1: 0 < 1 <= 1 < 2 holds
    for low, high, B, named in ((0.2, 0.2, 2, "0 / 0"), (0.3, 0.8, 2, "1 / 2"), (0.7, 0.3, 20, "14 / 6"), (0.0, 0.7, 20, "0 / 14"), (0.3, 1.0, 20, "6 / 20")):
        with pytest.raises(ValueError, match=f"bin edges {named} of {B}"):
            mf.snap_edges(low, high, B)
    # one histogram per branch of the flag rule, B = 10, edges 3 / 7, 20 sites, t = 0.1
    flag = lambda h, min_sites=20, t=0.1: mf.flag_of(h, 3, 7, min_sites, t)
    assert mf.zone_counts([1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 3, 7) == (6, 22, 27)
    assert flag([9, 0, 0, 0, 0, 0, 0, 0, 0, 10]) == "few_sites"                             # 19 < 20
    assert flag([1, 0, 0, 1, 0, 0, 0, 6, 6, 6]) == "methylated"                             # 18 >= 0.9 * 20
    assert flag([6, 6, 6, 0, 0, 0, 2, 0, 0, 0]) == "unmethylated"
    assert flag([6, 0, 0, 1, 0, 0, 0, 0, 0, 13]) == "bimodal"                               # both modes >= 2, the middle below the smaller
    assert flag([2, 0, 0, 0, 2, 0, 0, 0, 0, 16]) == "partial"                               # the middle is not below the smaller mode
    assert flag([1, 0, 0, 2, 0, 0, 0, 0, 0, 17]) == "partial"                               # 17 < 18 and the low mode below t n
    assert flag([0, 0, 0, 5, 5, 5, 5, 0, 0, 0]) == "partial"
    assert flag([10, 0, 0, 0, 0, 0, 0, 0, 0, 9], min_sites=19) == "bimodal" and flag([0] * 10, min_sites=0) == "methylated"
    assert flag([5, 0, 0, 0, 0, 0, 0, 0, 0, 15], t=0.2) == "bimodal" and flag([5, 0, 0, 0, 0, 0, 0, 0, 0, 15], t=0.25) == "methylated"   # 15 >= 0.75 * 20


_T = "\t".join
HAND_SUMMARY = "\n".join([
    _T(["bin", "motif", "mod_type", "mod_position", "n_occurrences", "n_sites", "mean_read_cov", "weighted_mean", "q10", "q25", "q50", "q75", "q90",
        "share_low", "share_mid", "share_high", "low_edge", "high_edge", "flag", "n_sites_fwd", "n_sites_rev", "bg_n_sites", "bg_weighted_mean",
        "bg_share_low", "bg_share_mid", "bg_share_high"]),
    # both strands and contigs: 12 0 2 10, n = 24 (needs 3, 6, 12, 18, 22 -> bins 0 0 0 3 3), coverage 240, modified 120
    _T(["b1", "GATC", "a", "1", "40", "24", "10.000000", "0.500000", "0.000000", "0.000000", "0.000000", "0.750000", "0.750000", "0.500000", "0.083333",
        "0.416667", "0.250000", "0.750000", "bimodal", "14", "10", "100", "0.250000", "0.600000", "0.300000", "0.100000"]),
    _T(["b1", "CCWGG", "m", "1", "3", "0"] + [""] * 10 + ["0.250000", "0.750000", "few_sites", "0", "0"] + [""] * 5)]) + "\n"
HAND_CONTIGS = "\n".join([
    _T(["bin", "contig", "motif", "mod_type", "mod_position", "n_occurrences", "n_sites", "mean_read_cov", "weighted_mean", "share_low", "share_mid",
        "share_high", "q50", "flag"]),
    # c1: 12 0 2 8, n = 22 (q50 needs 11 -> bin 0), coverage 220, modified 100; 8 < 0.9 * 22, 12 < 0.9 * 22, both >= 2.2, 2 < 8
    _T(["b1", "c1", "GATC", "a", "1", "30", "22", "10.000000", "0.454545", "0.545455", "0.090909", "0.363636", "0.000000", "bimodal"]),
    _T(["b1", "c2", "GATC", "a", "1", "10", "2", "10.000000", "1.000000", "0.000000", "0.000000", "1.000000", "0.750000", "few_sites"]),
    _T(["b1", "c2", "CCWGG", "m", "1", "3", "0"] + [""] * 6 + ["few_sites"])]) + "\n"
HAND_HIST_HEAD = """\
bin	motif	mod_type	mod_position	background	strand	bin_index	lower	upper	n_sites
b1	A	a	0	1	+	0	0.000000	0.250000	60
b1	A	a	0	1	+	1	0.250000	0.500000	20
b1	A	a	0	1	+	2	0.500000	0.750000	10
b1	A	a	0	1	+	3	0.750000	1.000000	10
b1	A	a	0	1	-	0	0.000000	0.250000	0
"""


def test_format_files_on_a_hand_table():
    """B = 4, edges 1 / 3, 20 sites, t = 0.1.  GATC_a_1 on c1: '+' 8 0 2 4 (20 occurrences, coverage 140, modified 60), '-' 4 0 0 4 (10, 80,
    40); on c2: '+' 0 0 0 0 (4 occurrences), '-' 0 0 0 2 (6, 20, 20); CCWGG_m_1: 3 occurrences on c2 and none on c1, no site, no
    background (an alias name shows as its contig)."""
    u = lambda x: np.array(x, dtype=np.uint64)
    gatc = u([[[8, 0, 2, 4, 20, 140, 60], [4, 0, 0, 4, 10, 80, 40]], [[0, 0, 0, 0, 4, 0, 0], [0, 0, 0, 2, 6, 20, 20]]])
    ccwgg = u([[[0] * 7, [0] * 7], [[0, 0, 0, 0, 2, 0, 0], [0, 0, 0, 0, 1, 0, 0]]])
    bg = u([[[60, 20, 10, 10, 500, 1000, 250], [0] * 7], [[0] * 7, [0] * 7]])
    names = ["c1", "c2" + fasta.ALIAS_SEP + "b1"]
    cands = [SiteCandidate("b1", "GATC", "a", 1), SiteCandidate("b1", "CCWGG", "m", 1)]
    summary, contigs, hist = mf.format_files(cands, [(names, gatc), (names, ccwgg)], [(("b1", "a"), bg)], 4, 1, 3, 20, 0.1)
    assert summary == HAND_SUMMARY
    assert contigs == HAND_CONTIGS
    lines = hist.splitlines()
    assert hist.startswith(HAND_HIST_HEAD) and len(lines) == 1 + 3 * 8
    assert lines[9:13] == ["b1\tGATC\ta\t1\t0\t+\t%d\t%.6f\t%.6f\t%d" % (k, k / 4, (k + 1) / 4, n) for k, n in enumerate((8, 0, 2, 4))]
    assert lines[13:17] == ["b1\tGATC\ta\t1\t0\t-\t%d\t%.6f\t%.6f\t%d" % (k, k / 4, (k + 1) / 4, n) for k, n in enumerate((4, 0, 0, 6))]
    assert lines[-1] == "b1\tCCWGG\tm\t1\t0\t-\t3\t0.750000\t1.000000\t0"
    assert mf.SUMMARY_HEADER == HAND_SUMMARY.splitlines()[0].split("\t") and len(mf.FLAGS) == 5


def test_the_parser_refuses_bins_out_of_range(capsys):
    from nanomotif_amd.argparser import create_parser
    base = ["motif_fractions", "a.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "m.tsv"]
    args = create_parser().parse_args(base)
    assert (args.bins, args.min_valid_read_coverage, args.min_valid_cov_to_diff_fraction, args.methylation_threshold_low, args.methylation_threshold_high,
            args.min_sites, args.minor_share, args.bin_motifs) == (20, 5, 0.8, 0.3, 0.7, 20, 0.1, ["m.tsv"])
    assert create_parser().parse_args(base + ["--bins", "64", "--bin_motifs", "m.tsv", "n.tsv"]).bins == 64
    for bad in ("1", "65", "x"):
        with pytest.raises(SystemExit) as e:
            create_parser().parse_args(base + ["--bins", bad])
        assert e.value.code == 2 and "--bins takes a number in [2, 64]" in capsys.readouterr().err
    with pytest.raises(ValueError):
        mf.parse_bins(0)


def test_the_loader_and_the_command_refuse_a_contig_listed_under_two_bins(tmp_path, monkeypatch, caplog):
    """The read statistics hold a pileup row once: a contig under two bins is refused before an engine exists, and the command exits 2."""
    from nanomotif_amd import loading
    from nanomotif_amd.argparser import create_parser

    def no_engine(*a, **kw):                                          # pragma: no cover - the refusal comes first
        raise AssertionError("an engine was created")
    monkeypatch.setattr(loading, "ScanEngine", no_engine)
    monkeypatch.setenv("WORLD_SIZE", "1")
    (tmp_path / "cb.tsv").write_text("c1\tbin_a\nc2\tbin_a\nc2\tbin_b\n")
    (tmp_path / "m.tsv").write_text("reference\tmotif\tmod_position\tmod_type\nbin_a\tGATC\t1\ta\n")
    args = create_parser().parse_args(["motif_fractions", str(tmp_path / "a.fasta"), str(tmp_path / "p.bed"), "-c", str(tmp_path / "cb.tsv"),
                                       "--bin_motifs", str(tmp_path / "m.tsv"), "--out", str(tmp_path / "out")])
    with pytest.raises(loading.AliasedContigs, match=r"1 contig\(s\) are listed under several bins \(e\.g\. c2\)"):
        loading.load_readstats_engine(args, 0, ["a"])
    with caplog.at_level("ERROR"):
        assert mf.run(args) == 2
    assert "listed under several bins" in caplog.text
    # the multi-rank refusal and the edge refusal come before anything is read
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert mf.run(args) == 2
    monkeypatch.setenv("WORLD_SIZE", "1")
    args.methylation_threshold_low, args.bins = 0.01, 20
    caplog.clear()
    with caplog.at_level("ERROR"):
        assert mf.run(args) == 2
    assert "bin edges 0 / 14 of 20" in caplog.text
    (tmp_path / "empty.tsv").write_text("")
    with pytest.raises(ValueError, match="No bin contig mapping"):
        loading.load_readstats_engine(argparse.Namespace(contig_bin=str(tmp_path / "empty.tsv")), 0, ["a"])
