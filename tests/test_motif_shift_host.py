"""Host side of ``motif_shift`` (no GPU): the brute force of tests/shift_geometry.py on a hand case and against the single-sample brute
force of tests/test_motif_pileup_host.py, the conditions that make its input worth running (counted, not assumed), the shifted rule at
its equalities and beside two wrong restatements, the engine's argument checks and the refusals of the two entry points that need no
device."""
import ctypes as C
import os

import numpy as np
import pytest

import shift_geometry as S
import test_motif_fractions_host as F
import test_motif_pileup_host as P
import test_read_methylation_host as H
from nanomotif_amd.motif import iupac_to_regex
from test_gpu_motif_compare import reach_class

LANE, WORD, BLOCK = 128, 32, 512


def test_the_brute_force_on_a_hand_case():
    """GATC x 3 ('+' A at 1, 5, 9; '-' A at 2, 6, 10).  A: kept (1 +) 10/4, (2 -) 5/5, (5 +) 8/2; dropped (6 -), (9 +).  B: kept (1 +) 5/2
    (equal at another coverage), (5 +) 8/6 (up by 500), (6 -) 4/4 (B only), (10 -) 3/0 (B only); (2 -) dropped by coverage."""
    col = lambda *x: np.array(x, dtype=np.int64)
    rec_a = {("c", "a"): dict(position=col(1, 2, 3, 5, 6, 9), strand=np.frombuffer(b"+-++-+", np.uint8), n_valid=col(10, 5, 9, 8, 2, 8), n_mod=col(4, 5, 9, 2, 1, 8),
                              n_diff=col(0, 0, 0, 2, 0, 3))}
    rec_b = {("c", "a"): dict(position=col(1, 2, 5, 6, 10), strand=np.frombuffer(b"+-+--", np.uint8), n_valid=col(5, 2, 8, 4, 3), n_mod=col(2, 2, 6, 4, 0),
                              n_diff=col(0, 0, 0, 1, 0))}
    seqs, bins_of, cands = {"c": "GATC" * 3, "d": "TTGATC"}, {"b": ["c", "d"]}, [("GATC", "a", 1, "b")]
    join = S.join_records(["c", "d"], seqs, rec_a, rec_b, bins_of, cands)
    assert [(int(r["contig"]), int(r["pos"]), int(r["strand"]), int(r["cls"]), int(r["dir"]), int(r["tmax"])) for r in join] == [
        (0, 1, 0, S.PAIRED, S.EQUAL, 0), (0, 2, 1, S.ONLY_A, 0, 0), (0, 5, 0, S.PAIRED, S.UP, 500), (0, 6, 1, S.ONLY_B, 0, 0), (0, 9, 0, S.BARE, 0, 0),
        (0, 10, 1, S.ONLY_B, 0, 0), (1, 3, 0, S.BARE, 0, 0), (1, 4, 1, S.BARE, 0, 0)]
    (t,) = S.tables(join, ["c", "d"], bins_of, cands, 2, 500)
    #                    hist 00 01 10 11 | occ paired only_a only_b | sums            | up down shift_up shift_down
    assert t[0].tolist() == [[1, 1, 0, 0, 3, 2, 0, 0, 18, 6, 13, 8, 1, 0, 1, 0], [0, 0, 0, 0, 3, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0]]
    assert t[1].tolist() == [[0, 0, 0, 0, 1] + [0] * 11, [0, 0, 0, 0, 1] + [0] * 11]
    assert S.tables(join, ["c", "d"], bins_of, cands, 2, 501)[0][0, 0, 4:].tolist() == [3, 2, 0, 0, 18, 6, 13, 8, 1, 0, 0, 0]
    assert S.records(join, 500, ("up", "down")).tolist() == [(0, 0, 5, 0, 8, 2, 8, 6)] and len(S.records(join, 500, ("down",))) == len(S.records(join, 501, ("up",))) == 0
    swapped = S.join_records(["c", "d"], seqs, rec_b, rec_a, bins_of, cands)
    assert S.records(swapped, 0, ("up", "down")).tolist() == [(0, 0, 5, S.DOWN_BIT, 8, 6, 8, 2)]


def test_the_single_sample_marginals_are_the_pileup_brute_force():
    names, seqs, rec_a, rec_b, cands, join = S.geometry()
    assert P.geometry()[3] == cands
    for rec, v, m, has in ((P.geometry()[4], "va", "ma", (S.PAIRED, S.ONLY_A)), (P.brute_records(names, seqs, rec_b, F.BINS_OF, cands), "vb", "mb", (S.PAIRED, S.ONLY_B))):
        assert len(rec) == len(join)
        for f in ("candidate", "contig", "pos"):
            assert np.array_equal(rec[f], join[f]), f
        site = np.isin(join["cls"], has)
        assert np.array_equal(rec["code"], join["strand"] * P.MINUS_BIT + ~site * P.BARE_BIT)
        assert np.array_equal(rec["n_valid"], np.where(site, join[v], 0)) and np.array_equal(rec["n_mod"], np.where(site, join[m], 0))


def test_the_input_holds_every_case_the_kernel_can_get_wrong():
    names, seqs, rec_a, rec_b, cands, join = S.geometry()
    da, db = F.dense_records(seqs, rec_a), F.dense_records(seqs, rec_b)
    # the four classes on both strands in all three reach classes
    reach = np.array([reach_class(iupac_to_regex(m), pos) for m, _, pos, _ in cands])
    seen = {(int(r), int(s), int(c)) for r, s, c in zip(reach[join["candidate"]], join["strand"], join["cls"])}
    assert seen == {(r, s, c) for r in (0, 1, 2) for s in (0, 1) for c in (S.PAIRED, S.ONLY_A, S.ONLY_B, S.BARE)}
    # records of ONE sample before a paired site: in an earlier lane of its rank block, and below its bit in its own word
    n = dict(lane_b=0, lane_a=0, word_b=0, word_a=0, last_bit=0, both_in_lane=0)
    pair = join[join["cls"] == S.PAIRED]
    for k, contig, pos, s in zip(pair["candidate"].tolist(), pair["contig"].tolist(), pair["pos"].tolist(), pair["strand"].tolist()):
        key = (names[contig], cands[k][1])
        a, b = da[key][0][s] >= 0, db[key][0][s] >= 0
        block0, lane0, word0 = pos // BLOCK * BLOCK, pos // LANE * LANE, pos // WORD * WORD
        n["lane_b"] += bool((b[block0:lane0] & ~a[block0:lane0]).any())
        n["lane_a"] += bool((a[block0:lane0] & ~b[block0:lane0]).any())
        n["word_b"] += bool((b[word0:pos] & ~a[word0:pos]).any())
        n["word_a"] += bool((a[word0:pos] & ~b[word0:pos]).any())
        n["both_in_lane"] += bool((b[lane0:word0] & ~a[lane0:word0]).any() and (a[lane0:word0] & ~b[lane0:word0]).any())
        n["last_bit"] += pos % BLOCK == BLOCK - 1
    print(n, "paired", len(pair))
    assert min(n["lane_b"], n["lane_a"], n["word_b"], n["word_a"], n["both_in_lane"]) > 1_000 and n["last_bit"] > 20
    # the planted sites of `long`: paired on the last bit of a rank block and either side of the 64-block carry, with the planted values
    gatc = cands.index(("GATC", "a", 1, "b2"))
    mine = join[(join["candidate"] == gatc) & (join["contig"] == names.index("long"))]
    got = {(int(r["pos"]), int(r["strand"])): r for r in mine}
    for (_, pos, strand), (vb, mb) in S.PLANTS_B.items():
        r = got[(pos, 1 if strand == H.MINUS else 0)]
        assert r["cls"] == S.PAIRED and (int(r["va"]), int(r["ma"])) == H.PLANTED[("long", pos, strand)] and (int(r["vb"]), int(r["mb"])) == (vb, mb)
    assert (got[(511, 0)]["dir"], got[(32_767, 0)]["dir"], got[(32_768, 1)]["dir"]) == (S.EQUAL, S.UP, S.EQUAL) and 511 % BLOCK == BLOCK - 1 and 32_768 % (64 * BLOCK) == 0
    assert [(int(got[k]["dir"]), int(got[k]["tmax"])) for k in ((512, 1), (36_863, 0), (36_864, 1), (H.LANES_SITE, 0))] == [(S.DOWN, 500), (S.DOWN, 500), (S.UP, 500), (S.UP, 58)]
    # a contig with A records only and one with B records only, each between two contigs with both
    t = S.tables(join, names, F.BINS_OF, cands, 2, 250)
    a_cand = cands.index(("A", "a", 0, "b1"))
    rows = {name: t[a_cand][i, :, 4:].sum(axis=0) for i, name in enumerate(F.BINS_OF["b1"])}
    assert F.BINS_OF["b1"][3:] == ["small", S.A_ONLY_CONTIG, "mid"] and rows["edge"][2] > 100 and rows["edge"][[1, 3]].sum() == 0
    print({x: rows[x].tolist() for x in rows})
    assert all(rows[x][1] > 10 for x in ("small", "mid"))                                    # paired sites: records of both samples
    a_cand = cands.index(("A", "a", 0, "b2"))
    rows = {name: t[a_cand][i, :, 4:].sum(axis=0) for i, name in enumerate(F.BINS_OF["b2"])}
    assert F.BINS_OF["b2"][:3] == ["long", S.B_ONLY_CONTIG, "endGA"] and rows["norec"][3] > 100 and rows["norec"][[1, 2]].sum() == 0
    assert all(rows[x][1] > 10 for x in ("long", "endGA"))
    # kept in A and dropped in B by each of the two filters, at a motif site
    only_a = join[join["cls"] == S.ONLY_A]
    by_cov = by_diff = 0
    raw_b = {key: {(p, st): (nv, nd) for p, st, nv, nd in zip(r["position"].tolist(), r["strand"].tolist(), r["n_valid"].tolist(), r["n_diff"].tolist())} for key, r in rec_b.items()}
    for k, contig, pos, s in zip(only_a["candidate"].tolist(), only_a["contig"].tolist(), only_a["pos"].tolist(), only_a["strand"].tolist()):
        r = raw_b.get((names[contig], cands[k][1]), {}).get((pos, H.MINUS if s else H.PLUS))
        if r is not None:
            by_cov += r[0] < H.MIN_COV
            by_diff += r[0] >= H.MIN_COV and r[0] / (r[0] + r[1]) < H.MIN_FRAC
    assert by_cov > 500 and by_diff > 500
    # equal fractions at another coverage, the threshold equality, and every direction on every strand
    quad = set(zip(pair["va"].tolist(), pair["ma"].tolist(), pair["vb"].tolist(), pair["mb"].tolist()))
    assert (4, 2, 6, 3) in quad and (4, 1, 4, 3) in quad and int(((pair["dir"] == S.EQUAL) & (pair["va"] != pair["vb"]) & (pair["ma"] > 0)).sum()) > 1_000
    assert int((pair["tmax"] == 500).sum()) > 100 and int((pair["tmax"] == 250).sum()) > 50 and int((pair["tmax"] == 1000).sum()) > 100
    for s in (0, 1):
        assert np.bincount(pair["dir"][pair["strand"] == s], minlength=3).min() > 3_000
    for B in S.ALL_B:                                                                        # no cell of the joint table is out of reach
        total = sum(x[:, :, :B * B].sum(axis=(0, 1)) for x in S.tables(join, names, F.BINS_OF, cands, B, 0))
        assert (total > 0).all(), B
    assert 150_000 < len(join) < 400_000 and len(rec_b) >= 2 * (len(names) - 1) - 2


def test_the_rule_at_its_equalities():
    assert S.judge(4, 1, 4, 3) == (S.UP, 500) and S.shifted(4, 1, 4, 3, 500) and not S.shifted(4, 1, 4, 3, 501)
    assert S.judge(4, 3, 4, 1) == (S.DOWN, 500) and S.judge(4, 2, 6, 3) == (S.EQUAL, 0) and not S.shifted(4, 2, 6, 3, 0)
    assert S.shifted(17, 5, 17, 6, 58) and not S.shifted(17, 5, 17, 6, 59) and S.shifted(3, 1, 3, 2, 0) and S.shifted(5, 0, 9, 9, 1000)
    for va, ma, vb, mb in S.LARGE_SITES:
        d, tmax = S.judge(va, ma, vb, mb)
        for t in range(0, 1001, 1 if max(va, vb) < 100 else 37):
            assert S.shifted(va, ma, vb, mb, t) == (d != S.EQUAL and t <= tmax)
    assert [site for site in S.LARGE_SITES if max(site) == S.BIG] and all(0 <= x < 1 << 31 and v >= 1 for va, ma, vb, mb in S.LARGE_SITES for x, v in ((ma, va), (mb, vb)))
    assert [S.site_bin(m, 4, 4) for m in range(5)] == [0, 1, 2, 3, 3] and S.site_bin(S.BIG, S.BIG, 16) == 15 and S.site_bin(S.BIG - 1, S.BIG, 16) == 15


def test_two_wrong_restatements_misjudge_the_planted_large_coverages():
    """The rule in wrapping 64-bit arithmetic and the rule in float64, run beside the right one on ``S.LARGE_SITES``: each misjudges at
    least one planted site, in direction or in shifted, at a threshold the GPU suite runs; neither misjudges the small equality."""
    wrong = {"wrapping": set(), "float": set()}
    for i, site in enumerate(S.LARGE_SITES):
        for t in S.ALL_T:
            right = (S.judge(*site)[0], S.shifted(*site, t))
            if S.judge_wrapping(*site, t) != right:
                wrong["wrapping"].add((i, t))
            if S.judge_float(*site, t) != right:
                wrong["float"].add((i, t))
    print(wrong)
    assert wrong["wrapping"] and wrong["float"] and not {i for i, _ in wrong["wrapping"]} & {i for i, _ in wrong["float"]} & {0}
    assert all(i != 0 for i, _ in wrong["wrapping"] | wrong["float"])
    assert {i for i, _ in wrong["float"]} >= {1, 2}                                          # two fractions 2^-62 apart are one float64
    names, seqs, rec_a, rec_b, bins_of, cands = S.large_input()
    join = S.join_records(names, seqs, rec_a, rec_b, bins_of, cands)
    pair = join[join["cls"] == S.PAIRED]
    assert list(zip(pair["va"].tolist(), pair["ma"].tolist(), pair["vb"].tolist(), pair["mb"].tolist())) == S.LARGE_SITES and (pair["strand"] == 0).all()


def test_the_engine_checks_its_arguments_before_the_library_is_called():
    from nanomotif_amd import engine as E
    assert [E.shift_select(s) for s in (("up",), ("down",), ("up", "down"), ("down", "up", "up"))] == [1, 2, 3, 3]
    for bad in ((), ("equal",), ("up", "sideways")):
        with pytest.raises(ValueError, match="direction"):
            E.shift_select(bad)
    assert [E.shift_permille(t) for t in (0, 250, 1000, 250.0)] == [0, 250, 1000, 250]
    for bad in (-1, 1001, 0.25, 250.5):
        with pytest.raises(ValueError, match="min_delta_permille"):
            E.shift_permille(bad)
    assert E.SHIFT_DTYPE == S.RECORD and E.SHIFT_RECORD_BYTES == 25 == sum(E.SHIFT_DTYPE[f].itemsize for f in E.SHIFT_DTYPE.names if f != "candidate")
    assert E.SHIFT_SUMS == S.SUMS and E.SHIFT_EXTRA == S.EXTRA == len(S.SUMS) and (E.SHIFT_MIN_BINS, E.SHIFT_MAX_BINS) == (2, 16) == (S.ALL_B[0], S.ALL_B[-1])
    assert (E.SHIFT_MINUS, E.SHIFT_DOWN, E.SHIFT_SLOT_B) == (S.MINUS_BIT, S.DOWN_BIT, 3)


def test_the_unit_is_built_and_bound():
    from nanomotif_amd import _lib, build
    assert os.path.join("csrc", "nmshift.hip") in [os.path.relpath(s, os.path.dirname(build.__file__)) for s in build.SRC_HIP]
    header = open(build.HEADER).read()
    for name in ("nm_motif_shift_count", "nm_motif_shift_sites"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS
    for define in ("NM_SHIFT_MIN_BINS 2", "NM_SHIFT_MAX_BINS 16", "NM_SHIFT_EXTRA 12", "NM_SHIFT_UP 1u", "NM_SHIFT_DOWN 2u", "NM_SHIFT_CODE_DOWN 1u", "NM_SHIFT_MINUS 4u"):
        assert f"#define {define}" in header
    lib = _lib.load()                                                 # refusals that need no device, in their order
    assert lib.nm_abi_version() == 1
    u64 = (C.c_uint64 * 2)()
    count = lambda B, t, ctx=None: lib.nm_motif_shift_count(ctx, 0, None, None, None, None, None, None, None, B, t, None)
    for B, text in ((0, b"n_bins 0"), (1, b"n_bins 1"), (17, b"n_bins 17")):
        assert count(B, 2000) == -1 and text in lib.nm_last_error()
    assert count(10, 1001) == -1 and b"min_delta_permille 1001" in lib.nm_last_error()
    assert count(10, 1000) == -1 and b"ctx" in lib.nm_last_error()
    sites = lambda t, select, off=u64, written=u64: lib.nm_motif_shift_sites(None, 0, None, None, None, None, None, None, None, t, select, 0, 0, None, None, None, None, None,
                                                                              None, None, off, written)
    assert sites(1001, 0) == -1 and b"min_delta_permille 1001" in lib.nm_last_error()
    for select, text in ((0, b"select 0"), (4, b"select 4"), (7, b"select 7")):
        assert sites(1000, select) == -1 and text in lib.nm_last_error()
    assert sites(0, 3) == -1 and b"ctx" in lib.nm_last_error()
    assert sites(0, 3, off=None) == -1 and b"NULL" in lib.nm_last_error() and sites(1001, 0, written=None) == -1 and b"NULL" in lib.nm_last_error()


def test_a_second_pileup_goes_to_a_slot_of_its_own():
    """``upload_read_statistics(..., slot=)``: the library is called with that slot and the code does not become resident for the
    single-sample calls; without it the call is the one it was."""
    from nanomotif_amd import contig_methylation as cm

    class Lib:
        def __init__(self):
            self.slots = []

        def nm_readstats_upload(self, ctx, slot, n, *rest):
            self.slots.append((slot, n))
            return 0

    class Engine:
        def __init__(self):
            self.lib, self.ctx, self.readstats_mods = Lib(), None, set()
    eng = Engine()
    cols = (np.zeros(2, np.uint32), np.array([1, 2]), np.frombuffer(b"+-", np.uint8), np.array([5, 6]), np.array([1, 2]))
    cm.upload_read_statistics(eng, "a", *cols)
    assert eng.lib.slots == [(1, 2)] and eng.readstats_mods == {"a"}
    cm.upload_read_statistics(eng, "m", *cols, slot=3)
    assert eng.lib.slots == [(1, 2), (3, 2)] and eng.readstats_mods == {"a"}
    cm.upload_read_statistics(eng, "m", *cols, slot=0)
    assert eng.lib.slots[-1] == (0, 2) and eng.readstats_mods == {"a", "m"}


# ------------------------------------------------------------------------------------------------ the command's host side
def test_the_parser_has_the_defaults_and_refuses_what_is_out_of_range(capsys):
    from nanomotif_amd import motif_shift as msh
    from nanomotif_amd.argparser import create_parser
    base = ["motif_shift", "a.fasta", "pa.bed", "pb.bed", "-c", "cb.tsv", "--bin_motifs", "m.tsv"]
    args = create_parser().parse_args(base)
    assert (args.command, args.assembly, args.pileup_a, args.pileup_b, args.contig_bin, args.bin_motifs, args.out, args.bins, args.min_delta, args.shifted_sites,
            args.directions, args.min_sites, args.min_share, args.minor_share, args.min_valid_read_coverage, args.min_valid_cov_to_diff_fraction,
            args.methylation_threshold_low, args.methylation_threshold_high, args.device) == (
        "motif_shift", "a.fasta", "pa.bed", "pb.bed", "cb.tsv", ["m.tsv"], "nanomotif", 10, 250, False, ("up", "down"), 20, 0.5, 0.1, 5, 0.8, 0.3, 0.7, None)
    args = create_parser().parse_args(base + ["n.tsv", "--bins", "16", "--min_delta", "0.125", "--shifted_sites", "--directions", "down", "--min_sites", "5",
                                              "--min_share", "0.6", "--minor_share", "0.2"])
    assert (args.bin_motifs, args.bins, args.min_delta, args.shifted_sites, args.directions, args.min_sites, args.min_share, args.minor_share) == (
        ["m.tsv", "n.tsv"], 16, 125, True, ("down",), 5, 0.6, 0.2)
    assert create_parser().parse_args(base + ["--directions", "down,up"]).directions == ("up", "down")
    assert [msh.parse_min_delta(x) for x in ("0", "1", "0.25", "0.001", "1.000", "0.5", "0.50", " 0.7 ")] == [0, 1000, 250, 1, 1000, 500, 500, 700]
    for bad in ("1.001", "2", "-0.1", "0.2500", "1e-1", "", ".", "0.", "a", "0.25x"):
        with pytest.raises(ValueError, match="--min_delta"):
            msh.parse_min_delta(bad)
    assert [msh.parse_bins(x) for x in ("2", "10", 16)] == [2, 10, 16]
    for bad in ("1", "17", "64", "x"):
        with pytest.raises(ValueError, match="--bins"):
            msh.parse_bins(bad)
    for bad in (["--bins", "17"], ["--min_delta", "0.2500"], ["--directions", "sideways"], ["--directions", ""], ["--states", "mod"]):
        with pytest.raises(SystemExit) as e:
            create_parser().parse_args(base + bad)
        assert e.value.code == 2 and capsys.readouterr().err
    with pytest.raises(SystemExit):
        create_parser().parse_args(base[:3] + base[4:])                   # one pileup only
    assert "motif_shift" in create_parser().format_help()


def test_the_parser_spec_follows_the_other_exports():
    """What ``tests/test_export_run_host.py`` records of the other commands, for the new one: positionals, the exclusive group, the option
    order of the shared blocks."""
    from test_export_run_host import dump_actions
    got = dump_actions(["motif_shift", "motif_fractions", "motif_compare"])
    spec, fr, cmp_ = got["motif_shift"], got["motif_fractions"], got["motif_compare"]
    assert spec["positionals"] == cmp_["positionals"] == ["assembly", "pileup_a", "pileup_b"] and spec["exclusive"] == [[True, ["contig_bin", "files", "directory"]]]
    dests = [a[2] for a in spec["actions"]]
    assert dests == ["assembly", "pileup_a", "pileup_b", "contig_bin", "files", "directory", "extension", "bin_motifs", "out", "bins", "min_delta", "shifted_sites",
                     "directions", "min_valid_read_coverage", "min_valid_cov_to_diff_fraction", "methylation_threshold_low", "methylation_threshold_high", "min_sites",
                     "min_share", "minor_share", "device", "threads", "verbose", "seed", "help"]
    shared = lambda s, names: [a for a in s["actions"] if a[2] in names]
    same = ("contig_bin", "files", "directory", "extension", "bin_motifs", "out", "min_valid_read_coverage", "min_valid_cov_to_diff_fraction", "methylation_threshold_low",
            "methylation_threshold_high", "device", "threads", "verbose", "seed", "help")
    assert shared(spec, same) == shared(fr, same)
    assert shared(spec, ("pileup_a", "pileup_b")) == shared(cmp_, ("pileup_a", "pileup_b"))


def _hand_table(rows):
    """uint64[len(rows), 2, 4 + 12] at 2 bins from per-row, per-strand (hist00, hist01, hist10, hist11, sums ...)."""
    return np.array(rows, dtype=np.uint64).reshape(len(rows), 2, 16)


def test_the_three_tables_and_the_bed_on_hand_made_input():
    from nanomotif_amd import fasta, motif_shift as msh
    from nanomotif_amd.motif_sites import SiteCandidate
    assert msh.FLAGS == ("few_sites", "gained", "lost", "mixed", "stable")
    # every flag, first match first: n, shift_up, shift_down at 20 sites, 0.5, 0.1
    for n, u, d, want in ((19, 19, 0, "few_sites"), (20, 10, 1, "gained"), (20, 10, 2, "mixed"), (20, 1, 10, "lost"), (20, 2, 10, "mixed"), (20, 9, 1, "stable"),
                          (20, 2, 2, "mixed"), (20, 0, 0, "stable"), (0, 0, 0, "few_sites"), (100, 50, 9, "gained"), (100, 49, 9, "stable"), (100, 50, 10, "mixed")):
        assert msh.flag_of(n, u, d, 20, 0.5, 0.1) == want, (n, u, d)
    cands = [SiteCandidate("binA", "GATC", "a", 1), SiteCandidate("binA", "CCWGG", "m", 1)]
    names = ["c1", "c2" + fasta.ALIAS_SEP + "binB", "c3"]
    #        hist 00 01 10 11 | occ paired only_a only_b | valid_a mod_a valid_b mod_b | up down shift_up shift_down
    gatc = _hand_table([[[2, 18, 0, 4, 30, 24, 3, 2, 240, 24, 480, 360, 20, 1, 18, 0], [0, 0, 0, 0, 5, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0]],
                        [[0] * 16, [0] * 16],
                        [[1, 0, 0, 0, 1, 1, 0, 0, 7, 0, 7, 0, 0, 0, 0, 0], [0] * 16]])
    ccwgg = _hand_table([[[0] * 4 + [3, 0, 1, 0] + [0] * 8, [0] * 16], [[0] * 16, [0] * 16], [[0] * 16, [0] * 16]])
    bg = _hand_table([[[10, 10, 5, 15, 100, 40, 30, 20, 400, 200, 400, 240, 12, 8, 10, 5], [0] * 16]])
    main, contigs, hist = msh.format_files(cands, [(names, gatc), (names, ccwgg)], [(("binA", "a"), bg)], 2, 1, 1)
    assert main.splitlines()[0].split("\t") == msh.SUMMARY_HEADER and contigs.splitlines()[0].split("\t") == msh.CONTIGS_HEADER and hist.splitlines()[0].split("\t") == msh.HIST_HEADER
    rows = [dict(zip(msh.SUMMARY_HEADER, line.split("\t"))) for line in main.splitlines()[1:]]
    assert len(rows) == 2
    g = rows[0]
    assert [g[k] for k in msh.KEY_COLUMNS + msh.CLASS_COLUMNS] == ["binA", "GATC", "a", "1", "36", "25", "3", "7", "1"]
    assert [g[k] for k in msh.MEAN_COLUMNS] == ["9.880000", "0.097166", "19.480000", "0.739220", "0.642054"]          # 247 / 25, 24 / 247, 487 / 25, 360 / 487
    assert [g[k] for k in ("n_up", "n_down", "n_equal", "sign_p", "n_shift_up", "n_shift_down", "flag")] == ["20", "1", "4", "%.6g" % (2 * 22 / 2 ** 21), "18", "0", "gained"]
    assert [g["n_%s_%s" % (a, b)] for a in ("low", "mid", "high") for b in ("low", "mid", "high")] == ["3", "0", "18", "0", "0", "0", "0", "0", "4"]
    assert [g[k] for k in ("bg_n_paired", "bg_weighted_mean_a", "bg_weighted_mean_b", "bg_delta", "excess_delta")] == ["40", "0.500000", "0.600000", "0.100000", "0.542054"]
    c = rows[1]
    assert [c[k] for k in msh.CLASS_COLUMNS + msh.MEAN_COLUMNS] == ["3", "0", "1", "0", "2", "", "", "", "", ""] and c["sign_p"] == "nan" and c["flag"] == "few_sites"
    assert [c[k] for k in ("bg_n_paired", "bg_delta", "excess_delta")] == ["", "", ""]                                 # no background of (binA, m) was read
    crow = [line.split("\t") for line in contigs.splitlines()[1:]]
    assert [r[:2] + r[5:10] + r[-1:] for r in crow] == [["binA", "c1", "35", "24", "3", "7", "1", "gained"], ["binA", "c3", "1", "1", "0", "0", "0", "few_sites"],
                                                         ["binA", "c1", "3", "0", "1", "0", "2", "few_sites"]]                # the aliased, empty c2 has no row
    assert [line.split("\t") for line in hist.splitlines()[1:]] == [
        ["binA", "A", "a", "0", "1", "+", "0", "0", "10"], ["binA", "A", "a", "0", "1", "+", "0", "1", "10"], ["binA", "A", "a", "0", "1", "+", "1", "0", "5"],
        ["binA", "A", "a", "0", "1", "+", "1", "1", "15"], ["binA", "GATC", "a", "1", "0", "+", "0", "0", "3"], ["binA", "GATC", "a", "1", "0", "+", "0", "1", "18"],
        ["binA", "GATC", "a", "1", "0", "+", "1", "1", "4"]]
    rec = np.array([(0, 0, 9, 0, 10, 1, 20, 15), (0, 1, 4_294_967_294, 5, 4, 3, 4, 1), (1, 2, 0, 4, 2_147_483_647, 0, 3, 3)], dtype=S.RECORD)
    assert msh.format_bed(rec, cands, ["c1", "c2", "c3"]) == ("c1\t9\t10\tGATC_a_1\t0\t+\t10\t1\t20\t15\tup\tbinA\n"
                                                               "c2\t4294967294\t4294967295\tGATC_a_1\t0\t-\t4\t3\t4\t1\tdown\tbinA\n"
                                                               "c3\t0\t1\tCCWGG_m_1\t0\t-\t2147483647\t0\t3\t3\tup\tbinA\n")
    assert msh.format_bed(rec[:0], cands, ["c1"]) == "" and (msh.SUMMARY_NAME, msh.CONTIGS_NAME, msh.HIST_NAME, msh.BED_NAME) == (
        "motif-shift.tsv", "motif-shift-contigs.tsv", "motif-shift-hist.tsv", "shifted-sites.bed")


def test_the_opening_refuses_in_the_order_of_the_other_exports(tmp_path, monkeypatch, caplog):
    """Bad zone edges before anything is opened, then the multi-rank launch, then the aliased contig — before an engine exists; a second
    pileup reaches the loader as ``pileups``."""
    from nanomotif_amd import export_run, loading, motif_shift as msh
    from nanomotif_amd.argparser import create_parser

    def no_engine(*a, **kw):                                          # pragma: no cover - the refusals come first
        raise AssertionError("an engine was created")
    monkeypatch.setattr(loading, "ScanEngine", no_engine)
    (tmp_path / "cb.tsv").write_text("c1\tbin_a\nc2\tbin_a\nc2\tbin_b\n")
    (tmp_path / "m.tsv").write_text("reference\tmotif\tmod_position\tmod_type\nbin_a\tGATC\t1\ta\n")
    base = ["motif_shift", str(tmp_path / "a.fasta"), str(tmp_path / "pa.bed"), str(tmp_path / "pb.bed"), "-c", str(tmp_path / "cb.tsv"), "--bin_motifs",
            str(tmp_path / "m.tsv"), "--out", str(tmp_path / "out")]
    monkeypatch.setenv("WORLD_SIZE", "2")
    with caplog.at_level("ERROR"):
        assert msh.run(create_parser().parse_args(base + ["--methylation_threshold_low", "0.01"])) == 2
    assert "snap to the bin edges" in caplog.text and "multi-rank" not in caplog.text
    caplog.clear()
    with caplog.at_level("ERROR"):
        assert msh.run(create_parser().parse_args(base)) == 2
    assert "motif_shift runs on one GPU" in caplog.text
    caplog.clear()
    monkeypatch.setenv("WORLD_SIZE", "1")
    with caplog.at_level("ERROR"):
        assert msh.run(create_parser().parse_args(base)) == 2
    assert "motif_shift" in caplog.text and "listed under several bins (e.g. c2)" in caplog.text and not os.path.exists(tmp_path / "out" / msh.SUMMARY_NAME)
    seen = {}

    def fake_loader(args, device, mod_types, **kw):
        seen.update(kw, mod_types=mod_types)
        raise loading.AliasedContigs("stop here")
    monkeypatch.setattr(export_run, "load_readstats_engine", fake_loader)
    assert msh.run(create_parser().parse_args(base)) == 2
    assert seen == {"pileups": (str(tmp_path / "pa.bed"), str(tmp_path / "pb.bed")), "mod_types": ["a"]}
    seen.clear()
    assert export_run.open_readstats_run("motif_fractions", create_parser().parse_args(["motif_fractions"] + base[1:2] + base[3:]), {})[2] == 2
    assert seen == {"mod_types": ["a"]}                                   # one pileup: the loader is called exactly as before
