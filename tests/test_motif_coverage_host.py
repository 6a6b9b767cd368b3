"""Host side of ``nanomotif motif_coverage`` (no GPU): the sub-command's arguments, the sets built from a bin-motifs.tsv, the three TSV
formatters on hand-made tables, and the two new exports in the header and in ``_lib.SYMBOLS``."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_accepts_motif_coverage_and_requires_bin_motifs():
    p = create_parser()
    a = p.parse_args(["motif_coverage", "asm.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "cov"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.bin_motifs, a.out) == ("motif_coverage", "asm.fasta", "pileup.bed", "contig_bin.tsv",
                                                                                      "out/bin-motifs.tsv", "cov")
    assert a.unexplained_sites is False
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose) == (0.3, 0.7, 5, None, False)
    a = p.parse_args(["motif_coverage", "asm.fasta", "pileup.bed.gz", "-d", "bins", "--bin_motifs", "b.tsv", "--unexplained_sites",
                      "--methylation_threshold_low", "0.1", "--methylation_threshold_high", "0.9", "--device", "1", "-v"])
    assert a.unexplained_sites is True and a.directory == "bins"
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.device, a.verbose) == (0.1, 0.9, 1, True)
    a = p.parse_args(["motif_coverage", "asm.fasta", "pileup.bed", "-f", "b1.fa", "b2.fa", "--bin_motifs", "b.tsv"])
    assert a.files == ["b1.fa", "b2.fa"]
    with pytest.raises(SystemExit):                                     # --bin_motifs and one of -c / -f / -d are required
        p.parse_args(["motif_coverage", "asm.fasta", "pileup.bed", "-c", "cb.tsv"])
    with pytest.raises(SystemExit):
        p.parse_args(["motif_coverage", "asm.fasta", "pileup.bed", "--bin_motifs", "b.tsv"])
    assert "motif_coverage" in p.format_help()


def test_multi_rank_launch_is_refused(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), WORLD_SIZE="2", RANK="0", NANOMOTIF_NO_EARLY_INIT="1")
    r = subprocess.run([sys.executable, "-c", "from nanomotif_amd.main import main; main()", "motif_coverage", "a.fasta", "p.bed", "-c", "cb.tsv",
                        "--bin_motifs", "b.tsv", "--out", "o"], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "one GPU" in r.stderr
    assert not os.path.exists(tmp_path / "o")


BIN_MOTIFS = """reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement
bin_b\tGATC\t1\ta\t700\t20\tpalindrome\t\t\t\t
bin_a\tGAAGY\t2\ta\t400\t9\tnon-palindrome\tRCTTC\t3\t395\t14
bin_a\tCCWGG\t1\tm\t300\t7\tpalindrome\t\t\t\t
bin_a\tGATC\t1\ta\t910\t12\tpalindrome\t\t\t\t
bin_a\tGATC\t1\ta\t910\t12\tpalindrome\t\t\t\t
bin_zz\tGATC\t1\ta\t5\t1\tpalindrome\t\t\t\t
bin_b\tGATC\t1\th\t5\t1\tpalindrome\t\t\t\t
"""


def test_sets_of_a_hand_written_bin_motifs(tmp_path):
    from nanomotif_amd.motif_coverage import build_sets
    from nanomotif_amd.motif_sites import candidates_of_bin_motifs
    path = tmp_path / "bin-motifs.tsv"
    path.write_text(BIN_MOTIFS)
    cands = candidates_of_bin_motifs(str(path))
    # bins come sorted whatever order they are given in; mod types in the order given (slot order); bin_c has no motif at all
    sets = build_sets(["bin_c", "bin_b", "bin_a"], ["m", "a"], cands)
    assert [(s.bin, s.mod_type) for s in sets] == [("bin_a", "m"), ("bin_a", "a"), ("bin_b", "m"), ("bin_b", "a"), ("bin_c", "m"), ("bin_c", "a")]
    assert [[c.name for c in s.candidates] for s in sets] == [["CCWGG_m_1"], ["GAAGY_a_2", "RCTTC_a_3", "GATC_a_1"], [], ["GATC_a_1"], [], []]
    b, mt, motifs = sets[1].engine_set()
    assert (b, mt) == ("bin_a", "a") and [(m.string, m.mod_position) for m in motifs] == [("GAAG[CT]", 2), ("[AG]CTTC", 3), ("GATC", 1)]
    assert sets[4].engine_set() == ("bin_c", "m", [])
    # candidates of a bin without contigs (bin_zz) or of a mod type the pileup lacks (h) belong to no set
    assert all(c.bin != "bin_zz" and c.mod_type != "h" for s in sets for c in s.candidates)


def _tables():
    from nanomotif_amd.motif_coverage import CoverageSet
    from nanomotif_amd.motif_sites import SiteCandidate
    sets = [CoverageSet("b1", "a", [SiteCandidate("b1", "GATC", "a", 1), SiteCandidate("b1", "RGATCY", "a", 2)]),
            CoverageSet("b1", "m", []),
            CoverageSet("b2", "a", [SiteCandidate("b2", "GCACNNNNNNGTT", "a", 2)])]
    names = [["c1", "c2"], ["c1", "c2"], ["c3"]]
    #            fwd: mod expl nomod ncov nocall   rev: mod expl nomod ncov nocall
    tables = [np.array([[10, 7, 4, 1, 100, 5, 3, 2, 0, 50], [1, 0, 0, 0, 9, 2, 2, 6, 5, 8]], dtype=np.int64),
              np.array([[0, 0, 3, 0, 0, 0, 0, 4, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int64),
              np.array([[3, 1, 0, 0, 2, 0, 0, 0, 0, 1]], dtype=np.int64)]
    return sets, names, tables


def test_set_table_formatter_sums_strands_and_contigs():
    from nanomotif_amd.motif_coverage import SETS_HEADER, format_sets
    sets, _, tables = _tables()
    lines = format_sets(sets, tables).split("\n")
    assert lines[-1] == "" and len(lines) == 5
    assert lines[0].split("\t") == SETS_HEADER == ["bin", "mod_type", "n_motifs", "n_mod", "n_mod_explained", "n_mod_unexplained", "fraction_explained",
                                                   "n_nomod", "n_nomod_covered", "n_nocall_covered"]
    assert lines[1] == "b1\ta\t2\t18\t12\t6\t0.666667\t12\t6\t167"
    assert lines[2] == "b1\tm\t0\t0\t0\t0\tnan\t7\t0\t0"                # no methylated call at all: nan, not a division by zero
    assert lines[3] == "b2\ta\t1\t3\t1\t2\t0.333333\t0\t0\t3"
    full = format_sets(sets[:1], [np.array([[4, 4, 0, 0, 0, 3, 3, 0, 0, 0]])]).split("\n")[1]
    assert full.split("\t")[6] == "1.000000"


def test_contig_table_formatter():
    from nanomotif_amd.motif_coverage import CONTIGS_HEADER, format_contigs
    sets, names, tables = _tables()
    lines = format_contigs(sets, names, tables).split("\n")
    assert lines[0].split("\t") == CONTIGS_HEADER == ["bin", "contig", "mod_type", "n_mod_fwd", "n_mod_explained_fwd", "n_nomod_fwd", "n_nomod_covered_fwd",
                                                      "n_nocall_covered_fwd", "n_mod_rev", "n_mod_explained_rev", "n_nomod_rev", "n_nomod_covered_rev",
                                                      "n_nocall_covered_rev"]
    assert lines[1:] == ["b1\tc1\ta\t10\t7\t4\t1\t100\t5\t3\t2\t0\t50", "b1\tc2\ta\t1\t0\t0\t0\t9\t2\t2\t6\t5\t8",
                         "b1\tc1\tm\t0\t0\t3\t0\t0\t0\t0\t4\t0\t0", "b1\tc2\tm\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0",
                         "b2\tc3\ta\t3\t1\t0\t0\t2\t0\t0\t0\t0\t1", ""]


def test_motif_table_formatter():
    from nanomotif_amd.motif_coverage import MOTIFS_HEADER, format_motifs
    sets, _, _ = _tables()
    six = lambda *rows: np.array(rows, dtype=np.int64)
    site_counts = [[six([6, 1, 50, 3, 0, 20], [0, 0, 4, 2, 5, 3]), six([2, 0, 9, 1, 0, 4], [0, 0, 1, 1, 2, 0])], [], [six([1, 0, 2, 0, 0, 1])]]
    exclusive = [[six([4, 1, 2, 0], [0, 0, 1, 3]), six([0, 0, 0, 0], [0, 0, 0, 0])], [], [six([1, 0, 0, 0])]]
    lines = format_motifs(sets, site_counts, exclusive).split("\n")
    assert lines[0].split("\t") == MOTIFS_HEADER == ["bin", "motif", "mod_type", "mod_position", "n_mod", "n_nomod", "n_mod_exclusive", "n_nomod_exclusive"]
    assert lines[1:] == ["b1\tGATC\ta\t1\t11\t6\t7\t4",                 # n_mod = 6 + 3 + 0 + 2, n_nomod = 1 + 0 + 0 + 5; exclusive 4 + 2 + 0 + 1 and 1 + 0 + 0 + 3
                         "b1\tRGATCY\ta\t2\t4\t2\t0\t0",                # nested in GATC: counts of its own, nothing only it explains
                         "b2\tGCACNNNNNNGTT\ta\t2\t1\t0\t1\t0", ""]


def test_unexplained_formatter():
    from nanomotif_amd.engine import UNEXPLAINED_DTYPE
    from nanomotif_amd.motif_coverage import format_unexplained
    sets, _, _ = _tables()
    rec = np.zeros(3, dtype=UNEXPLAINED_DTYPE)
    rec["set"], rec["contig"], rec["pos"], rec["code"] = [0, 0, 2], [1, 1, 0], [7, 7, 4_000_000_000], [0, 4, 4]
    assert format_unexplained(rec, sets, ["c3", "c1"]) == "c1\t7\t8\ta\t0\t+\tb1\nc1\t7\t8\ta\t0\t-\tb1\nc3\t4000000000\t4000000001\ta\t0\t-\tb2\n"
    assert format_unexplained(rec[:0], sets, ["c3", "c1"]) == ""


def test_the_two_exports_are_declared_and_listed():
    from nanomotif_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("nm_motif_coverage_count", "nm_motif_coverage_sites"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS
    assert "find_motifs_bin.py:801-823" in text
    assert any(os.path.basename(s) == "nmcoverage.hip" for s in build.SRC_HIP)
    lib = _lib.load()
    # argument checks come before any device call
    assert lib.nm_motif_coverage_count(None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.nm_motif_coverage_sites(None, 1, None, None, None, None, None, None, None, 0, 0, None, None, None, None, None) == -1
