"""Host side of ``nanomotif motif_compare`` (no GPU): the sub-command's arguments, the formatters of its three tables on hand-made
tables, the exact McNemar test on hand values, the native text writer of switched-sites.bed (nm_motif_compare_text) against Python
string formatting, and the exports in the header and the binding."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ("mod", "nomod", "nocall")
TRANSITIONS = tuple(f"{a}>{b}" for a in STATES for b in STATES)


# ------------------------------------------------------------------------------------------------ the parser
def test_parser_accepts_motif_compare(capsys):
    p = create_parser()
    a = p.parse_args(["motif_compare", "asm.fasta", "a.bed", "b.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out_a/bin-motifs.tsv",
                      "out_b/bin-motifs.tsv", "--out", "cmp"])
    assert (a.command, a.assembly, a.pileup_a, a.pileup_b, a.contig_bin, a.out) == ("motif_compare", "asm.fasta", "a.bed", "b.bed", "contig_bin.tsv", "cmp")
    assert a.bin_motifs == ["out_a/bin-motifs.tsv", "out_b/bin-motifs.tsv"]
    assert tuple(a.transitions) == ("mod>nomod", "nomod>mod") and a.switched_sites is False
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose, a.threads) == (0.3, 0.7, 5, None, False, 1)
    a = p.parse_args(["motif_compare", "asm.fasta", "a.bed.gz", "b.bed.gz", "-d", "bins", "--bin_motifs", "b.tsv", "--switched_sites",
                      "--transitions", "nocall>mod, mod>mod,mod>nocall", "--methylation_threshold_low", "0.2", "--methylation_threshold_high", "0.8",
                      "--threshold_valid_coverage", "3", "--device", "1", "-v", "-t", "4"])
    assert tuple(a.transitions) == ("mod>mod", "mod>nocall", "nocall>mod") and a.switched_sites and a.directory == "bins" and a.bin_motifs == ["b.tsv"]
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose, a.threads) == (0.2, 0.8, 3, 1, True, 4)
    a = p.parse_args(["motif_compare", "asm.fasta", "a.bed", "b.bed", "-f", "b1.fa", "b2.fa", "--bin_motifs", "b.tsv", "--transitions",
                      ",".join(TRANSITIONS)])
    assert tuple(a.transitions) == TRANSITIONS and a.files == ["b1.fa", "b2.fa"]
    for bad in ("switched", "mod>nomod,mod>unknown", "mod", "mod<nomod", "", ","):
        with pytest.raises(SystemExit):
            p.parse_args(["motif_compare", "asm.fasta", "a.bed", "b.bed", "-c", "cb.tsv", "--bin_motifs", "b.tsv", "--transitions", bad])
        assert "--transitions" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                     # --bin_motifs, one of -c / -f / -d and BOTH pileups are required
        p.parse_args(["motif_compare", "asm.fasta", "a.bed", "b.bed", "-c", "cb.tsv"])
    with pytest.raises(SystemExit):
        p.parse_args(["motif_compare", "asm.fasta", "a.bed", "b.bed", "--bin_motifs", "b.tsv"])
    with pytest.raises(SystemExit):
        p.parse_args(["motif_compare", "asm.fasta", "a.bed", "-c", "cb.tsv", "--bin_motifs", "b.tsv"])
    capsys.readouterr()
    assert "motif_compare" in p.format_help()


def test_parse_transitions():
    from nanomotif_amd.engine import transition_set
    from nanomotif_amd.motif_compare import parse_transitions
    assert parse_transitions("nomod>mod,mod>nomod") == ("mod>nomod", "nomod>mod")
    assert parse_transitions(" nocall>nocall ,mod>mod,mod>mod") == ("mod>mod", "nocall>nocall")
    for bad in ("", "mod", "on>off", "mod>nomod;nomod>mod"):
        with pytest.raises(ValueError):
            parse_transitions(bad)
    assert transition_set(("mod>nomod", "nomod>mod")) == (1 << 1) | (1 << 3)
    assert transition_set(TRANSITIONS) == 0x1FF and [transition_set((t,)) for t in TRANSITIONS] == [1 << i for i in range(9)]
    for bad in ((), ("mod",), ("mod>nomod", "x>y")):
        with pytest.raises(ValueError):
            transition_set(bad)


def test_multi_rank_launch_is_refused(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), WORLD_SIZE="2", RANK="0", NANOMOTIF_NO_EARLY_INIT="1")
    r = subprocess.run([sys.executable, "-c", "from nanomotif_amd.main import main; main()", "motif_compare", "a.fasta", "a.bed", "b.bed", "-c", "cb.tsv",
                        "--bin_motifs", "b.tsv", "--out", "o"], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "one GPU" in r.stderr
    assert not os.path.exists(tmp_path / "o")


# ------------------------------------------------------------------------------------------------ the test
def _exact_p(g, l):
    """min(1, 2 P[X <= min(g, l)]) from integer binomials."""
    n, k = g + l, min(g, l)
    return min(1.0, 2 * sum(math.comb(n, i) for i in range(k + 1)) / 2 ** n)


def test_mcnemar_p_hand_values():
    from nanomotif_amd.motif_compare import mcnemar_p
    assert math.isnan(mcnemar_p(0, 0))
    assert mcnemar_p(5, 0) == pytest.approx(2 * math.comb(5, 0) / 2 ** 5, rel=1e-12) and _exact_p(5, 0) == 0.0625
    assert mcnemar_p(3, 3) == 1.0 and _exact_p(3, 3) == 1.0
    assert mcnemar_p(1, 9) == pytest.approx(2 * (math.comb(10, 0) + math.comb(10, 1)) / 2 ** 10, rel=1e-12) and _exact_p(1, 9) == 22 / 1024
    assert mcnemar_p(9, 1) == mcnemar_p(1, 9)
    for g, l in ((0, 1), (1, 0), (2, 1), (7, 8), (8, 7), (40, 2), (100, 60), (0, 900), (1200, 1000), (5000, 4700)):
        assert mcnemar_p(g, l) == pytest.approx(_exact_p(g, l), rel=1e-9), (g, l)
    # a large case: finite, in (0, 1], symmetric, and what the normal approximation with continuity correction says to two digits
    g, l = 501_500, 498_500
    p = mcnemar_p(g, l)
    assert math.isfinite(p) and 0.0 < p <= 1.0 and p == mcnemar_p(l, g)
    z = (abs(g - l) - 1) / math.sqrt(g + l)
    assert p == pytest.approx(math.erfc(z / math.sqrt(2)), rel=2e-2)
    assert mcnemar_p(3_000_000, 3_000_000) == 1.0
    assert mcnemar_p(2_000_000, 0) == 0.0 or mcnemar_p(2_000_000, 0) > 0.0      # underflows to zero, does not raise


# ------------------------------------------------------------------------------------------------ the formatters
def _cand(bin, motif, mod_type, pos):
    from nanomotif_amd.motif_sites import SiteCandidate
    return SiteCandidate(bin, motif, mod_type, pos)


def _expect_derived(n):
    mod_a, nomod_a, mod_b, nomod_b = n[0] + n[1] + n[2], n[3] + n[4] + n[5], n[0] + n[3] + n[6], n[1] + n[4] + n[7]
    both = n[0] + n[1] + n[3] + n[4]
    deg = ["%.6f" % ((n[0] + n[1]) / both), "%.6f" % ((n[0] + n[3]) / both), "%.6f" % ((n[3] - n[1]) / both)] if both else ["nan"] * 3
    g, l = n[3], n[1]
    p = "nan" if g + l == 0 else "%.6g" % _exact_p(g, l)
    return [str(mod_a), str(nomod_a), str(mod_b), str(nomod_b)] + deg + [p]


def test_formatters_on_hand_made_tables():
    from nanomotif_amd.motif_compare import BINS_HEADER, CONTIGS_HEADER, MAIN_HEADER, format_bins, format_contigs, format_main
    assert MAIN_HEADER == ["bin", "motif", "mod_type", "mod_position", "n_mod_mod", "n_mod_nomod", "n_mod_nocall", "n_nomod_mod", "n_nomod_nomod",
                           "n_nomod_nocall", "n_nocall_mod", "n_nocall_nomod", "n_nocall_nocall", "n_mod_a", "n_nomod_a", "n_mod_b", "n_nomod_b",
                           "degree_a", "degree_b", "degree_delta", "mcnemar_p"]
    assert BINS_HEADER == ["bin", "mod_type"] + MAIN_HEADER[4:]
    assert CONTIGS_HEADER[:5] == ["bin", "contig", "motif", "mod_type", "mod_position"] and len(CONTIGS_HEADER) == 23
    assert CONTIGS_HEADER[5] == "n_mod_mod_fwd" and CONTIGS_HEADER[13] == "n_nocall_nocall_fwd" and CONTIGS_HEADER[14] == "n_mod_mod_rev" and CONTIGS_HEADER[22] == "n_nocall_nocall_rev"
    cands = [_cand("b1", "GATC", "a", 1), _cand("b1", "CCWGG", "m", 1), _cand("b2", "GATC", "a", 1)]
    t0 = np.array([[10, 1, 2, 9, 20, 3, 4, 5, 6, 1, 0, 0, 0, 1, 0, 0, 0, 7], [0, 4, 0, 0, 0, 0, 0, 0, 1, 5, 0, 1, 0, 0, 0, 1, 0, 0]], dtype=np.int64)
    t1 = np.array([[0, 0, 3, 0, 0, 0, 2, 0, 9, 0, 0, 1, 0, 0, 0, 0, 4, 0]], dtype=np.int64)          # nothing called in both
    t2 = np.zeros((0, 18), dtype=np.int64)                                                          # a bin without contigs
    nines = [[16, 5, 3, 9, 21, 3, 5, 5, 14], [0, 0, 4, 0, 0, 0, 2, 4, 9], [0] * 9]
    text = format_main(cands, [t0, t1, t2])
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == MAIN_HEADER and len(lines) == 5
    for c, nine, line in zip(cands, nines, lines[1:]):
        assert line.split("\t") == [c.bin, c.motif, c.mod_type, str(c.mod_position)] + [str(x) for x in nine] + _expect_derived(nine)
    assert lines[1].split("\t")[13:] == ["24", "33", "30", "31", "0.411765", "0.490196", "0.078431", "0.42395"]
    assert lines[2].split("\t")[13:] == ["4", "0", "2", "4", "nan", "nan", "nan", "nan"]
    text = format_contigs(cands, [["c1", "c2"], ["c1"], []], [t0, t1, t2])
    lines = text.split("\n")
    assert lines[0].split("\t") == CONTIGS_HEADER and len(lines) == 5
    assert lines[1].split("\t") == ["b1", "c1", "GATC", "a", "1"] + [str(x) for x in t0[0]]
    assert lines[2].split("\t") == ["b1", "c2", "GATC", "a", "1"] + [str(x) for x in t0[1]]
    assert lines[3].split("\t") == ["b1", "c1", "CCWGG", "m", "1"] + [str(x) for x in t1[0]]
    text = format_bins([("b1", "a"), ("b1", "m")], [t0, t1])
    lines = text.split("\n")
    assert lines[0].split("\t") == BINS_HEADER and len(lines) == 4
    assert lines[1].split("\t") == ["b1", "a"] + [str(x) for x in nines[0]] + _expect_derived(nines[0])
    assert lines[2].split("\t") == ["b1", "m"] + [str(x) for x in nines[1]] + _expect_derived(nines[1])


def test_candidates_of_several_files(tmp_path):
    from nanomotif_amd.motif_compare import candidates_of_files
    head = "reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement\n"
    (tmp_path / "a.tsv").write_text(head + "bin_a\tGATC\t1\ta\t910\t12\tpalindrome\t\t\t\t\nbin_a\tGAAGY\t2\ta\t400\t9\tnon-palindrome\tRCTTC\t3\t395\t14\n")
    (tmp_path / "b.tsv").write_text(head + "bin_a\tRCTTC\t3\ta\t1\t1\tnon-palindrome\tGAAGY\t2\t1\t1\nbin_b\tGATC\t1\ta\t5\t5\tpalindrome\t\t\t\t\n"
                                    "bin_a\tCCWGG\t1\tm\t7\t7\tpalindrome\t\t\t\t\n")
    got = [c.key for c in candidates_of_files([str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")])]
    assert got == [("bin_a", "GATC", "a", 1), ("bin_a", "GAAGY", "a", 2), ("bin_a", "RCTTC", "a", 3), ("bin_b", "GATC", "a", 1), ("bin_a", "CCWGG", "m", 1)]
    assert [c.key for c in candidates_of_files([str(tmp_path / "b.tsv")])][:2] == [("bin_a", "RCTTC", "a", 3), ("bin_a", "GAAGY", "a", 2)]


# ------------------------------------------------------------------------------------------------ the native text writer
def _python_lines(contig, pos, code, seg_begin, names, bins, contig_names) -> bytes:
    lines = []
    for s in range(len(names)):
        for i in range(int(seg_begin[s]), int(seg_begin[s + 1])):
            t = code[i] & 15
            lines.append("%s\t%d\t%d\t%s\t0\t%s\t%s>%s\t%s\n" % (contig_names[contig[i]], int(pos[i]), int(pos[i]) + 1, names[s],
                                                                  "-" if code[i] & 16 else "+", STATES[t // 3], STATES[t % 3], bins[s]))
    return "".join(lines).encode()


ALL_CODES = list(range(9)) + [16 + t for t in range(9)]


def _random_span(n, seed):
    rng = np.random.default_rng(seed)
    contig_names = ["contig_1", "c", "NODE_17_length_123456_cov_7.5", "x" * 40, "k141_9"]
    names = ["GATC_a_1", "CCWGG_m_1", "GCACNNNNNNGTT_a_2", "A_a_0", "RGATCY_a_2", "TTAA_21839_3", "G_m_0"]
    bins = ["bin.1", "bin.1", "b2", "a_rather_long_bin_name.fa", "b2", "bin.1", "z"]
    cuts = np.sort(rng.integers(0, n + 1, size=len(names) - 1))
    cuts[2] = cuts[1]                                                   # an empty run in the middle
    seg_begin = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    contig = rng.integers(0, len(contig_names), size=n).astype(np.uint32)
    pos = rng.integers(0, 2 ** 32 - 1, size=n, dtype=np.uint64).astype(np.uint32)
    edge = [2 ** 32 - 2, 0, 1, 9, 10, 99, 100, 999_999_999, 1_000_000_000, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3]
    pos[:12] = edge[:len(pos[:12])]
    code = rng.choice(np.array(ALL_CODES, dtype=np.uint8), size=n)
    code[:18] = ALL_CODES[:len(code[:18])]
    return contig, pos, code, seg_begin, names, bins, contig_names


def _format(*span):
    from nanomotif_amd.motif_sites import format_sites
    return format_sites(*span, symbol="nm_motif_compare_text")


def test_native_writer_equals_python_formatting(monkeypatch):
    for n, seed in ((5000, 1), (4097, 2), (18, 3), (1, 4)):
        span = _random_span(n, seed)
        assert set(span[2].tolist()) == set(ALL_CODES) or n < 18
        assert len(set(np.searchsorted(span[3], np.arange(n), side="right").tolist())) > 1 or n == 1      # several candidates / bins
        expect = _python_lines(*span)
        got = {}
        for threads in ("1", "8", "3"):
            monkeypatch.setenv("NM_POST_THREADS", threads)
            got[threads] = _format(*span)
        assert got["1"] == expect, n
        assert got["8"] == got["1"] and got["3"] == got["1"]
    monkeypatch.delenv("NM_POST_THREADS")
    assert _format(*_random_span(3000, 5)) == _python_lines(*_random_span(3000, 5))
    empty = np.zeros(0, np.uint32)
    assert _format(empty, empty, np.zeros(0, np.uint8), np.zeros(2, np.uint64), ["GATC_a_1"], ["b"], ["c"]) == b""


def test_native_writer_refuses_bad_records_and_short_buffers():
    from nanomotif_amd import _lib
    contig, pos, code, seg_begin, names, bins, contig_names = _random_span(600, 7)
    for wrong in (9, 15, 16 + 9, 32, 64 + 1):                              # no such transition / bits beyond the strand bit
        bad = code.copy()
        bad[300] = wrong
        with pytest.raises(_lib.NmScanError) as e:
            _format(contig, pos, bad, seg_begin, names, bins, contig_names)
        assert e.value.code == -1
    far = contig.copy()
    far[599] = len(contig_names)
    with pytest.raises(_lib.NmScanError):
        _format(far, pos, code, seg_begin, names, bins, contig_names)
    short = seg_begin.copy()
    short[-1] = 599                                                     # the runs do not cover the span
    with pytest.raises(_lib.NmScanError):
        _format(contig, pos, code, short, names, bins, contig_names)
    lib = _lib.load()
    assert lib.nm_motif_compare_text(1, None, None, None, 0, None, None, None, 0, None, None, None, 0, None) == -1      # NM_EINVAL
    n = C.c_uint64(7)
    assert lib.nm_motif_compare_text(0, None, None, None, 0, None, None, None, 0, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    # the size query, and a buffer one byte short is refused (NM_ERANGE): nothing is cut off
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    one = (np.zeros(1, np.uint32), np.array([41], np.uint32), np.array([16 + 5], np.uint8), np.array([0, 1], np.uint64))
    off = np.array([0, 4, 5], np.uint64)
    coff = np.array([0, 2], np.uint64)
    args = (1, p(one[0], C.c_uint32), p(one[1], C.c_uint32), p(one[2], C.c_uint8), 1, p(one[3], C.c_uint64), b"GATCb", p(off, C.c_uint64), 1, b"c1",
            p(coff, C.c_uint64))
    assert lib.nm_motif_compare_text(*args, None, 0, C.byref(n)) == 0
    line = b"c1\t41\t42\tGATC\t0\t-\tnomod>nocall\tb\n"
    assert n.value == len(line)
    buf = C.create_string_buffer(len(line))
    assert lib.nm_motif_compare_text(*args, buf, len(line) - 1, C.byref(n)) == -5
    assert lib.nm_motif_compare_text(*args, buf, len(line), C.byref(n)) == 0 and buf.raw == line
    # the neighbour's writer still refuses what it refused: a state 3 and the bit 8
    assert lib.nm_motif_sites_text(*args, None, 0, C.byref(n)) == -1


# ------------------------------------------------------------------------------------------------ exports
def test_exports_are_declared_bound_and_built():
    from nanomotif_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    for name in ("nm_motif_compare_count", "nm_motif_compare_sites", "nm_motif_compare_text"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS
    assert "#define NM_COMPARE_MINUS 16u" in header
    assert any(os.path.basename(s) == "nmcompare.hip" for s in build.SRC_HIP)
    lib = _lib.load()
    assert lib.nm_abi_version() == 1
    # NULL arguments are refused before anything touches a device
    assert lib.nm_motif_compare_count(None, 1, None, None, None, None, None, None, None, 0x1FF, None, None, None) == -1
    assert lib.nm_motif_compare_sites(None, 1, None, None, None, None, None, None, None, 0x1FF, 0, 0, None, None, None, None, None) == -1
