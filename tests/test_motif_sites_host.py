"""Host side of ``nanomotif motif_sites`` (no GPU): the sub-command's arguments, the native text writer of motif-sites.bed
(nm_motif_sites_text) against Python string formatting, and the candidate list read from a bin-motifs.tsv."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ("mod", "nomod", "nocall")


def test_parser_accepts_motif_sites_and_rejects_unknown_states(capsys):
    p = create_parser()
    a = p.parse_args(["motif_sites", "asm.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "sites"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.bin_motifs, a.out) == ("motif_sites", "asm.fasta", "pileup.bed", "contig_bin.tsv",
                                                                                      "out/bin-motifs.tsv", "sites")
    assert tuple(a.states) == STATES
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose) == (0.3, 0.7, 5, None, False)
    a = p.parse_args(["motif_sites", "asm.fasta", "pileup.bed.gz", "-d", "bins", "--bin_motifs", "b.tsv", "--states", "nocall,mod",
                      "--methylation_threshold_low", "0.2", "--methylation_threshold_high", "0.8", "--threshold_valid_coverage", "3",
                      "--device", "1", "-v"])
    assert tuple(a.states) == ("mod", "nocall") and a.directory == "bins"
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose) == (0.2, 0.8, 3, 1, True)
    a = p.parse_args(["motif_sites", "asm.fasta", "pileup.bed", "-f", "b1.fa", "b2.fa", "--bin_motifs", "b.tsv", "--states", "nomod"])
    assert tuple(a.states) == ("nomod",) and a.files == ["b1.fa", "b2.fa"]
    for bad in ("methylated", "mod,unknown", "", ","):
        with pytest.raises(SystemExit):
            p.parse_args(["motif_sites", "asm.fasta", "pileup.bed", "-c", "cb.tsv", "--bin_motifs", "b.tsv", "--states", bad])
        assert "--states" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                     # --bin_motifs and one of -c / -f / -d are required
        p.parse_args(["motif_sites", "asm.fasta", "pileup.bed", "-c", "cb.tsv"])
    with pytest.raises(SystemExit):
        p.parse_args(["motif_sites", "asm.fasta", "pileup.bed", "--bin_motifs", "b.tsv"])
    assert "motif_sites" in p.format_help()


def test_multi_rank_launch_is_refused(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), WORLD_SIZE="2", RANK="0", NANOMOTIF_NO_EARLY_INIT="1")
    r = subprocess.run([sys.executable, "-c", "from nanomotif_amd.main import main; main()", "motif_sites", "a.fasta", "p.bed", "-c", "cb.tsv",
                        "--bin_motifs", "b.tsv", "--out", "o"], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "one GPU" in r.stderr
    assert not os.path.exists(tmp_path / "o")


def _python_lines(contig, pos, code, seg_begin, names, bins, contig_names) -> bytes:
    lines = []
    for s in range(len(names)):
        for i in range(int(seg_begin[s]), int(seg_begin[s + 1])):
            lines.append("%s\t%d\t%d\t%s\t0\t%s\t%s\t%s\n" % (contig_names[contig[i]], int(pos[i]), int(pos[i]) + 1, names[s],
                                                               "-" if code[i] & 4 else "+", STATES[code[i] & 3], bins[s]))
    return "".join(lines).encode()


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
    code = rng.choice(np.array([0, 1, 2, 4, 5, 6], dtype=np.uint8), size=n)
    code[:6] = [6, 0, 1, 2, 4, 5][:len(code[:6])]
    return contig, pos, code, seg_begin, names, bins, contig_names


def test_native_writer_equals_python_formatting(monkeypatch):
    from nanomotif_amd.motif_sites import format_sites
    for n, seed in ((5000, 1), (4097, 2), (13, 3), (1, 4)):
        span = _random_span(n, seed)
        assert set(span[2].tolist()) == {0, 1, 2, 4, 5, 6} or n < 12
        assert int(span[1].max()) == 2 ** 32 - 2
        expect = _python_lines(*span)
        got = {}
        for threads in ("1", "16", "3"):
            monkeypatch.setenv("NM_POST_THREADS", threads)
            got[threads] = format_sites(*span)
        assert got["1"] == expect, n
        assert got["16"] == got["1"] and got["3"] == got["1"]
    monkeypatch.delenv("NM_POST_THREADS")
    assert format_sites(*_random_span(3000, 5)) == _python_lines(*_random_span(3000, 5))
    # an empty span writes nothing
    empty = np.zeros(0, np.uint32)
    assert format_sites(empty, empty, np.zeros(0, np.uint8), np.zeros(2, np.uint64), ["GATC_a_1"], ["b"], ["c"]) == b""


def test_native_writer_refuses_bad_records_and_short_buffers():
    import ctypes as C
    from nanomotif_amd import _lib
    from nanomotif_amd.motif_sites import format_sites
    contig, pos, code, seg_begin, names, bins, contig_names = _random_span(600, 7)
    bad = code.copy()
    bad[300] = 3                                                        # no such state
    with pytest.raises(_lib.NmScanError):
        format_sites(contig, pos, bad, seg_begin, names, bins, contig_names)
    far = contig.copy()
    far[599] = len(contig_names)
    with pytest.raises(_lib.NmScanError):
        format_sites(far, pos, code, seg_begin, names, bins, contig_names)
    short = seg_begin.copy()
    short[-1] = 599                                                     # the runs do not cover the span
    with pytest.raises(_lib.NmScanError):
        format_sites(contig, pos, code, short, names, bins, contig_names)
    lib = _lib.load()
    assert lib.nm_motif_sites_text(1, None, None, None, 0, None, None, None, 0, None, None, None, 0, None) == -1      # NM_EINVAL
    n = C.c_uint64(7)
    assert lib.nm_motif_sites_text(0, None, None, None, 0, None, None, None, 0, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    # a buffer one byte short is refused (NM_ERANGE), nothing is cut off
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    one = (np.zeros(1, np.uint32), np.array([41], np.uint32), np.array([5], np.uint8), np.array([0, 1], np.uint64))
    off = np.array([0, 4, 5], np.uint64)
    coff = np.array([0, 2], np.uint64)
    args = (1, p(one[0], C.c_uint32), p(one[1], C.c_uint32), p(one[2], C.c_uint8), 1, p(one[3], C.c_uint64), b"GATCb", p(off, C.c_uint64), 1, b"c1",
            p(coff, C.c_uint64))
    assert lib.nm_motif_sites_text(*args, None, 0, C.byref(n)) == 0
    line = b"c1\t41\t42\tGATC\t0\t-\tnomod\tb\n"
    assert n.value == len(line)
    buf = C.create_string_buffer(len(line))
    assert lib.nm_motif_sites_text(*args, buf, len(line) - 1, C.byref(n)) == -5
    assert lib.nm_motif_sites_text(*args, buf, len(line), C.byref(n)) == 0 and buf.raw == line


BIN_MOTIFS = """reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement
bin_a\tGATC\t1\ta\t910\t12\tpalindrome\t\t\t\t
bin_a\tGAAGY\t2\ta\t400\t9\tnon-palindrome\tRCTTC\t3\t395\t14
bin_a\tGCACNNNNNNGTT\t2\ta\t88\t1\tbipartite\tAACNNNNNNGTGC\t1\t85\t3
bin_b\tGATC\t1\ta\t700\t20\tpalindrome\t\t\t\t
bin_a\tGATC\t1\ta\t910\t12\tpalindrome\t\t\t\t
bin_b\tCCWGG\t1\tm\t300\t7\tpalindrome\t\t\t\t
bin_b\tRCTTC\t3\ta\t50\t2\tnon-palindrome\tGAAGY\t2\t51\t1
"""


def test_candidates_of_a_hand_written_bin_motifs(tmp_path):
    from nanomotif_amd.motif_sites import candidates_of_bin_motifs
    path = tmp_path / "bin-motifs.tsv"
    path.write_text(BIN_MOTIFS)
    cands = candidates_of_bin_motifs(str(path))
    assert [c.key for c in cands] == [
        ("bin_a", "GATC", "a", 1),                                     # palindrome: no complement column, one candidate
        ("bin_a", "GAAGY", "a", 2), ("bin_a", "RCTTC", "a", 3),        # a motif and its complement
        ("bin_a", "GCACNNNNNNGTT", "a", 2), ("bin_a", "AACNNNNNNGTGC", "a", 1),      # bipartite
        ("bin_b", "GATC", "a", 1),                                     # the same motif in a second bin; the repeated bin_a row is dropped
        ("bin_b", "CCWGG", "m", 1),
        ("bin_b", "RCTTC", "a", 3), ("bin_b", "GAAGY", "a", 2)]
    assert [c.name for c in cands[:5]] == ["GATC_a_1", "GAAGY_a_2", "RCTTC_a_3", "GCACNNNNNNGTT_a_2", "AACNNNNNNGTGC_a_1"]
    m, mod_type, b = cands[1].engine_candidate()
    assert (m.string, m.mod_position, mod_type, b) == ("GAAG[CT]", 2, "a", "bin_a")
    m, _, _ = cands[3].engine_candidate()
    assert (m.string, m.mod_position) == ("GCAC......GTT", 2)
    # the name is binnary's motif_mod spelling
    from nanomotif_amd.binnary import motif_mods_of_bin_motifs
    assert set(motif_mods_of_bin_motifs(str(path))) == {"GATC_a_1", "GAAGY_a_2", "GCACNNNNNNGTT_a_2", "CCWGG_m_1", "RCTTC_a_3"} <= {c.name for c in cands}
    # a table without the columns is refused
    other = tmp_path / "other.tsv"
    other.write_text("contig\tbin\nc1\tb\n")
    with pytest.raises(ValueError):
        candidates_of_bin_motifs(str(other))


def test_states_of_the_python_interface():
    from nanomotif_amd.engine import site_state_set
    from nanomotif_amd.motif_sites import parse_states
    assert parse_states("nocall, mod") == ("mod", "nocall") and parse_states("mod,nomod,nocall") == STATES
    with pytest.raises(ValueError):
        parse_states("mod,methylated")
    assert site_state_set(STATES) == 7 and site_state_set(("nomod",)) == 2 and site_state_set(["nocall", "mod"]) == 5
    for bad in ((), ("x",), ("mod", "x")):
        with pytest.raises(ValueError):
            site_state_set(bad)
