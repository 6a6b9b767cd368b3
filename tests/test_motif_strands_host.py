"""Host side of ``nanomotif motif_strands`` (no GPU): the brute force both suites compare against (built only from
``oracle.scan.subseq_indices``, ``oracle.scan.split_positions`` and ``oracle.motif.Motif``) and the conditions on the geometry input it is
run on, ``pair_set`` / ``--pairs``, the partner rule on a hand-written bin-motifs.tsv, the partner offset under stripping, the derived
columns against integer arithmetic, the native text writer of hemi-sites.bed (nm_motif_strands_text), and the exports in the header and
the binding."""
import ctypes as C
import functools
import logging
import os

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser
from test_gpu_motif_compare import exact_p, oracle_calls, reach_class, state_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ("mod", "nomod", "nocall")
PAIRS = tuple(f"{a}-{b}" for a in STATES for b in STATES)
HEMI = ("mod-nomod", "nomod-mod")
CHUNK = 8192


# ------------------------------------------------------------------------------------------------ the brute force
def offset_of(motif, i, j):
    """d = L - 1 - i - j, L = tokens of the unstripped motif."""
    from oracle.motif import Motif as OMotif
    return len(OMotif(motif, i).split()) - 1 - i - j


def oracle_pairs(seq, motif, i, j):
    """[(own position, occurrence strand, partner position)] of one candidate on one contig in contract order: the stripped motif on '+'
    (strand 0, partner on '-' at p + d), its reverse complement on '-' (strand 1, partner on '+' at p - d)."""
    from oracle.motif import Motif as OMotif
    from oracle.scan import subseq_indices
    d = offset_of(motif, i, j)
    st = OMotif(motif, i).new_stripped_motif()
    rc = st.reverse_compliment()
    out = [(int(p), 0, int(p) + d) for p in subseq_indices(st.string, seq) + st.mod_position]
    out += [(int(p), 1, int(p) - d) for p in subseq_indices(rc.string, seq) + rc.mod_position]
    return sorted(out)                                                  # ascending position, '+' before '-'


class Expected:
    """What the contract says about ``cands`` = [(bin, mod type, motif string, mod position, partner position), ...]: per candidate the
    int64[n, 18] table and all records (candidate, contig id, own position, code, partner position) in contract order.  ``piles``: mod
    type -> {contig name -> ContigPileup}."""

    def __init__(self, cands, bin_contigs, contig_index, seqs, piles, low=0.3, high=0.7):
        from oracle.scan import _EMPTY
        calls = {}

        def calls_of(mt, name):
            if (mt, name) not in calls:
                calls[(mt, name)] = oracle_calls(piles[mt].get(name, _EMPTY), low, high)
            return calls[(mt, name)]
        self.tables, self.records = [], []
        for k, (b, mt, motif, i, j) in enumerate(cands):
            names = bin_contigs[b]
            table = np.zeros((len(names), 18), dtype=np.int64)
            for r, name in enumerate(names):
                c = calls_of(mt, name)
                for p, strand, q in oracle_pairs(seqs[name], motif, i, j):
                    assert 0 <= q < len(seqs[name])                     # the partner lies inside the occurrence, hence inside the contig
                    t = 3 * state_of((p, strand), c) + state_of((q, 1 - strand), c)
                    table[r, 9 * strand + t] += 1
                    self.records.append((k, contig_index[name], p, 16 * strand + t, q))
            self.tables.append(table)

    def selected(self, pairs):
        want = {PAIRS.index(t) for t in pairs}
        return [r[:4] for r in self.records if (r[3] & 15) in want]


# ------------------------------------------------------------------------------------------------ the geometry input (shared with the GPU suite)
GEOMETRY_SEED = 20
# (motif, mod position i, partner position j in the reverse complement): d = L - 1 - i - j
GEOMETRY_MOTIFS = [("GATC", 1, 1), ("GATC", 1, 2), ("A", 0, 0), ("AATT", 1, 0), ("AATT", 0, 0), ("AATT", 3, 3), ("G[AG]TC", 1, 1), ("..GATC.", 3, 2),
                   ("A" + "." * 30 + "T", 0, 0), ("A" + "." * 31 + "T", 0, 0), ("A" + "." * 32 + "T", 0, 0), ("A" + "." * 40 + "T", 0, 0),
                   ("A" + "." * 62 + "T", 0, 0), ("A" + "." * 63 + "T", 0, 0), ("A" + "." * 70 + "T", 0, 0), ("A" + "." * 94 + "T", 0, 1),
                   ("G" + "." * 50 + "A", 51, 3), ("A" + "." * 70 + "T", 71, 71), ("A" + "." * 94 + "T", 95, 95), ("A" + "." * 40 + "C", 0, 20)]
GEOMETRY_OFFSETS = [1, 0, 0, 2, 3, -3, 1, 1, 31, 32, 33, 41, 63, 64, 71, 94, -3, -71, -95, 21]


@functools.lru_cache(maxsize=None)
def geometry_input():
    """(names, seqs, bins, bin_names, rows, piles): a 30 kbp contig of four chunks with planted occurrences astride the 8 192 border, a
    128-position lane border and a 32-bit word border and an N run across a chunk border; a 9 kbp contig that ends in the motif; an 8 kbp
    one that starts and ends in it; 320 bp of back-to-back sites; contigs shorter than the motif; a second bin and an empty one.  Every
    (position, strand) has a row independently with probability 0.6, fractions from {0, 0.3, 0.5, 0.7, 1.0}.  ``rows``: the flat upload
    (contig id, position, strand byte, fraction); ``piles``: {"a": {name: ContigPileup}}."""
    from oracle.scan import ContigPileup
    rng = np.random.default_rng(GEOMETRY_SEED)
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    big = list(rand(30_000))
    big[8190:8194] = "GATC"                                             # astride the chunk border: own base 8191, partner 8192
    big[16380:16390] = "TAATTAATTC"                                     # AATT at 16381 .. 16384 astride the next one
    big[9630:9634] = "GATC"                                             # own base at bit 31 of a word, partner in the next word
    big[10238:10242] = "GATC"                                           # own base in the last position of a lane's 128, partner in the next lane
    big[24566:24570] = "GATC"
    big[24570:24585] = "N" * 15                                         # an N run across a chunk border
    big[24585:24589] = "GATC"
    seqs = {"big": "".join(big), "tiny1": "G", "tiny2": "GA", "tiny3": "ATC", "small": "GATC" * 50 + "AATT" * 30,
            "edge": "GATC" + rand(CHUNK - 8) + "GATC", "mid": rand(9_000 - 4) + "GATC"}
    bins = {n: ("b2" if n == "mid" else "b1") for n in seqs}
    names = list(seqs)
    cid, pos, st, fr, piles = [], [], [], [], {}
    for c, n in enumerate(names):
        L = len(seqs[n])
        p, s = np.nonzero(rng.random((L, 2)) < 0.6)                     # ascending position, '+' before '-'
        strand = np.where(s == 0, ord("+"), ord("-")).astype(np.uint8)
        f = rng.choice([0.0, 0.3, 0.5, 0.7, 1.0], size=len(p))
        piles[n] = ContigPileup(p.astype(np.int64), strand, f)
        cid.append(np.full(len(p), c, np.uint32)); pos.append(p); st.append(strand); fr.append(f)
    rows = (np.concatenate(cid), np.concatenate(pos), np.concatenate(st), np.concatenate(fr))
    return names, seqs, bins, ["b0_empty", "b1", "b2"], rows, {"a": piles}


def geometry_cands():
    return [(b, "a", m, i, j) for b in ("b1", "b2") for m, i, j in GEOMETRY_MOTIFS]


@functools.lru_cache(maxsize=None)
def geometry_expected():
    names, seqs, bins, _, _, piles = geometry_input()
    bin_contigs = {b: [n for n in names if bins[n] == b] for b in ("b1", "b2")}
    return Expected(geometry_cands(), bin_contigs, {n: i for i, n in enumerate(names)}, seqs, piles)


def test_the_input_is_not_degenerate():
    """The brute force alone fills all 18 columns with more than 1 500 sites each; the offsets are the ones the shift can go wrong at, at
    all three widths, some with i != j; own base and partner fall into different chunks, lanes and words."""
    names, seqs, bins, _, _, _ = geometry_input()
    assert sorted(len(s) for s in seqs.values())[-4:] == [320, CHUNK, 9_000, 30_000]
    cands = geometry_cands()
    assert [offset_of(m, i, j) for m, i, j in GEOMETRY_MOTIFS] == GEOMETRY_OFFSETS
    assert {0, 1, 2, 3, -3, 31, 32, 33, 41, 63, 64, 71, 94} <= set(GEOMETRY_OFFSETS)
    assert {reach_class(m, i) for m, i, _ in GEOMETRY_MOTIFS} == {0, 1, 2} and any(i != j for _, i, j in GEOMETRY_MOTIFS)
    exp = geometry_expected()
    table = np.concatenate(exp.tables).sum(axis=0)
    print("columns", table.tolist())
    assert (table > 1500).all(), table.tolist()
    for t in PAIRS:
        assert len(exp.selected((t,))) > 0
    big = names.index("big")
    for k, (b, _, m, i, j) in enumerate(cands):
        if b != "b1" or offset_of(m, i, j) == 0:
            continue
        on_big = [(r[2], r[4]) for r in exp.records if r[0] == k and r[1] == big]
        for unit in (CHUNK, 128, 32):
            assert any(p // unit != q // unit for p, q in on_big), (m, i, j, unit)
    gatc = cands.index(("b1", "a", "GATC", 1, 1))
    own = {(r[2], r[3] >> 4, r[4]) for r in exp.records if r[0] == gatc and r[1] == big}
    assert {(8191, 0, 8192), (8192, 1, 8191), (9631, 0, 9632), (10239, 0, 10240), (24567, 0, 24568), (24586, 0, 24587)} <= own
    assert not any(24570 <= p < 24585 for p, _, _ in own)
    aatt = cands.index(("b1", "a", "AATT", 0, 0))
    assert (16381, 0, 16384) in {(r[2], r[3] >> 4, r[4]) for r in exp.records if r[0] == aatt and r[1] == big}
    mid = names.index("mid")                                            # the contig that ends in the motif: '-' own base on its second to last position
    k = cands.index(("b2", "a", "GATC", 1, 1))
    assert (9_000 - 2, 1, 9_000 - 3) in {(r[2], r[3] >> 4, r[4]) for r in exp.records if r[0] == k and r[1] == mid}


def test_identities_hold_in_the_brute_force():
    """(b) the '-' nine of (M, i | j) is the transposed '+' nine of (revcomp M, j | i); (c) for a palindrome with j = i the '-' nine is the
    transpose of the '+' nine."""
    from oracle.motif import Motif as OMotif
    names, seqs, bins, _, _, piles = geometry_input()
    bin_contigs = {"b1": [n for n in names if bins[n] == "b1"]}
    index = {n: i for i, n in enumerate(names)}
    exp = geometry_expected()
    cands = geometry_cands()
    for m, i, j in (("GATC", 1, 1), ("AATT", 1, 0), ("G[AG]TC", 1, 1), ("A" + "." * 40 + "C", 0, 20), ("G" + "." * 50 + "A", 51, 3)):
        t = exp.tables[cands.index(("b1", "a", m, i, j))]
        rc = OMotif(m, i).reverse_compliment()
        u = Expected([("b1", "a", rc.string, j, i)], bin_contigs, index, seqs, piles).tables[0]
        assert np.array_equal(t[:, 9:].reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9), u[:, :9]), (m, i, j)
        assert np.array_equal(t[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9), u[:, 9:]), (m, i, j)
    for m, i in (("GATC", 1), ("AATT", 0), ("AATT", 3)):
        t = exp.tables[cands.index(("b1", "a", m, i, i))]
        assert t.sum() > 0 and np.array_equal(t[:, 9:].reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9), t[:, :9]), (m, i)


# ------------------------------------------------------------------------------------------------ pairs, the parser
def test_pair_set_and_parse_pairs():
    from nanomotif_amd import engine
    from nanomotif_amd.motif_strands import parse_pairs
    assert engine.PAIRS == PAIRS and engine.HEMI == HEMI and engine.STRANDS_MINUS == 16
    assert engine.pair_set(HEMI) == (1 << 1) | (1 << 3)
    assert engine.pair_set(PAIRS) == 0x1FF and [engine.pair_set((t,)) for t in PAIRS] == [1 << i for i in range(9)]
    assert engine.pair_set(("mod-mod", "mod-mod")) == 1
    for bad in ((), ("mod",), ("mod>nomod",), ("mod-nomod", "x-y")):
        with pytest.raises(ValueError):
            engine.pair_set(bad)
    assert parse_pairs("nomod-mod,mod-nomod") == HEMI
    assert parse_pairs(" nocall-nocall ,mod-mod,mod-mod") == ("mod-mod", "nocall-nocall")
    for bad in ("", "mod", "mod>nomod", "mod-nomod;nomod-mod", ","):
        with pytest.raises(ValueError):
            parse_pairs(bad)


def test_parser_accepts_motif_strands(capsys):
    p = create_parser()
    a = p.parse_args(["motif_strands", "asm.fasta", "p.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "st"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.out, a.bin_motifs) == ("motif_strands", "asm.fasta", "p.bed", "contig_bin.tsv", "st", ["out/bin-motifs.tsv"])
    assert tuple(a.pairs) == HEMI and a.hemi_sites is False
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose, a.threads) == (0.3, 0.7, 5, None, False, 1)
    a = p.parse_args(["motif_strands", "asm.fasta", "p.bed.gz", "-d", "bins", "--bin_motifs", "a.tsv", "b.tsv", "--hemi_sites", "--pairs",
                      "nocall-mod, mod-mod,mod-nocall", "--device", "1", "-v", "-t", "4"])
    assert tuple(a.pairs) == ("mod-mod", "mod-nocall", "nocall-mod") and a.hemi_sites and a.bin_motifs == ["a.tsv", "b.tsv"] and a.device == 1
    for bad in ("hemi", "mod-nomod,mod-unknown", "mod>nomod", "", ","):
        with pytest.raises(SystemExit):
            p.parse_args(["motif_strands", "asm.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "b.tsv", "--pairs", bad])
        assert "--pairs" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["motif_strands", "asm.fasta", "p.bed", "-c", "cb.tsv"])
    capsys.readouterr()
    assert "motif_strands" in p.format_help()


# ------------------------------------------------------------------------------------------------ the partner rule
HEAD = "reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement\n"


def test_partner_rule_on_a_hand_written_file(tmp_path, caplog):
    from nanomotif_amd.motif_sites import candidates_of_files
    from nanomotif_amd.motif_strands import complement_partners, strand_candidates
    (tmp_path / "a.tsv").write_text(HEAD + "bin_a\tGAAGY\t2\ta\t400\t9\tnon-palindrome\tRCTTC\t3\t395\t14\n"      # a complement row
                                    "bin_a\tGATC\t1\ta\t910\t12\tpalindrome\t\t\t\t\n"                            # a palindrome without one
                                    "bin_a\tATTG\t0\ta\t50\t5\tnon-palindrome\t\t\t\t\n"                          # revcomp CAAT: A at 1 and 2
                                    "bin_a\tGAAC\t1\ta\t50\t5\tnon-palindrome\t\t\t\t\n"                          # revcomp GTTC: no A
                                    "bin_b\tCCWGG\t1\tm\t70\t7\tpalindrome\t\t\t\t\n")                            # revcomp CCWGG: C at 0 and 1
    files = [str(tmp_path / "a.tsv")]
    with caplog.at_level(logging.WARNING):
        got = strand_candidates(candidates_of_files(files), complement_partners(files))
    assert [c.key for c in got] == [("bin_a", "GAAGY", "a", 2, 3), ("bin_a", "RCTTC", "a", 3, 2), ("bin_a", "GATC", "a", 1, 1), ("bin_a", "ATTG", "a", 0, 1),
                                    ("bin_a", "ATTG", "a", 0, 2), ("bin_b", "CCWGG", "m", 1, 0), ("bin_b", "CCWGG", "m", 1, 1)]
    assert "GAAC_a_1" in caplog.text and "skipped" in caplog.text
    # d = L - 1 - i - j: a motif and its complement see each other at the same offset; only (palindrome, j = i) counts each duplex site once
    assert [c.offset for c in got] == [-1, -1, 1, 2, 1, 3, 2]
    assert [c.palindrome for c in got] == [False, False, True, False, False, False, True]
    assert got[0].name == "GAAGY_a_2" and got[0].engine_candidate()[1:] == ("a", "bin_a", 3) and got[0].engine_candidate()[0].string == "GAAG[CT]"
    # a motif that is a complement in one file and a plain row in another keeps the complement's partner
    (tmp_path / "b.tsv").write_text(HEAD + "bin_a\tRCTTC\t3\ta\t1\t1\tnon-palindrome\t\t\t\t\n")
    files = [str(tmp_path / "b.tsv"), str(tmp_path / "a.tsv")]
    got = strand_candidates(candidates_of_files(files), complement_partners(files))
    assert [c.key for c in got][:2] == [("bin_a", "RCTTC", "a", 3, 2), ("bin_a", "GAAGY", "a", 2, 3)]


def test_offset_is_unchanged_under_stripping():
    from nanomotif_amd.engine import partner_offset
    from nanomotif_amd.motif import Motif
    for s, i, j in (("GATC", 1, 1), ("GAAG[CT]", 2, 3), ("A" + "." * 40 + "C", 0, 20), ("ATTG", 0, 2), ("CC[AT]GG", 1, 0)):
        d = partner_offset(Motif(s, i), j)
        assert d == offset_of(s, i, j)
        for lead, trail in ((2, 1), (0, 3), (4, 0), (1, 1)):
            padded = Motif("." * lead + s + "." * trail, i + lead)
            # the reverse complement of the padded motif carries `trail` dots in front of the partner
            assert partner_offset(padded, j + trail) == d, (s, lead, trail)
            sets, mp = padded.stripped_sets()
            assert 0 <= mp + d < len(sets)
    assert partner_offset(Motif("A", 0), 0) == 0


# ------------------------------------------------------------------------------------------------ the formatters
def _expect_derived(n):
    both = n[0] + n[1] + n[3] + n[4]
    shares = ["%.6f" % (n[0] / both), "%.6f" % ((n[1] + n[3]) / both), "%.6f" % (n[4] / both)] if both else ["nan"] * 3
    p = "nan" if n[1] + n[3] == 0 else "%.6g" % exact_p(n[3], n[1])
    return [str(n[0]), str(n[1]), str(n[3]), str(n[4])] + shares + [p]


def test_formatters_on_hand_made_tables():
    from nanomotif_amd.motif_strands import CONTIGS_HEADER, MAIN_HEADER, StrandCandidate, format_contigs, format_main
    assert MAIN_HEADER == ["bin", "motif", "mod_type", "mod_position", "partner_position", "palindrome"] + ["n_" + t.replace("-", "_") for t in PAIRS] + \
        ["n_full", "n_hemi_own", "n_hemi_partner", "n_unmethylated", "frac_full", "frac_hemi", "frac_unmethylated", "strand_bias_p"]
    assert CONTIGS_HEADER[:6] == ["bin", "contig", "motif", "mod_type", "mod_position", "partner_position"] and len(CONTIGS_HEADER) == 24
    assert CONTIGS_HEADER[6] == "n_mod_mod_fwd" and CONTIGS_HEADER[14] == "n_nocall_nocall_fwd" and CONTIGS_HEADER[15] == "n_mod_mod_rev" and CONTIGS_HEADER[23] == "n_nocall_nocall_rev"
    cands = [StrandCandidate("b1", "GATC", "a", 1, 1), StrandCandidate("b1", "GAAGY", "a", 2, 3), StrandCandidate("b2", "CCWGG", "m", 1, 0),
             StrandCandidate("b3", "GATC", "a", 1, 1)]
    t0 = np.array([[10, 1, 2, 9, 20, 3, 4, 5, 6, 10, 9, 4, 1, 20, 5, 2, 3, 6], [0, 4, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 4, 0, 0, 0, 0, 1]], dtype=np.int64)
    t1 = np.array([[10, 1, 2, 9, 20, 3, 4, 5, 6, 1, 0, 0, 0, 1, 0, 0, 0, 7]], dtype=np.int64)
    t2 = np.array([[0, 0, 3, 0, 0, 0, 2, 0, 9, 0, 0, 1, 0, 0, 0, 0, 4, 0]], dtype=np.int64)          # nothing called on both strands
    t3 = np.zeros((0, 18), dtype=np.int64)                                                          # a bin without contigs
    # the palindrome with j = i counts its '+' occurrences only; the others both strands
    nines = [[10, 5, 2, 9, 20, 3, 4, 5, 7], [11, 1, 2, 9, 21, 3, 4, 5, 13], [0, 0, 4, 0, 0, 0, 2, 4, 9], [0] * 9]
    lines = format_main(cands, [t0, t1, t2, t3]).split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == MAIN_HEADER and len(lines) == 6
    for c, nine, line in zip(cands, nines, lines[1:]):
        assert line.split("\t") == [c.bin, c.motif, c.mod_type, str(c.mod_position), str(c.partner_position), str(int(c.palindrome))] + [str(x) for x in nine] + \
            _expect_derived(nine)
    assert lines[1].split("\t")[4:6] == ["1", "1"] and lines[2].split("\t")[4:6] == ["3", "0"]
    assert lines[1].split("\t")[15:] == ["10", "5", "9", "20", "0.227273", "0.318182", "0.454545", "0.42395"]
    assert lines[3].split("\t")[15:] == ["0", "0", "0", "0", "nan", "nan", "nan", "nan"]
    lines = format_contigs(cands, [["c1", "c2"], ["c1"], ["c9"], []], [t0, t1, t2, t3]).split("\n")
    assert lines[0].split("\t") == CONTIGS_HEADER and len(lines) == 6
    assert lines[1].split("\t") == ["b1", "c1", "GATC", "a", "1", "1"] + [str(x) for x in t0[0]]
    assert lines[2].split("\t") == ["b1", "c2", "GATC", "a", "1", "1"] + [str(x) for x in t0[1]]
    assert lines[3].split("\t") == ["b1", "c1", "GAAGY", "a", "2", "3"] + [str(x) for x in t1[0]]


# ------------------------------------------------------------------------------------------------ the native text writer
def _python_lines(contig, pos, code, seg_begin, names, bins, contig_names, offsets) -> bytes:
    lines = []
    for s in range(len(names)):
        for i in range(int(seg_begin[s]), int(seg_begin[s + 1])):
            t, minus = code[i] & 15, bool(code[i] & 16)
            lines.append("%s\t%d\t%d\t%s\t0\t%s\t%s-%s\t%s\t%d\n" % (contig_names[contig[i]], int(pos[i]), int(pos[i]) + 1, names[s], "-" if minus else "+",
                                                                      STATES[t // 3], STATES[t % 3], bins[s], int(pos[i]) + (-offsets[s] if minus else offsets[s])))
    return "".join(lines).encode()


ALL_CODES = list(range(9)) + [16 + t for t in range(9)]


def _random_span(n, seed):
    rng = np.random.default_rng(seed)
    contig_names = ["contig_1", "c", "NODE_17_length_123456_cov_7.5", "x" * 40, "k141_9"]
    names = ["GATC_a_1", "CCWGG_m_1", "GCACNNNNNNGTT_a_2", "A_a_0", "RGATCY_a_2", "TTAA_21839_3", "G_m_0"]
    bins = ["bin.1", "bin.1", "b2", "a_rather_long_bin_name.fa", "b2", "bin.1", "z"]
    offsets = [1, 3, -8, 0, 95, -95, 2]
    cuts = np.sort(rng.integers(0, n + 1, size=len(names) - 1))
    cuts[2] = cuts[1]                                                   # an empty run in the middle
    seg_begin = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    contig = rng.integers(0, len(contig_names), size=n).astype(np.uint32)
    pos = rng.integers(100, 2 ** 32 - 200, size=n, dtype=np.uint64).astype(np.uint32)
    edge = [2 ** 32 - 200, 100, 999, 1000, 9_999_999, 999_999_999 + 95, 1_000_000_000, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 95]
    pos[:10] = edge[:len(pos[:10])]
    code = rng.choice(np.array(ALL_CODES, dtype=np.uint8), size=n)
    code[:18] = ALL_CODES[:len(code[:18])]
    return contig, pos, code, seg_begin, names, bins, contig_names, offsets


def _format(contig, pos, code, seg_begin, names, bins, contig_names, offsets):
    from nanomotif_amd.motif_sites import format_sites
    return format_sites(contig, pos, code, seg_begin, names, bins, contig_names, symbol="nm_motif_strands_text", seg_partner_offsets=offsets)


def test_native_writer_equals_python_formatting(monkeypatch):
    for n, seed in ((5000, 1), (4097, 2), (18, 3), (1, 4)):
        span = _random_span(n, seed)
        expect = _python_lines(*span)
        got = {}
        for threads in ("1", "8", "3"):
            monkeypatch.setenv("NM_POST_THREADS", threads)
            got[threads] = _format(*span)
        assert got["1"] == expect, n
        assert got["8"] == got["1"] and got["3"] == got["1"]
    empty = np.zeros(0, np.uint32)
    assert _format(empty, empty, np.zeros(0, np.uint8), np.zeros(2, np.uint64), ["GATC_a_1"], ["b"], ["c"], [1]) == b""


def test_native_writer_refuses_bad_records_and_short_buffers():
    from nanomotif_amd import _lib
    contig, pos, code, seg_begin, names, bins, contig_names, offsets = _random_span(600, 7)
    for wrong in (9, 15, 16 + 9, 32, 64 + 1):                              # a code outside the eighteen
        bad = code.copy()
        bad[300] = wrong
        with pytest.raises(_lib.NmScanError) as e:
            _format(contig, pos, bad, seg_begin, names, bins, contig_names, offsets)
        assert e.value.code == -1
    far = contig.copy()
    far[599] = len(contig_names)
    with pytest.raises(_lib.NmScanError):
        _format(far, pos, code, seg_begin, names, bins, contig_names, offsets)
    low = pos.copy()                                                    # a partner before the start of the contig
    low[:] = 3
    with pytest.raises(_lib.NmScanError) as e:
        _format(contig, low, code, seg_begin, names, bins, contig_names, offsets)
    assert e.value.code == -1
    lib = _lib.load()
    assert lib.nm_motif_strands_text(1, None, None, None, 0, None, None, None, None, 0, None, None, None, 0, None) == -1      # NM_EINVAL
    n = C.c_uint64(7)
    assert lib.nm_motif_strands_text(0, None, None, None, 0, None, None, None, None, 0, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    one = (np.zeros(1, np.uint32), np.array([41], np.uint32), np.array([16 + 1], np.uint8), np.array([0, 1], np.uint64), np.array([2], np.int32))
    off = np.array([0, 8, 9], np.uint64)
    coff = np.array([0, 2], np.uint64)
    head = (1, p(one[0], C.c_uint32), p(one[1], C.c_uint32), p(one[2], C.c_uint8), 1, p(one[3], C.c_uint64), b"GATC_a_1b", p(off, C.c_uint64))
    tail = (1, b"c1", p(coff, C.c_uint64))
    assert lib.nm_motif_strands_text(*head, None, *tail, None, 0, C.byref(n)) == -1                 # the offsets are not optional
    args = head + (p(one[4], C.c_int32),) + tail
    assert lib.nm_motif_strands_text(*args, None, 0, C.byref(n)) == 0
    line = b"c1\t41\t42\tGATC_a_1\t0\t-\tmod-nomod\tb\t39\n"          # on '-' the partner is at position - d
    assert n.value == len(line)
    buf = C.create_string_buffer(len(line))
    assert lib.nm_motif_strands_text(*args, buf, len(line) - 1, C.byref(n)) == -5                   # NM_ERANGE: nothing is cut off
    assert lib.nm_motif_strands_text(*args, buf, len(line), C.byref(n)) == 0 and buf.raw == line
    one[2][0] = 3                                                       # the same record on '+': partner at position + d
    assert lib.nm_motif_strands_text(*args, buf, len(line), C.byref(n)) == 0 and buf.raw == b"c1\t41\t42\tGATC_a_1\t0\t+\tnomod-mod\tb\t43\n"
    # the neighbours' writers are what they were: eight columns
    cmp_args = head + tail
    assert lib.nm_motif_compare_text(*cmp_args, buf, len(line), C.byref(n)) == 0 and buf.raw[:n.value] == b"c1\t41\t42\tGATC_a_1\t0\t+\tnomod>mod\tb\n"


# ------------------------------------------------------------------------------------------------ exports
def test_exports_are_declared_bound_and_built():
    from nanomotif_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    for name in ("nm_motif_strands_count", "nm_motif_strands_sites", "nm_motif_strands_text"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS
    for line in ("#define NM_STRANDS_MINUS 16u", "#define NM_STRANDS_ALL 0x1FFu", "#define NM_STRANDS_HEMI ((1u << 1) | (1u << 3))"):
        assert line in header
    assert any(os.path.basename(s) == "nmstrands.hip" for s in build.SRC_HIP)
    lib = _lib.load()
    assert lib.nm_abi_version() == 1
    # NULL arguments are refused before anything touches a device
    assert lib.nm_motif_strands_count(None, 1, None, None, None, None, None, None, None, 0x1FF, None, None, None) == -1
    assert lib.nm_motif_strands_sites(None, 1, None, None, None, None, None, None, None, 0x1FF, 0, 0, None, None, None, None, None) == -1
    rows, tot, tab = np.array([0, 1], np.uint64), np.zeros(1, np.uint64), np.zeros((1, 18), np.int64)
    q = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    assert lib.nm_motif_strands_count(None, 1, None, None, None, None, None, None, None, 0x1FF, q(rows, C.c_uint64), q(tot, C.c_uint64), q(tab, C.c_int64)) == -1
