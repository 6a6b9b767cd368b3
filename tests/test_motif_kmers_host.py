"""Host side of ``nanomotif motif_kmers`` (no GPU): the brute force both suites compare against — strings, slices, a reverse complement by
``str.translate`` and a dict (contig, position, strand) -> fraction with the 0.7 / 0.3 rule; nothing of the engine's bit planes —, the
conditions on the input it runs on, the shape parser and the row index, ``implied`` / ``compatible`` on cases derived by hand, the four
files byte for byte from hand-made tables, and the reverse-complement identity of the definition itself."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser
from test_motif_profile_host import CHUNK, profile_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "ACGT"
COMP = str.maketrans("ACGT", "TGCA")
CANONICAL = {"a": "A", "m": "C", "21839": "C"}
SLOTS = ("a", "m", "21839")                                             # slot order of the k-mer engine
BINS = ("b0_empty", "b1", "b2", "b3")
KMER_SEED = 20240
# planted in the random bin on '+' in its first and third chunk and as the reverse complement in its second: the row of the centre site
# receives sites from different chunks and from both strands at every F
WORDS = {"A": "CGTTAGCCTGAGTCAAGCTTG", "C": "CGTTAGCCTGCGTCAAGCTTG"}
# the shapes of the GPU suite: F = 0; one offset either side; 5; 6 (the last LDS size); 7 (the first global size); 10; the single offsets
# -31 and +31; a bipartite one
SHAPES = ["*", "N*", "*N", "NN*NNN", "NNN*NNN", "NNNN*NNN", "NNNNN*NNNNN", "N" + "." * 30 + "*", "*" + "." * 30 + "N", "NNN*......NNN"]


def offsets_of(shape):
    centre = shape.index("*")
    return tuple(j - centre for j, ch in enumerate(shape) if ch == "N")


# ------------------------------------------------------------------------------------------------ the input (shared with the GPU suite)
@functools.lru_cache(maxsize=None)
def kmer_input():
    """(names, seqs, bins, bin_names, {mod type: rows}, {mod type: {(contig, position, strand 0 / 1): fraction}}): ``profile_input`` (contigs
    over word, lane and chunk borders, an N run across a chunk border, contigs shorter than a motif) plus, in b1, two short contigs that
    start and end in each of the four letters and hold every letter either side of an N; in b2 a 20 kbp all-A contig with calls; a bin b3
    of one random contig longer than three chunks; and a "21839" pileup over everything."""
    names, seqs, bins, _, rows, _ = profile_input()
    names, seqs, bins = list(names), dict(seqs), dict(bins)
    rng = np.random.default_rng(KMER_SEED)
    rand = lambda n: "".join(rng.choice(list(LETTERS), size=n))
    fresh = {"cap1": ("TACG" + rand(40) + "ANATNTCNCGNG" + rand(40) + "CGTA", "b1"), "cap2": ("CATG" + rand(90) + "CATG", "b1"),
             "polyA": ("A" * 20_000, "b2"), "rand3": (rand(3 * CHUNK + 1_000), "b3")}
    r3 = list(fresh["rand3"][0])
    for k, word in enumerate(WORDS.values()):
        r3[1_000 + 100 * k:1_021 + 100 * k] = word
        r3[CHUNK + 3_000 + 100 * k:CHUNK + 3_021 + 100 * k] = word.translate(COMP)[::-1]
        r3[2 * CHUNK + 500 + 100 * k:2 * CHUNK + 521 + 100 * k] = word
    fresh["rand3"] = ("".join(r3), "b3")
    for n, (s, b) in fresh.items():
        names.append(n)
        seqs[n], bins[n] = s, b

    def draw(contigs):
        cid, pos, st, fr = [], [], [], []
        for n in contigs:
            p, s = np.nonzero(rng.random((len(seqs[n]), 2)) < 0.6)
            cid.append(np.full(len(p), names.index(n), np.uint32)); pos.append(p)
            st.append(np.where(s == 0, ord("+"), ord("-")).astype(np.uint8)); fr.append(rng.choice([0.0, 0.3, 0.5, 0.7, 1.0], size=len(p)))
        return tuple(np.concatenate(x) for x in (cid, pos, st, fr))
    out = {}
    for mt in ("a", "m"):
        more = draw(list(fresh))
        out[mt] = tuple(np.concatenate([np.asarray(a), b]) for a, b in zip(rows[mt], more))
    out["21839"] = draw(names)
    calls = {mt: {(names[int(c)], int(p), 0 if s == ord("+") else 1): float(f) for c, p, s, f in zip(*out[mt])} for mt in SLOTS}
    for mt in SLOTS:
        assert len(calls[mt]) == len(out[mt][0])                        # no (position, strand) twice: the dict IS the pileup
    return names, seqs, bins, list(BINS), out, calls


def contigs_of(bin_name):
    names, seqs, bins, _, _, _ = kmer_input()
    return [(n, seqs[n]) for n in names if bins[n] == bin_name]


# ------------------------------------------------------------------------------------------------ the brute force
def state_of(fraction):
    """0 mod, 1 nomod, 2 nocall."""
    if fraction is None:
        return 2
    return 0 if fraction >= 0.7 else 1 if fraction <= 0.3 else 2


@functools.lru_cache(maxsize=None)
def sites_of(seq, base):
    """[(strand, p, the contig read on that strand, q = the site's index in it)] of every site of ``base``."""
    rc = seq.translate(COMP)[::-1]
    return [(0, q, seq, q) for q in range(len(seq)) if seq[q] == base] + [(1, len(seq) - 1 - q, rc, q) for q in range(len(rc)) if rc[q] == base]


def window_row(text, q, offsets):
    """The row of the site at ``q`` of ``text``; -1 when a probed position lies outside or holds no A, C, G, T."""
    row = 0
    for o in offsets:
        letter = text[q + o:q + o + 1] if q + o >= 0 else ""
        if letter not in LETTERS or not letter:
            return -1
        row = row * 4 + LETTERS.index(letter)
    return row


def site_rows(contigs, base, offsets):
    """[(contig, p, strand, row or -1)] of every site of ``base`` in ``contigs`` = [(name, sequence)]."""
    return [(name, p, s, window_row(text, q, offsets)) for name, seq in contigs for s, p, text, q in sites_of(seq, base)]


def tally(rows, calls, n_offsets):
    totals, table = np.zeros((2, 3), dtype=np.int64), np.zeros((4 ** n_offsets, 3), dtype=np.int64)
    for name, p, s, row in rows:
        st = state_of(calls.get((name, p, s)))
        totals[s, st] += 1
        if row >= 0:
            table[row, st] += 1
    return totals, table


def brute(contigs, calls, base, offsets):
    """(totals int64[2, 3], table int64[4^F, 3]) over ``contigs`` = [(name, sequence)]."""
    return tally(site_rows(contigs, base, offsets), calls, len(offsets))


@functools.lru_cache(maxsize=None)
def shared_site_rows(shape, base, bin_name):
    return site_rows(contigs_of(bin_name), base, offsets_of(shape))


@functools.lru_cache(maxsize=None)
def expected(shape, mod_type, bin_name):
    """(totals, table) of one request of the shared input (the windows of a bin are walked once per canonical base)."""
    _, _, _, _, _, calls = kmer_input()
    return tally(shared_site_rows(shape, CANONICAL[mod_type], bin_name), calls[mod_type], len(offsets_of(shape)))


def all_requests():
    return [(mt, b) for b in BINS for mt in SLOTS]


def expected_all(shape, requests=None):
    requests = all_requests() if requests is None else requests
    return np.stack([expected(shape, mt, b)[0] for mt, b in requests]), np.stack([expected(shape, mt, b)[1] for mt, b in requests])


def incomplete_reasons(contigs, base, offsets):
    """{"start", "end", "N"}: why windows are incomplete, in contig coordinates."""
    seen = set()
    for _, seq in contigs:
        for s, p, _, _ in sites_of(seq, base):
            for o in offsets:
                at = p + o if s == 0 else p - o
                seen.add("start" if at < 0 else "end" if at >= len(seq) else "N" if seq[at] == "N" else "")
    return seen - {""}


def row_sources(contigs, base, offsets, row):
    """{(contig, chunk of the contig, strand)} of the complete sites of ``row``."""
    return {(name, p // CHUNK, s) for name, p, s, r in site_rows(contigs, base, offsets) if r == row}


# ------------------------------------------------------------------------------------------------ non-degeneracy, on the brute force alone
def test_the_input_is_not_degenerate():
    names, seqs, bins, bin_names, rows, calls = kmer_input()
    assert bin_names == list(BINS) and not contigs_of("b0_empty")                      # the empty bin exists
    assert len(seqs["polyA"]) == 20_000 and set(seqs["polyA"]) == {"A"} and any(k[0] == "polyA" for k in calls["a"])
    assert len(seqs["rand3"]) > 3 * CHUNK and [n for n, _ in contigs_of("b3")] == ["rand3"]
    assert seqs["big"][3 * CHUNK - 6:3 * CHUNK + 9] == "N" * 15 and min(len(s) for s in seqs.values()) < 4
    for shape in SHAPES:
        offsets = offsets_of(shape)
        for base in "AC":
            if offsets:                                                                # incomplete at a start, at an end and through an N
                assert incomplete_reasons(contigs_of("b1"), base, offsets) == {"start", "end", "N"}, (shape, base)
        for mt in SLOTS:                                                               # the A slot and the C slots: non-empty tables
            for b in BINS[1:]:
                totals, table = expected(shape, mt, b)
                assert table.sum() > 0 and (totals.sum(axis=0) - table.sum(axis=0) >= 0).all(), (shape, mt, b)
                if offsets and b == "b1":
                    assert (totals.sum(axis=0) - table.sum(axis=0)).sum() > 0, (shape, mt, b)
            totals, _ = expected(shape, mt, "b1")
            assert (totals > 0).all(), (mt, totals.tolist())                           # all three states on both strands
        # a row that receives sites from different chunks and from both strands
        for mt in ("a", "m"):
            word = WORDS[CANONICAL[mt]]
            row = window_row(word, 10, offsets) if all(abs(o) <= 10 for o in offsets) else int(expected(shape, mt, "b3")[1].sum(axis=1).argmax())
            src = row_sources(contigs_of("b3"), CANONICAL[mt], offsets, row)
            assert len({(n, c) for n, c, _ in src}) >= 2 and {s for _, _, s in src} == {0, 1}, (shape, mt)
    assert not expected("NNN*NNN", "a", "b0_empty")[0].any() and not expected("NNN*NNN", "a", "b0_empty")[1].any()


def test_the_reverse_complement_input_exchanges_the_strands():
    """Reverse-complementing every contig and mirroring the calls (position -> len - 1 - position, strands exchanged) leaves ``table``
    as it is and exchanges the strands of ``totals``: a site and its window are properties of the duplex."""
    names, seqs, bins, _, _, calls = kmer_input()
    for shape in ("N*", "NN*NNN", "NNN*......NNN", "*" + "." * 30 + "N"):
        for mt, b in (("a", "b1"), ("m", "b2"), ("21839", "b3")):
            contigs = contigs_of(b)
            mirrored = [(n, s.translate(COMP)[::-1]) for n, s in contigs]
            length = dict((n, len(s)) for n, s in contigs)
            mcalls = {(n, length[n] - 1 - p, 1 - s): f for (n, p, s), f in calls[mt].items() if n in length}
            totals, table = expected(shape, mt, b)
            t_m, tab_m = brute(mirrored, mcalls, CANONICAL[mt], offsets_of(shape))
            assert np.array_equal(tab_m, table) and np.array_equal(t_m, totals[::-1]), (shape, mt, b)
            assert not np.array_equal(totals, totals[::-1])


# ------------------------------------------------------------------------------------------------ the shape parser and the row index
def test_shape_parser():
    from nanomotif_amd.engine import KMER_MAX_FLANKS, KMER_MAX_OFFSET, kmer_shape
    assert (KMER_MAX_FLANKS, KMER_MAX_OFFSET) == (10, 31)
    assert kmer_shape("NNN*NNN") == (-3, -2, -1, 1, 2, 3) and kmer_shape("*") == () and kmer_shape("N*") == (-1,) and kmer_shape("*.N") == (2,)
    assert kmer_shape("NNN*......NNN") == (-3, -2, -1, 7, 8, 9) and kmer_shape("..N*N..") == (-1, 1)
    assert kmer_shape([3, -1, 1]) == (-1, 1, 3) and kmer_shape(()) == () and kmer_shape("N" + "." * 30 + "*") == (-31,)
    for shape in SHAPES:
        assert kmer_shape(shape) == offsets_of(shape)
    for bad, word in (("NNN", "exactly one *"), ("N*N*N", "exactly one *"), ("NNNNNN*NNNNN", "at most 10"), ("N" + "." * 31 + "*", "more than 31"),
                      ("*" + "." * 31 + "N", "more than 31"), ("NNx*", "only N, . and *"), ("nn*", "only N, . and *"), ([1, 1], "distinct"),
                      ([0, 1], "non-zero"), ([32], "more than 31"), (list(range(1, 12)), "at most 10")):
        with pytest.raises(ValueError) as e:
            kmer_shape(bad)
        assert word in str(e.value), (bad, str(e.value))


def test_row_index_and_text_round_trip():
    from nanomotif_amd.engine import kmer_motif, kmer_row, kmer_text
    assert kmer_text("N*NN", "A", 0b10_11_01) == "GATC" and kmer_text("NN*", "C", 0) == "AAC" and kmer_text("*", "A", 0) == "A"
    assert kmer_text("NNN*......NNN", "A", kmer_row("NNN*......NNN", "GATA......TCC")) == "GATA......TCC"
    assert kmer_text("*..N", "C", 3) == "C..T" and kmer_text("N..*", "C", 2) == "G..C"
    m = kmer_motif("N*NN", "A", 0b10_11_01)
    assert (m.string, m.mod_position) == ("GATC", 1)
    m = kmer_motif("*.N", "C", 1)
    assert (m.string, m.mod_position) == ("C.C", 0)
    for shape in ("N*", "NN*NNN", "NNN*......NNN", "*" + "." * 30 + "N"):
        n = 4 ** len(offsets_of(shape))
        for row in sorted({0, 1, n // 3, n - 2, n - 1} & set(range(n))):
            text = kmer_text(shape, "A", row)
            assert kmer_row(shape, text) == row and len(text) == len(shape.strip(".")) and text[shape.strip(".").index("*")] == "A"
            digits = [LETTERS.index(text[j]) for j, ch in enumerate(shape.strip(".")) if ch == "N"]
            assert sum(d * 4 ** (len(digits) - 1 - f) for f, d in enumerate(digits)) == row      # the first offset is the most significant
    for bad in (-1, 16):
        with pytest.raises(ValueError):
            kmer_text("N*N", "A", bad)


# ------------------------------------------------------------------------------------------------ implied, compatible, the four files
def test_implied_and_compatible_by_hand():
    from nanomotif_amd.engine import kmer_row
    from nanomotif_amd.motif_kmers import relation
    rel = lambda motif, pos, shape, text, base="A": relation(motif, pos, shape, base, kmer_row(shape, text))
    # GATC @ 1 constrains offsets -1 G, 0 A, 1 T, 2 C.  N*NN counts all of them: it implies GATC and nothing else
    assert rel("GATC", 1, "N*NN", "GATC") == "implied"
    assert [rel("GATC", 1, "N*NN", t) for t in ("AATC", "GAAC", "GATA", "CATC")] == ["", "", "", ""]
    # NN*N counts -2, -1, 1: the C at offset 2 is outside, so GATC never implies; .GAT is compatible, everything else is neither
    assert [rel("GATC", 1, "NN*N", t) for t in ("AGAT", "CGAT", "TGAT")] == ["compatible"] * 3
    assert [rel("GATC", 1, "NN*N", t) for t in ("AGAA", "ACAT", "AAAT")] == ["", "", ""]
    # G[AG]TC = GRTC admits the canonical base; GTTC does not and relates to nothing
    assert rel("GRTC", 1, "N*NN", "GATC") == "implied" and rel("GRTC", 1, "N*NN", "GATG") == ""
    assert rel("GTTC", 1, "N*NN", "GATC") == "" and rel("GATC", 1, "N*NN", "GCTC", base="C") == ""
    assert rel("RGATCY", 2, "NN*NNN", "AGATCT") == "implied" and rel("RGATCY", 2, "NN*NNN", "CGATCT") == "" and rel("RGATCY", 2, "NN*NNN", "GGATCA") == ""
    # a motif longer than the shape: compatible where the overlap fits; N positions of the motif constrain nothing
    assert rel("GATCNNNNNNGTT", 1, "N*NN", "GATC") == "compatible" and rel("GATCNNNNNNGTT", 1, "N*NN", "GATG") == ""
    assert rel("GANTC", 1, "N*.NN", "GA.TC") == "implied" and rel("GANTC", 1, "N*NNN", "GACTC") == "implied"
    assert rel("A", 0, "N*N", "CAT") == "implied" and rel("A", 0, "*", "A") == "implied"


def _cand(bin, motif, mod_type, pos):
    from nanomotif_amd.motif_sites import SiteCandidate
    return SiteCandidate(bin, motif, mod_type, pos)


def _hand_tables():
    """Two requests under N*N: hand-made rows around the limits 20 (called), 0.7 (unexplained) and 0.3 (overcalled)."""
    from nanomotif_amd.engine import kmer_row
    requests = [("b2", "m"), ("b1", "a")]                                  # (out of order: the files sort by bin, mod type)
    totals = np.array([[[10, 30, 5], [10, 30, 6]], [[100, 100, 10], [60, 60, 5]]], dtype=np.int64)
    tables = np.zeros((2, 16, 3), dtype=np.int64)
    row = lambda text: kmer_row("N*N", text)
    tables[1, row("GAT")] = (14, 6, 2)                                     # 20 called, 0.7 exactly: written, unexplained without a motif
    tables[1, row("CAT")] = (14, 5, 9)                                     # 19 called: not written
    tables[1, row("AAT")] = (69, 31, 0)                                    # 0.69: written, not unexplained
    tables[1, row("TAG")] = (6, 14, 0)                                     # 0.3 exactly: not overcalled
    tables[1, row("TAC")] = (29, 71, 1)                                    # 0.29: overcalled when a motif implies it
    tables[0, row("CCG")] = (20, 0, 3)
    return requests, totals, tables


def test_the_four_files_byte_for_byte():
    from nanomotif_amd.motif_kmers import BINS_HEADER, MAIN_HEADER, MOTIF_COLUMNS, format_files
    requests, totals, tables = _hand_tables()
    assert MAIN_HEADER == ["bin", "mod_type", "kmer", "n_mod", "n_nomod", "n_nocall", "frac_mod", "bin_frac_mod"] and MOTIF_COLUMNS == ["implied_by", "compatible_with"]
    head = "\t".join(MAIN_HEADER) + "\n"
    main, bins = format_files(requests, totals, tables, "N*N")
    assert main == head + ("b1\ta\tAAT\t69\t31\t0\t0.690000\t0.500000\n" "b1\ta\tGAT\t14\t6\t2\t0.700000\t0.500000\n" "b1\ta\tTAC\t29\t71\t1\t0.290000\t0.500000\n"
                           "b1\ta\tTAG\t6\t14\t0\t0.300000\t0.500000\n" "b2\tm\tCCG\t20\t0\t3\t1.000000\t0.250000\n")
    assert bins == "\t".join(BINS_HEADER) + "\n" + "b1\ta\t100\t100\t10\t60\t60\t5\t28\t33\t3\t4\n" "b2\tm\t10\t30\t5\t10\t30\t6\t0\t60\t8\t1\n"
    motifs = [_cand("b1", "TAS", "a", 1), _cand("b1", "GATC", "a", 1), _cand("b2", "GAT", "a", 1), _cand("b1", "NAT", "m", 1)]
    main, bins2, unexplained, overcalled = format_files(requests, totals, tables, "N*N", motifs)
    head = "\t".join(MAIN_HEADER + MOTIF_COLUMNS) + "\n"
    assert bins2 == bins
    assert main == head + ("b1\ta\tAAT\t69\t31\t0\t0.690000\t0.500000\t\t\n" "b1\ta\tGAT\t14\t6\t2\t0.700000\t0.500000\t\tGATC_a_1\n"
                           "b1\ta\tTAC\t29\t71\t1\t0.290000\t0.500000\tTAS_a_1\t\n" "b1\ta\tTAG\t6\t14\t0\t0.300000\t0.500000\tTAS_a_1\t\n"
                           "b2\tm\tCCG\t20\t0\t3\t1.000000\t0.250000\t\t\n")
    # a motif of another bin or mod type plays no part: CCG of (b2, m) stays unexplained; GAT is compatible with GATC and is not
    assert unexplained == head + "b2\tm\tCCG\t20\t0\t3\t1.000000\t0.250000\t\t\n"
    assert overcalled == head + "b1\ta\tTAC\t29\t71\t1\t0.290000\t0.500000\tTAS_a_1\t\n"
    # without the motifs that account for it GAT (0.7 exactly) is unexplained; an empty list still writes four files
    four = format_files(requests, totals, tables, "N*N", [])
    assert len(four) == 4 and four[2] == head + "b1\ta\tGAT\t14\t6\t2\t0.700000\t0.500000\t\t\n" "b2\tm\tCCG\t20\t0\t3\t1.000000\t0.250000\t\t\n" and four[3] == head


def test_min_called_and_min_frac_are_compared_with_greater_or_equal():
    from nanomotif_amd.motif_kmers import format_files
    requests, totals, tables = _hand_tables()
    kmers = lambda text: [line.split("\t")[2] for line in text.split("\n")[1:-1]]
    assert kmers(format_files(requests, totals, tables, "N*N", min_called=19)[0]) == ["AAT", "CAT", "GAT", "TAC", "TAG", "CCG"]
    assert kmers(format_files(requests, totals, tables, "N*N", min_called=20)[0]) == ["AAT", "GAT", "TAC", "TAG", "CCG"]
    assert kmers(format_files(requests, totals, tables, "N*N", min_called=21)[0]) == ["AAT", "TAC"]
    assert kmers(format_files(requests, totals, tables, "N*N", [], min_frac=0.7)[2]) == ["GAT", "CCG"]
    assert kmers(format_files(requests, totals, tables, "N*N", [], min_frac=0.69)[2]) == ["AAT", "GAT", "CCG"]
    assert kmers(format_files(requests, totals, tables, "N*N", [], min_frac=0.7000001)[2]) == ["CCG"]
    assert kmers(format_files(requests, totals, tables, "N*N", [], min_called=21, min_frac=0.0)[2]) == ["AAT", "TAC"]


# ------------------------------------------------------------------------------------------------ the parser, the engine, the exports
def test_parser_accepts_motif_kmers(capsys):
    p = create_parser()
    a = p.parse_args(["motif_kmers", "asm.fasta", "p.bed", "-c", "contig_bin.tsv", "--out", "km"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.out, a.bin_motifs, a.shape, a.min_called, a.min_frac) == \
        ("motif_kmers", "asm.fasta", "p.bed", "contig_bin.tsv", "km", None, "NNN*NNN", 20, 0.7)
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose, a.threads) == (0.3, 0.7, 5, None, False, 1)
    a = p.parse_args(["motif_kmers", "asm.fasta", "p.bed.gz", "-d", "bins", "--bin_motifs", "a.tsv", "b.tsv", "--shape", "NNN*......NNN", "--min_called", "5",
                      "--min_frac", "0.5", "--device", "1"])
    assert (a.bin_motifs, a.shape, a.min_called, a.min_frac, a.device) == (["a.tsv", "b.tsv"], "NNN*......NNN", 5, 0.5, 1)
    for bad in ("NNN", "N*N*", "NNNNNN*NNNNN", "N" + "." * 31 + "*", "NX*"):
        with pytest.raises(SystemExit):
            p.parse_args(["motif_kmers", "asm.fasta", "p.bed", "-c", "cb.tsv", "--shape", bad])
        assert "--shape" in capsys.readouterr().err
    assert "motif_kmers" in p.format_help()


def test_engine_refuses_a_bad_shape_before_it_needs_a_device():
    from nanomotif_amd.engine import ScanEngine
    eng = ScanEngine.__new__(ScanEngine)                                # no context: the check comes first
    for bad in ("NNN", "NNNNNN*NNNNN", [0], [40]):
        with pytest.raises(ValueError):
            ScanEngine.kmer_methylation(eng, [], bad)
    eng.ctx = None                                                      # (nothing for __del__ to destroy)


def test_exports_are_declared_bound_and_built():
    from nanomotif_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    assert "int nm_kmer_methylation(" in header and "nm_kmer_methylation" in _lib.SYMBOLS
    assert "#define NM_KMER_MAX_FLANKS 10" in header and "#define NM_KMER_MAX_OFFSET 31" in header
    assert any(os.path.basename(s) == "nmkmers.hip" for s in build.SRC_HIP)
    lib = _lib.load()
    bins, slots, totals, table = np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(6, np.uint64), np.zeros(3 * 4 ** 10, np.uint64)
    q = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    good = (q(bins, C.c_uint32), q(slots, C.c_uint8))
    out = (q(totals, C.c_uint64), q(table, C.c_uint64))

    def call(offsets, req=good, out=out, n=1):
        off = np.asarray(offsets, np.int8)
        return lib.nm_kmer_methylation(None, n, *req, len(off), q(off, C.c_int8) if len(off) else None, *out)
    last = lambda: lib.nm_last_error().decode()
    # refused with a NULL ctx, before any device call, in the order NULLs, shape, ctx
    for kw in (dict(req=(None, good[1])), dict(req=(good[0], None)), dict(out=(None, out[1])), dict(out=(out[0], None))):
        assert call([0, 0], **kw) == -1 and "NULL" in last(), kw        # (the NULL comes before the bad shape)
    assert lib.nm_kmer_methylation(None, 1, *good, 2, None, *out) == -1 and "NULL" in last()
    for offsets, word in (([-1, 0, 1], "offsets[1]"), ([32], "offsets[0]"), ([-32, 1], "offsets[0]"), ([1, 1], "offsets[1]"), ([2, 1], "offsets[1]"),
                          ([-3, -2, -1, 5, 4], "offsets[4]"), (list(range(1, 12)), "n_offsets 11")):
        assert call(offsets) == -1 and word in last(), (offsets, last())
        assert call(offsets, n=0, req=(None, None), out=(None, None)) == -1 and word in last()     # the shape is checked whatever n_req is
    assert call([-1, 1]) == -1 and "ctx" in last()
    assert call([], n=0, req=(None, None), out=(None, None)) == -1 and "ctx" in last()             # n_req = 0 still needs a ctx
    assert not totals.any() and not table.any()
