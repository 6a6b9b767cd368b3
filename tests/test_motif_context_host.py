"""Host side of ``nanomotif motif_context`` (no GPU): the brute force both suites compare against — built only from
``test_motif_profile_host.occurrences``, its ``Classes`` / ``probe_class`` (the state of an occurrence is the class of its own base on its
own strand under its own mod type: 0 mod, 1 nomod, anything else nocall) and plain string indexing with a complement table —, the
conditions on the geometry input it runs on, the identities that fix offsets, letters and strands, gain / keep / flag on hand-made
tables, the three files' text, the parser, and the exports in the header and the binding.

``context_by_loops`` is the definition: one occurrence, one offset, one probe at a time.  ``context_of`` is the same walk with the loop
over the occurrences of one contig and strand taken as one numpy index; the two are compared on whole candidates below."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser
from test_motif_profile_host import CANONICAL, CHUNK, COMPLEMENT, Classes, bin_contigs_of, occurrences, probe_class, profile_cands, profile_classes, profile_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "ACGT"
PAD = Classes.PAD


# ------------------------------------------------------------------------------------------------ the brute force
def own_state(seq, calls, base, p, s):
    c = probe_class(seq, calls, base, p, s)
    return c if c in (0, 1) else 2


def letter_of(seq, q, s):
    """0..3 for A, C, G, T read on strand s at q; 4 (other) for N, any other character and a position outside the contig."""
    if not 0 <= q < len(seq):
        return 4
    ch = seq[q] if s == 0 else COMPLEMENT.get(seq[q], "?")
    return LETTERS.index(ch) if ch in LETTERS else 4


def context_by_loops(seq, calls, base, motif, i, radius):
    """(states[2][3], table[2 R + 1][2][3][5]) of one candidate on one contig, one probe at a time."""
    states = np.zeros((2, 3), dtype=np.int64)
    table = np.zeros((2 * radius + 1, 2, 3, 5), dtype=np.int64)
    for p, s in occurrences(seq, motif, i):
        st = own_state(seq, calls, base, p, s)
        states[s, st] += 1
        for o in range(-radius, radius + 1):
            table[o + radius, s, st, letter_of(seq, p + o if s == 0 else p - o, s)] += 1
    return states, table


@functools.lru_cache(maxsize=None)
def letter_codes(seq):
    """int8[2, L + 2 PAD]: ``letter_of`` of every (strand, position) of ``seq``, PAD positions of `other` either side."""
    a = np.full((2, len(seq) + 2 * PAD), 4, dtype=np.int8)
    for s in (0, 1):
        a[s, PAD:PAD + len(seq)] = [letter_of(seq, q, s) for q in range(len(seq))]
    return a


def context_of(names, mod_type, motif, i, radius, classes=None):
    """(states[2][3], table[2 R + 1][2][3][5]) of one candidate summed over the contigs ``names`` of ``classes`` (default: those of the
    geometry input)."""
    assert radius <= PAD
    classes = classes or profile_classes()
    states = np.zeros((2, 3), dtype=np.int64)
    table = np.zeros((2 * radius + 1, 2, 3, 5), dtype=np.int64)
    for name in names:
        occ = occurrences(classes.seqs[name], motif, i)
        cls, codes = classes.cls[(mod_type, name)], letter_codes(classes.seqs[name])
        for s in (0, 1):
            own = np.array([p for p, st in occ if st == s], dtype=np.int64)
            st = np.minimum(cls[s, own + PAD].astype(np.int64), 2)       # classes 2 (nocall) and 3 (other) are the state nocall
            states[s] += np.bincount(st, minlength=3)
            for o in range(-radius, radius + 1):
                q = own + o if s == 0 else own - o
                table[o + radius, s] += np.bincount(st * 5 + codes[s, q + PAD], minlength=15).reshape(3, 5)
    return states, table


@functools.lru_cache(maxsize=None)
def context_expected():
    """Per candidate of ``profile_cands`` (states, table) at radius 31; smaller radii are its middle slices by definition."""
    names, _, bins, _, _, _ = profile_input()
    contigs = bin_contigs_of(names, bins)
    return [context_of(contigs[b], mt, m, i, 31) for b, mt, m, i in profile_cands()]


def middle(table, radius, axis=0):
    return np.take(table, range(31 - radius, 31 + radius + 1), axis=axis)


def narrowed(motif, i, o, letter):
    """(motif, mod position) narrowed to ``letter`` at offset ``o``, padded with dots outside; None when the motif excludes the letter."""
    toks = re.findall(r"\[[^\]]*\]|.", motif)
    at = i + o
    if at < 0:
        toks, i, at = ["."] * (-at) + toks, i - at, 0
    elif at >= len(toks):
        toks = toks + ["."] * (at + 1 - len(toks))
    if toks[at] != "." and letter not in toks[at]:
        return None
    toks[at] = letter
    return "".join(toks), i


# ------------------------------------------------------------------------------------------------ non-degeneracy, on the brute force alone
def test_the_input_is_not_degenerate():
    names, seqs, bins, _, _, _ = profile_input()
    cands, exp = profile_cands(), context_expected()
    assert len(cands) == 18
    total = sum(t for _, t in exp)                                       # [offset][s][state][letter]
    print("min over the cells, per strand:", int(total[..., :4].min()), "pooled:", int(total[..., :4].sum(axis=1).min()))
    assert (total[..., :4] > 0).all() and (total[..., :4].sum(axis=1) >= 90).all()
    with_other = [(b, m) for (b, _, m, _), (_, t) in zip(cands, exp) if t[..., 4].sum() > 0]
    assert len(with_other) == 17 and ("b2", "AATT") not in with_other
    # GATC @ 1 on the 30 kbp contig: own base and probe in different chunks, lanes and words at the four offsets
    occ = occurrences(seqs["big"], "GATC", 1)
    assert {(8191, 0), (8192, 1), (16384, 0)} <= set(occ)
    for o in (-31, -1, 1, 31):
        pairs = [(p, p + o if s == 0 else p - o) for p, s in occ]
        for unit in (CHUNK, 128, 32):
            assert any(p // unit != q // unit for p, q in pairs), (o, unit)
    # an N run across a chunk border, probes before position 0 and past the end, contigs shorter than the motif
    assert seqs["big"][3 * CHUNK - 6:3 * CHUNK + 9] == "N" * 15
    seen = {(s, (p + o if s == 0 else p - o) < 0) for p, s in occurrences(seqs["edge"], "GATC", 1) for o in range(-31, 32)
            if not 0 <= (p + o if s == 0 else p - o) < len(seqs["edge"])}
    assert seen == {(0, True), (0, False), (1, True), (1, False)}
    assert min(len(s) for s in seqs.values()) < 4


def test_the_vectorised_walk_is_the_loop():
    names, seqs, bins, _, _, _ = profile_input()
    classes = profile_classes()
    for name in ("edge", "small", "tiny1", "tiny2", "tiny3"):
        for m, i, mt in (("GATC", 1, "a"), ("AATT", 0, "a"), ("G.TC", 1, "a"), ("C..GG", 0, "m"), ("A" + "." * 40 + "C", 0, "a"), ("A" + "." * 70 + "T", 0, "a")):
            s_loop, t_loop = context_by_loops(seqs[name], classes.calls[(mt, name)], CANONICAL[mt], m, i, 31)
            s_vec, t_vec = context_of([name], mt, m, i, 31)
            assert np.array_equal(s_loop, s_vec) and np.array_equal(t_loop, t_vec), (name, m)
    assert context_of(["edge"], "a", "GATC", 1, 31)[0].sum() > 40


# ------------------------------------------------------------------------------------------------ the definition
def test_rows_sum_to_the_states_and_radius_10_is_the_middle():
    names, _, bins, _, _, _ = profile_input()
    contigs = bin_contigs_of(names, bins)
    for (b, mt, m, i), (states, table) in zip(profile_cands(), context_expected()):
        assert states.sum() > 0, (b, m)
        assert np.array_equal(table.sum(axis=-1), np.broadcast_to(states[None], table.shape[:-1])), (b, m)
    for k in (0, 5, 16):
        b, mt, m, i = profile_cands()[k]
        s10, t10 = context_of(contigs[b], mt, m, i, 10)
        assert np.array_equal(s10, context_expected()[k][0]) and np.array_equal(t10, middle(context_expected()[k][1], 10))


REFINEMENTS = [("GATC", 1, "a", (-1, 0, 1, 2)),                         # inside the motif: one letter holds everything, the others nothing
               ("..GATC.", 3, "a", (-3, -2, 3)),                        # `.` positions of the motif
               ("C..GG", 0, "m", (1, 2)),
               ("G[AG]TC", 1, "a", (0,)),                               # an IUPAC set at the modified base
               ("GATC", 1, "a", (-31, -3, -2, 3, 4, 31)),               # outside, both sides
               ("A" + "." * 40 + "C", 0, "a", (-2, 20, 31))]


def test_a_cell_is_the_refined_motif_on_its_own():
    """The cell (o, X) equals the state counts of the motif narrowed to X at o, computed by ``occurrences`` on that motif alone."""
    names, _, bins, _, _, _ = profile_input()
    contigs = bin_contigs_of(names, bins)
    cands, exp = profile_cands(), context_expected()
    checked = excluded = 0
    for m, i, mt, offsets in REFINEMENTS:
        table = exp[cands.index(("b1", mt, m, i))][1]
        for o in offsets:
            for x, letter in enumerate(LETTERS):
                fine = narrowed(m, i, o, letter)
                if fine is None:
                    assert not table[o + 31, :, :, x].any(), (m, o, letter)
                    excluded += 1
                    continue
                states, _ = context_of(contigs["b1"], mt, fine[0], fine[1], 0)
                assert np.array_equal(states, table[o + 31, :, :, x]), (m, o, letter)
                checked += int(states.sum() > 0)
    assert checked >= 60 and excluded >= 12


def test_the_reverse_complement_candidate_is_the_mirror():
    """The reverse-complement candidate (the motif's reverse complement, its modified base at the same duplex position) occurs on '-'
    wherever the candidate occurs on '+' and the other way round, with the same own coordinate p.  Its state is read on the other
    strand, so states do not carry over; pooled over the states, its cell (o, s, X) is the candidate's (-o, 1 - s, complement of X):
    the probe p + o of a '+' occurrence is the probe p - (-o) of the '-' occurrence at p, read on the other strand.  `other` maps to
    itself."""
    from oracle.motif import Motif as OMotif
    names, _, bins, _, _, _ = profile_input()
    contigs = bin_contigs_of(names, bins)
    cands, exp = profile_cands(), context_expected()
    comp = [3, 2, 1, 0, 4]
    for m, i, mt in (("GATC", 1, "a"), ("AATT", 0, "a"), ("G[AG]TC", 1, "a"), ("C..GG", 0, "m"), ("A" + "." * 40 + "C", 0, "a")):
        rc = OMotif(m, i).reverse_compliment()
        states, table = exp[cands.index(("b1", mt, m, i))]
        s_rc, t_rc = context_of(contigs["b1"], mt, rc.string, rc.mod_position, 31)
        assert np.array_equal(s_rc.sum(axis=1), states.sum(axis=1)[::-1]), m
        assert np.array_equal(t_rc.sum(axis=2), table.sum(axis=2)[::-1, ::-1][..., comp]), m
        assert not np.array_equal(t_rc.sum(axis=2), table.sum(axis=2)), m
        assert not np.array_equal(t_rc.sum(axis=2), table.sum(axis=2)[::-1, ::-1]), m          # letters are complemented, not kept
        assert not np.array_equal(t_rc.sum(axis=2), table.sum(axis=2)[:, ::-1][..., comp]), m  # offsets change sign


# ------------------------------------------------------------------------------------------------ gain, keep, flag
def _table(radius, per_offset, default):
    """int64[W, 2, 3, 5] with ``per_offset`` = {offset: {letter or "other": (mod, nomod, nocall)}} on the '+' occurrences (nothing on
    '-'), ``default`` for the offsets not named."""
    t = np.zeros((2 * radius + 1, 2, 3, 5), dtype=np.int64)
    for o in range(-radius, radius + 1):
        for letter, three in per_offset.get(o, default).items():
            t[o + radius, 0, :, 4 if letter == "other" else LETTERS.index(letter)] = three
    return t


def _cand(bin, motif, mod_type, pos):
    from nanomotif_amd.motif_sites import SiteCandidate
    return SiteCandidate(bin, motif, mod_type, pos)


def _files(cands, tables, bg_keys=(), bg_tables=(), **kw):
    from nanomotif_amd.motif_context import format_files
    out = []
    for text in format_files(cands, tables, list(bg_keys), list(bg_tables), **kw):
        lines = text.split("\n")
        assert lines[-1] == ""
        out.append([line.split("\t") for line in lines[:-1]])
    return out


GATC_FIXED = {-1: {"G": (190, 210, 40)}, 0: {"A": (190, 210, 40)}, 1: {"T": (190, 210, 40)}, 2: {"C": (190, 210, 40)}}
FLAT = {"A": (47, 52, 10), "C": (48, 53, 10), "G": (47, 52, 10), "T": (48, 53, 10)}


def test_gain_keep_and_flag_on_hand_made_tables():
    from nanomotif_amd.motif_context import SUMMARY_HEADER
    assert SUMMARY_HEADER == ["bin", "motif", "mod_type", "mod_position", "n_mod", "n_nomod", "n_nocall", "frac_mod", "best_offset", "best_gain", "keep",
                              "refined_motif", "refined_mod_position", "refined_n_mod", "refined_n_nomod", "refined_frac_mod", "kept_mod_share",
                              "dropped_called", "dropped_frac_mod", "flag"]
    cand = [_cand("b", "GATC", "a", 1)]
    summary = lambda per_offset, default=FLAT, **kw: _files(cand, [_table(3, {**GATC_FIXED, **per_offset}, default)], **kw)[2][1][4:]
    # RGATCY planted in GATC: R before the G separates best, Y behind the C a little less
    planted = {-2: {"A": (90, 10, 10), "C": (5, 95, 10), "G": (90, 10, 10), "T": (5, 95, 10)},
               3: {"A": (10, 90, 10), "C": (85, 15, 10), "G": (10, 90, 10), "T": (85, 15, 10)}}
    # gain(-2) = 2 ll(90, 100) + 2 ll(5, 100) - ll(190, 400) = 2 (-32.5083) + 2 (-19.8515) - (-276.7587) = 172.0390
    assert summary(planted) == ["190", "210", "40", "0.475000", "-2", "172.039", "AG", "RGATC", "2", "180", "20", "0.900000", "0.947368", "200", "0.050000",
                                "underspecified"]
    # the same split below --min_gain, and with fewer dropped sites than --min_called: not flagged
    assert summary(planted, min_gain=172.1)[-1] == "none" and summary(planted, min_called=201)[-1] == "none"
    assert summary(planted, min_gain=172.0, min_called=200)[-1] == "underspecified"
    # uniform: nothing separates; the best offset is whichever flat offset comes first under the tie rule (-2 before 3, |o| = 2 before 3)
    assert summary({}) == ["190", "210", "40", "0.475000", "-2", "0.000", "CT", "YGATC", "2", "96", "106", "0.475248", "0.505263", "198", "0.474747", "none"]
    # too few called sites
    few = {o: {k: (3, 2, 40)} for o, d in GATC_FIXED.items() for k in d}
    assert summary({**few, -2: {"A": (3, 0, 20), "C": (0, 2, 20)}}, default={"A": (2, 1, 20), "C": (1, 1, 20)}) == \
        ["3", "2", "40", "0.600000", "-2", "3.365", "A", "AGATC", "2", "3", "0", "1.000000", "1.000000", "2", "0.000000", "few_sites"]
    # a tie between -2 and +2 (radius 2 around the one-letter candidate A): negative before positive; between -1 and the pair: smallest |o|
    one = [_cand("b", "A", "a", 0)]
    split = {"A": (90, 10, 0), "C": (5, 95, 0), "G": (90, 10, 0), "T": (5, 95, 0)}
    own = {0: {"A": (190, 210, 0)}}
    row = lambda per_offset: _files(one, [_table(2, {**own, **per_offset}, FLAT)])[2][1][4:]
    assert row({-2: split, 2: split}) == ["190", "210", "0", "0.475000", "-2", "172.039", "AG", "RNA", "2", "180", "20", "0.900000", "0.947368", "200", "0.050000",
                                          "underspecified"]
    assert row({2: split})[4:9] == ["2", "172.039", "AG", "ANR", "0"]
    assert row({-2: split, 2: split, 1: split})[4:9] == ["1", "172.039", "AG", "AR", "0"]
    assert row({-2: split, 2: split, 1: split, -1: split})[4:9] == ["-1", "172.039", "AG", "RA", "1"]
    # the sites whose probe has no letter are a fifth group: they separate, and they are dropped
    edge = {-2: {"A": (95, 5, 0), "other": (95, 205, 0)}}
    assert row(edge)[4:] == ["-2", "69.608", "A", "ANA", "2", "95", "5", "0.950000", "0.500000", "300", "0.316667", "underspecified"]
    # a candidate without a called site: no letter is kept, nothing is refined
    none = _files(one, [_table(1, {}, {"A": (0, 0, 7), "T": (0, 0, 3)})])[2][1][4:]
    assert none == ["0", "0", "10", "", "0", "0.000", "", "", "", "0", "0", "", "", "0", "", "few_sites"]


def test_rows_of_the_three_files():
    from nanomotif_amd.motif_context import MAIN_HEADER
    assert MAIN_HEADER == ["bin", "motif", "mod_type", "mod_position", "offset", "letter", "n_mod", "n_nomod", "n_nocall", "frac_mod", "share_mod", "share_nomod",
                           "refined_motif", "refined_mod_position"]
    t = _table(1, {-1: {"A": (6, 2, 1), "G": (0, 0, 1), "T": (2, 6, 0), "other": (0, 0, 1)}, 0: {"A": (8, 8, 3)}, 1: {"C": (4, 4, 3), "T": (4, 4, 0)}}, {})
    t[:, 1] = t[:, 0]                                                    # the same again on '-': the files pool the two strands
    bg = _table(1, {0: {"C": (1, 3, 0)}}, {"A": (1, 0, 0), "G": (0, 3, 0)})
    main, bins_file, summary = _files([_cand("b1", "RA", "a", 1)], [t], [("b1", "m")], [bg], min_called=16, min_gain=3.0)
    assert main[0] == MAIN_HEADER and bins_file[0] == MAIN_HEADER
    key = ["b1", "RA", "a", "1"]
    assert main[1:] == [key + ["-1", "A", "12", "4", "2", "0.750000", "0.750000", "0.250000", "AA", "1"],
                        key + ["-1", "C", "0", "0", "0", "", "0.000000", "0.000000", "", ""],            # R excludes C
                        key + ["-1", "G", "0", "0", "2", "", "0.000000", "0.000000", "GA", "1"],
                        key + ["-1", "T", "4", "12", "0", "0.250000", "0.250000", "0.750000", "", ""],   # (not a possible table: R excludes T too)
                        key + ["0", "A", "16", "16", "6", "0.500000", "1.000000", "1.000000", "RA", "1"],
                        key + ["0", "C", "0", "0", "0", "", "0.000000", "0.000000", "", ""],
                        key + ["0", "G", "0", "0", "0", "", "0.000000", "0.000000", "", ""],
                        key + ["0", "T", "0", "0", "0", "", "0.000000", "0.000000", "", ""],
                        key + ["1", "A", "0", "0", "0", "", "0.000000", "0.000000", "RAA", "1"],
                        key + ["1", "C", "8", "8", "6", "0.500000", "0.500000", "0.500000", "RAC", "1"],
                        key + ["1", "G", "0", "0", "0", "", "0.000000", "0.000000", "RAG", "1"],
                        key + ["1", "T", "8", "8", "0", "0.500000", "0.500000", "0.500000", "RAT", "1"]]
    assert summary[1] == key + ["16", "16", "6", "0.500000", "-1", "4.186", "A", "AA", "1", "12", "4", "0.750000", "0.750000", "16", "0.250000", "underspecified"]
    bkey = ["b1", "C", "m", "0"]
    assert [r[:6] for r in bins_file[1:]] == [bkey + [str(o), x] for o in (-1, 0, 1) for x in LETTERS]
    assert bins_file[1] == bkey + ["-1", "A", "1", "0", "0", "1.000000", "1.000000", "0.000000", "AC", "1"]
    assert bins_file[6] == bkey + ["0", "C", "1", "3", "0", "0.250000", "1.000000", "1.000000", "C", "0"]
    assert bins_file[11] == bkey + ["1", "G", "0", "3", "0", "0.000000", "0.000000", "1.000000", "CG", "0"]


def test_refined_names_the_motif_of_the_cell():
    from nanomotif_amd.motif_context import refined
    assert refined("GATC", 1, -3, "A") == ("ANGATC", 3) and refined("GATC", 1, 2, "C") == ("GATC", 1) and refined("GATC", 1, 2, "A") == ("", "")
    assert refined("GATC", 1, -2, "AG") == ("RGATC", 2) and refined("GATC", 1, 4, "CT") == ("GATCNY", 1) and refined("GATC", 1, 3, "ACGT") == ("GATC", 1)
    assert refined("GRTC", 1, 0, "A") == ("GATC", 1) and refined("GRTC", 1, 0, "AC") == ("GATC", 1) and refined("GRTC", 1, 0, "CT") == ("", "")
    assert refined("CNNGG", 0, 1, "T") == ("CTNGG", 0) and refined("GATC", 1, 0, "") == ("", "")
    # the reach limit [-96, 95] and the length limit 191 of the engine
    assert refined("A", 0, 95, "C") == ("A" + "N" * 94 + "C", 0) and refined("A", 0, -96, "C") == ("C" + "N" * 95 + "A", 96)
    long = "A" + "N" * 70 + "T"
    assert refined(long, 0, -31, "G") == ("G" + "N" * 30 + long, 31) and refined(long, 71, 31, "G") == (long + "N" * 30 + "G", 71)
    assert refined("A" + "N" * 93 + "C", 0, -96, "G") == ("G" + "N" * 95 + "A" + "N" * 93 + "C", 96)   # 191 letters
    assert refined("A" + "N" * 94 + "C", 0, -96, "G") == ("", "") and refined("A" + "N" * 94 + "C", 0, 96, "G") == ("", "") and refined("A", 0, -97, "G") == ("", "")


# ------------------------------------------------------------------------------------------------ the parser, the engine, the exports
def test_parser_accepts_motif_context(capsys):
    p = create_parser()
    a = p.parse_args(["motif_context", "asm.fasta", "p.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "cx"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.out, a.bin_motifs) == ("motif_context", "asm.fasta", "p.bed", "contig_bin.tsv", "cx", ["out/bin-motifs.tsv"])
    assert (a.radius, a.min_called, a.min_gain) == (10, 20, 30.0)
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose, a.threads) == (0.3, 0.7, 5, None, False, 1)
    a = p.parse_args(["motif_context", "asm.fasta", "p.bed.gz", "-d", "bins", "--bin_motifs", "a.tsv", "b.tsv", "--radius", "31", "--min_called", "5", "--min_gain", "12.5",
                      "--device", "1", "-v", "-t", "4"])
    assert (a.radius, a.min_called, a.min_gain, a.bin_motifs, a.device) == (31, 5, 12.5, ["a.tsv", "b.tsv"], 1)
    assert p.parse_args(["motif_context", "a", "p", "-c", "c", "--bin_motifs", "b.tsv", "--radius", "0"]).radius == 0
    for flag, bad in (("--radius", "32"), ("--radius", "-1"), ("--radius", "x")):
        with pytest.raises(SystemExit):
            p.parse_args(["motif_context", "asm.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "b.tsv", flag, bad])
        assert flag in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["motif_context", "asm.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs"])          # an empty list
    assert "--bin_motifs" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["motif_context", "asm.fasta", "p.bed", "-c", "cb.tsv"])
    capsys.readouterr()
    assert "motif_context" in p.format_help()


def test_engine_refuses_a_radius_outside_the_range_before_it_needs_a_device():
    from nanomotif_amd.engine import CONTEXT_LETTERS, CONTEXT_MAX_RADIUS, ScanEngine
    assert CONTEXT_MAX_RADIUS == 31 and CONTEXT_LETTERS == ("A", "C", "G", "T", "other")
    eng = ScanEngine.__new__(ScanEngine)                                # no context: the check comes first
    for bad in (-1, 32, 100):
        with pytest.raises(ValueError) as e:
            ScanEngine.motif_context(eng, [], radius=bad)
        assert "radius" in str(e.value)
    eng.ctx = None                                                      # (nothing for __del__ to destroy)


def test_exports_are_declared_bound_and_built():
    from nanomotif_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    assert "int nm_motif_context_count(" in header and "nm_motif_context_count" in _lib.SYMBOLS
    assert "#define NM_CONTEXT_MAX_RADIUS 31" in header
    assert any(os.path.basename(s) == "nmcontext.hip" for s in build.SRC_HIP)
    lib = _lib.load()
    assert lib.nm_abi_version() == 1
    q = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    bins, slots, lens, modpos, off, masks = np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.array([1], np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint32), np.array([1], np.uint8)
    states, counts = np.zeros(6, np.uint64), np.zeros(63 * 24, np.int64)
    cand = (q(bins, C.c_uint32), q(slots, C.c_uint8), q(lens, C.c_uint8), q(modpos, C.c_uint8), q(off, C.c_uint32), q(masks, C.c_uint8))
    out = (q(states, C.c_uint64), q(counts, C.c_int64))
    call = lambda cand=cand, radius=10, out=out: lib.nm_motif_context_count(None, 1, *cand, radius, *out)
    # refused with a NULL ctx, before any device call, and by name
    nulls = [dict(cand=cand[:j] + (None,) + cand[j + 1:]) for j in range(6)] + [dict(out=(None, out[1])), dict(out=(out[0], None))]
    for kw, word in [(kw, "NULL") for kw in nulls] + [(dict(radius=32), "radius"), (dict(radius=1 << 31), "radius"), (dict(), "ctx")]:
        assert call(**kw) == -1, kw                                     # NM_EINVAL
        assert word in lib.nm_last_error().decode(), (kw, lib.nm_last_error())
    assert lib.nm_motif_context_count(None, 0, None, None, None, None, None, None, 10, None, None) == -1      # n_cand = 0 still needs a ctx
    assert lib.nm_motif_context_count(None, 0, None, None, None, None, None, None, 32, None, None) == -1 and b"radius" in lib.nm_last_error()
