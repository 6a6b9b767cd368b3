"""Host side of ``nanomotif motif_profile`` (no GPU): the brute force both suites compare against — built only from
``oracle.scan.subseq_indices``, ``oracle.scan.split_positions`` (through ``test_gpu_motif_compare.oracle_calls``) and ``oracle.motif.Motif`` —
the conditions on the geometry input it runs on, the two identities that fix the orientation, ``--targets`` / ``--radius``, the three
files on hand-written tables, and the exports in the header and the binding.

The brute force is the definition: ``probe_class`` classifies one (position, strand) under one target with plain set look-ups, and
``profile_by_loops`` walks occurrences, offsets, strands and targets one by one.  ``profile_of`` is the same walk with the innermost loop
(over the occurrences of one contig and strand) taken as one numpy index into the per-position classes ``probe_class`` gave; the two are
compared on whole candidates below."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from nanomotif_amd.argparser import create_parser
from test_gpu_motif_compare import Expected as CompareExpected
from test_gpu_motif_compare import oracle_calls, reach_class
from test_motif_strands_host import Expected as StrandsExpected
from test_motif_strands_host import geometry_input, offset_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192
CLASSES = ("mod", "nomod", "nocall", "other")
CANONICAL = {"a": "A", "m": "C", "21839": "C"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
TARGETS = ("a", "m")                                                    # slot order of the geometry engine: "a" is uploaded first
M_SEED = 2111


# ------------------------------------------------------------------------------------------------ the brute force
def occurrences(seq, motif, i):
    """[(own position p, occurrence strand s)]: the stripped motif on '+', its reverse complement on '-'."""
    from oracle.motif import Motif as OMotif
    from oracle.scan import subseq_indices
    st = OMotif(motif, i).new_stripped_motif()
    rc = st.reverse_compliment()
    return [(int(p), 0) for p in subseq_indices(st.string, seq) + st.mod_position] + [(int(p), 1) for p in subseq_indices(rc.string, seq) + rc.mod_position]


def probe_class(seq, calls, base, q, strand):
    """The class 0 mod / 1 nomod / 2 nocall / 3 other of (q, strand) under a target with the calls (M, U) and canonical base ``base``."""
    if (q, strand) in calls[0]:
        return 0
    if (q, strand) in calls[1]:                                         # (oracle_calls has taken M out of U)
        return 1
    if 0 <= q < len(seq):
        letter = seq[q] if strand == 0 else COMPLEMENT.get(seq[q])
        if letter == base:
            return 2
    return 3


def profile_by_loops(seq, motif, i, calls_of_target, bases, radius):
    """(sites[2], table[n_targets][2 R + 1][2][2][4]) of one candidate on one contig, one probe at a time."""
    sites = np.zeros(2, dtype=np.int64)
    table = np.zeros((len(bases), 2 * radius + 1, 2, 2, 4), dtype=np.int64)
    for p, s in occurrences(seq, motif, i):
        sites[s] += 1
        for o in range(-radius, radius + 1):
            q = p + o if s == 0 else p - o
            for r in (0, 1):
                for t, base in enumerate(bases):
                    table[t, o + radius, s, r, probe_class(seq, calls_of_target[t], base, q, s ^ r)] += 1
    return sites, table


class Classes:
    """Per (target, contig): ``probe_class`` of every (position, strand), radius 31 positions of ``other`` either side."""
    PAD = 31

    def __init__(self, seqs, piles, targets, low=0.3, high=0.7):
        from oracle.scan import _EMPTY
        self.seqs, self.targets = seqs, tuple(targets)
        self.calls, self.cls = {}, {}
        for t in self.targets:
            for name, seq in seqs.items():
                calls = oracle_calls(piles[t].get(name, _EMPTY), low, high)
                self.calls[(t, name)] = calls
                a = np.full((2, len(seq) + 2 * self.PAD), 3, dtype=np.int8)
                for strand in (0, 1):
                    for q in range(len(seq)):
                        a[strand, q + self.PAD] = probe_class(seq, calls, CANONICAL[t], q, strand)
                self.cls[(t, name)] = a


def profile_of(classes: Classes, names, motif, i, radius):
    """(sites[2], table[n_targets][2 R + 1][2][2][4]) of one candidate summed over the contigs ``names``."""
    assert radius <= Classes.PAD
    sites = np.zeros(2, dtype=np.int64)
    table = np.zeros((len(classes.targets), 2 * radius + 1, 2, 2, 4), dtype=np.int64)
    for name in names:
        occ = occurrences(classes.seqs[name], motif, i)
        for s in (0, 1):
            own = np.array([p for p, st in occ if st == s], dtype=np.int64)
            sites[s] += len(own)
            for o in range(-radius, radius + 1):
                q = own + o if s == 0 else own - o
                for r in (0, 1):
                    for t, target in enumerate(classes.targets):
                        table[t, o + radius, s, r] += np.bincount(classes.cls[(target, name)][s ^ r, q + Classes.PAD], minlength=4)
    return sites, table


# ------------------------------------------------------------------------------------------------ the input (shared with the GPU suite)
# (motif, mod position, own mod type); G.TC leaves the modified base open: the only candidates whose own base can be the T / G that a
# probe at (opposite, 0) needs for a nocall
PROFILE_MOTIFS = [("GATC", 1, "a"), ("A", 0, "a"), ("AATT", 0, "a"), ("G[AG]TC", 1, "a"), ("..GATC.", 3, "a"), ("A" + "." * 40 + "C", 0, "a"),
                  ("A" + "." * 70 + "T", 0, "a"), ("C..GG", 0, "m"), ("G.TC", 1, "a")]
OPEN_MODIFIED_BASE = [("G[AG]TC", 1), ("G.TC", 1)]                     # the motif does not fix the modified base to the canonical letter
# the candidates that have a partner (motif, i, j): the letter at j of the reverse complement is the canonical base, |d| <= 31
PARTNERS = [("GATC", 1, 1), ("A", 0, 0), ("AATT", 0, 0), ("G[AG]TC", 1, 1), ("..GATC.", 3, 2), ("A" + "." * 40 + "C", 0, 20), ("C..GG", 0, 0), ("C..GG", 0, 1)]


@functools.lru_cache(maxsize=None)
def profile_input():
    """(names, seqs, bins, bin_names, {"a": rows, "m": rows}, piles): the sequences, bins and "a" pileup of
    ``test_motif_strands_host.geometry_input`` plus an independently drawn "m" pileup of the same row model.  One plant of our own on the
    30 kbp contig: GATC with its A ON the first position of a chunk (16 384), which the offsets below 0 need to leave the chunk — the
    geometry input has its A on the last position of one (8 191), which serves the offsets above 0."""
    from oracle.scan import ContigPileup
    names, seqs, bins, bin_names, rows_a, piles_a = geometry_input()
    seqs = dict(seqs)
    big = list(seqs["big"])
    big[16383:16387] = "GATC"
    seqs["big"] = "".join(big)
    rng = np.random.default_rng(M_SEED)
    cid, pos, st, fr, piles_m = [], [], [], [], {}
    for c, n in enumerate(names):
        L = len(seqs[n])
        p, s = np.nonzero(rng.random((L, 2)) < 0.6)
        strand = np.where(s == 0, ord("+"), ord("-")).astype(np.uint8)
        f = rng.choice([0.0, 0.3, 0.5, 0.7, 1.0], size=len(p))
        piles_m[n] = ContigPileup(p.astype(np.int64), strand, f)
        cid.append(np.full(len(p), c, np.uint32)); pos.append(p); st.append(strand); fr.append(f)
    rows_m = (np.concatenate(cid), np.concatenate(pos), np.concatenate(st), np.concatenate(fr))
    return names, seqs, bins, bin_names, {"a": rows_a, "m": rows_m}, {"a": piles_a["a"], "m": piles_m}


def profile_cands():
    """[(bin, own mod type, motif, mod position)]: every motif in both non-empty bins."""
    return [(b, mt, m, i) for b in ("b1", "b2") for m, i, mt in PROFILE_MOTIFS]


def bin_contigs_of(names, bins):
    return {b: [n for n in names if bins[n] == b] for b in ("b0_empty", "b1", "b2")}


@functools.lru_cache(maxsize=None)
def profile_classes():
    names, seqs, bins, _, _, piles = profile_input()
    return Classes(seqs, piles, TARGETS)


@functools.lru_cache(maxsize=None)
def profile_expected():
    """Per candidate of ``profile_cands`` (sites, table) at radius 31; smaller radii are its middle slices by definition."""
    names, seqs, bins, _, _, _ = profile_input()
    contigs = bin_contigs_of(names, bins)
    return [profile_of(profile_classes(), contigs[b], m, i, 31) for b, _, m, i in profile_cands()]


def middle(table, radius, axis=1):
    """The offsets -radius .. radius of a table that holds -31 .. 31 on ``axis``."""
    return np.take(table, range(31 - radius, 31 + radius + 1), axis=axis)


# ------------------------------------------------------------------------------------------------ non-degeneracy, on the brute force alone
def test_the_input_is_not_degenerate():
    names, seqs, bins, _, _, piles = profile_input()
    assert sorted(len(s) for s in seqs.values())[-4:] == [320, CHUNK, 9_000, 30_000]
    assert {reach_class(m, i) for m, i, _ in PROFILE_MOTIFS} == {0, 1, 2}
    cands, exp = profile_cands(), profile_expected()
    total = sum(t for _, t in exp)                                      # [target][offset][s][r][class]
    by_cell = total.sum(axis=2)                                         # [target][offset][r][class]
    print("min over the 63 offsets, [target][r][class]:", by_cell.min(axis=1).tolist())
    for c in (0, 1, 3):
        assert (by_cell[..., c] > 100).all(), (CLASSES[c], by_cell[..., c].min(axis=1).tolist())
    assert (by_cell[..., 2] > 0).all(), by_cell[..., 2].min(axis=1).tolist()
    # GATC @ 1 on the 30 kbp contig: own base and probe in different chunks, lanes and words at the four offsets
    classes = profile_classes()
    occ = occurrences(seqs["big"], "GATC", 1)
    assert {(8191, 0), (8192, 1), (16384, 0), (9631, 0), (10239, 0)} <= set(occ)
    for o in (-31, -1, 1, 31):
        pairs = [(p, p + o if s == 0 else p - o) for p, s in occ]
        for unit in (CHUNK, 128, 32):
            assert any(p // unit != q // unit for p, q in pairs), (o, unit)
    # probes before position 0 and at or past the end, both occurrence strands, all of them `other` under both targets
    for name in ("edge", "mid"):
        seq = seqs[name]
        seen = set()
        for m, i in (("GATC", 1),):
            for p, s in occurrences(seq, m, i):
                for o in range(-31, 32):
                    q = p + o if s == 0 else p - o
                    if q < 0 or q >= len(seq):
                        seen.add((s, q < 0))
                        for t in TARGETS:
                            for strand in (0, 1):
                                assert probe_class(seq, classes.calls[(t, name)], CANONICAL[t], q, strand) == 3
        if name == "edge":
            assert seen == {(0, True), (0, False), (1, True), (1, False)}
        else:
            assert {(0, False), (1, False)} <= seen


def test_the_vectorised_walk_is_the_loop():
    """``profile_of`` against ``profile_by_loops`` on whole candidates: the contigs with sites at both ends, back-to-back sites and
    the ones shorter than the motif, all widths of the motif that fit them."""
    names, seqs, bins, _, _, _ = profile_input()
    classes = profile_classes()
    for name in ("edge", "small", "tiny1", "tiny2", "tiny3"):
        for m, i in (("GATC", 1), ("AATT", 0), ("G.TC", 1), ("C..GG", 0), ("A" + "." * 40 + "C", 0), ("A" + "." * 70 + "T", 0)):
            calls = [classes.calls[(t, name)] for t in TARGETS]
            s_loop, t_loop = profile_by_loops(seqs[name], m, i, calls, [CANONICAL[t] for t in TARGETS], 31)
            s_vec, t_vec = profile_of(classes, [name], m, i, 31)
            assert np.array_equal(s_loop, s_vec) and np.array_equal(t_loop, t_vec), (name, m)
    assert profile_of(classes, ["edge"], "GATC", 1, 31)[0].sum() > 40


# ------------------------------------------------------------------------------------------------ the definition
def test_classes_sum_to_the_sites():
    for (b, mt, m, i), (sites, table) in zip(profile_cands(), profile_expected()):
        assert sites.sum() > 0, (b, m)
        assert np.array_equal(table.sum(axis=-1), np.broadcast_to(sites[None, None, :, None], table.shape[:-1])), (b, m)


def test_identities_hold_in_the_brute_force():
    """(o = 0, r = 0) under the own target is the row of ``motif_site_counts`` (the diagonal of the compare brute force of a sample with
    itself; where the motif leaves the modified base open, its no-call column is nocall + other); (o = d, r = 1) gives the partner marginals of the strands brute force."""
    names, seqs, bins, _, _, piles = profile_input()
    contigs = bin_contigs_of(names, bins)
    index = {n: k for k, n in enumerate(names)}
    cands, exp = profile_cands(), profile_expected()
    own = CompareExpected([(b, mt, m, i) for b, mt, m, i in cands], contigs, index, seqs, piles, piles)
    for (b, mt, m, i), (sites, table), t18 in zip(cands, exp, own.tables):
        six = t18.sum(axis=0).reshape(2, 3, 3).diagonal(axis1=1, axis2=2)                                  # [s][state]
        cell = table[TARGETS.index(mt), 31, :, 0]
        assert np.array_equal(sites, six.sum(axis=1)), (b, m)
        if (m, i) in OPEN_MODIFIED_BASE:                                # the own letter may be another than the canonical one: no call there is `other`
            assert np.array_equal(cell[:, :2], six[:, :2]) and np.array_equal(cell[:, 2] + cell[:, 3], six[:, 2]) and cell[:, 3].sum() > 0, (b, m)
        else:
            assert np.array_equal(cell[:, :3], six) and not cell[:, 3].any(), (b, m)
    checked = 0
    for b in ("b1", "b2"):
        for m, i, j in PARTNERS:
            mt = next(t for mm, ii, t in PROFILE_MOTIFS if (mm, ii) == (m, i))
            d = offset_of(m, i, j)
            assert abs(d) <= 31
            nine = StrandsExpected([(b, mt, m, i, j)], contigs, index, seqs, piles).tables[0].sum(axis=0).reshape(2, 3, 3)   # [s][own][partner]
            cell = exp[cands.index((b, mt, m, i))][1][TARGETS.index(mt), 31 + d, :, 1]                      # [s][class]
            marg = nine.sum(axis=1)
            assert np.array_equal(cell[:, :2], marg[:, :2]) and np.array_equal(cell[:, 2] + cell[:, 3], marg[:, 2]), (b, m, i, j)
            checked += int(marg.sum() > 0)
    assert checked >= 12


# ------------------------------------------------------------------------------------------------ --targets, --radius, the parser
def test_parse_targets_and_radius():
    from nanomotif_amd.motif_profile import parse_radius, parse_targets
    assert parse_targets("a,m,21839") == ("m", "a", "21839") and parse_targets(" a ") == ("a",) and parse_targets("21839,21839,m") == ("m", "21839")
    for bad in ("", ",", "a;m", "x", "a,5mC", "A"):
        with pytest.raises(ValueError) as e:
            parse_targets(bad)
        assert "--targets" in str(e.value)
    assert [parse_radius(x) for x in (0, "0", 10, " 31 ")] == [0, 0, 10, 31]
    for bad in (-1, 32, "32", "ten", "", "1.5", 1000):
        with pytest.raises(ValueError) as e:
            parse_radius(bad)
        assert "--radius" in str(e.value)


def test_parser_accepts_motif_profile(capsys):
    p = create_parser()
    a = p.parse_args(["motif_profile", "asm.fasta", "p.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "pr"])
    assert (a.command, a.assembly, a.pileup, a.contig_bin, a.out, a.bin_motifs) == ("motif_profile", "asm.fasta", "p.bed", "contig_bin.tsv", "pr", ["out/bin-motifs.tsv"])
    assert (a.radius, a.targets, a.min_called) == (10, None, 20)
    assert (a.methylation_threshold_low, a.methylation_threshold_high, a.threshold_valid_coverage, a.device, a.verbose, a.threads) == (0.3, 0.7, 5, None, False, 1)
    a = p.parse_args(["motif_profile", "asm.fasta", "p.bed.gz", "-d", "bins", "--bin_motifs", "a.tsv", "b.tsv", "--radius", "31", "--targets", "a, 21839",
                      "--min_called", "5", "--device", "1", "-v", "-t", "4"])
    assert (a.radius, a.targets, a.min_called, a.bin_motifs, a.device) == (31, ("a", "21839"), 5, ["a.tsv", "b.tsv"], 1)
    for flag, bad in (("--radius", "32"), ("--radius", "-1"), ("--radius", "x"), ("--targets", "q"), ("--targets", ","), ("--targets", "")):
        with pytest.raises(SystemExit):
            p.parse_args(["motif_profile", "asm.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "b.tsv", flag, bad])
        assert flag in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["motif_profile", "asm.fasta", "p.bed", "-c", "cb.tsv"])
    capsys.readouterr()
    assert "motif_profile" in p.format_help()


def test_engine_refuses_a_radius_outside_the_range_before_it_needs_a_device():
    from nanomotif_amd.engine import PROFILE_CLASSES, PROFILE_MAX_RADIUS, ScanEngine
    assert PROFILE_MAX_RADIUS == 31 and PROFILE_CLASSES == CLASSES
    eng = ScanEngine.__new__(ScanEngine)                                # no context: the checks come first
    eng.slot_of_mod = {"a": 0, "a@2": 0, "m": 1}
    for bad in (-1, 32, 100):
        with pytest.raises(ValueError) as e:
            ScanEngine.motif_profile(eng, [], radius=bad)
        assert "radius" in str(e.value)
    labels, slots = eng._profile_targets(None)
    assert labels == ["a", "m"] and slots.tolist() == [0, 1]
    labels, slots = eng._profile_targets(["m", 0, "a@2", 5])
    assert labels == ["m", "a", "a@2", "5"] and slots.tolist() == [1, 0, 0, 5]
    for bad in (["x"], []):
        with pytest.raises(ValueError):
            eng._profile_targets(bad)
    eng.ctx = None                                                      # (nothing for __del__ to destroy)


# ------------------------------------------------------------------------------------------------ the three files
def _table(n_targets, radius, cells):
    """int64[n_targets, W, 2, 2, 4] with ``cells`` = {(target, relative strand, offset): (mod, nomod, nocall, other)} on the '+' occurrences
    and a tenth of it (integer part) on the '-' ones."""
    t = np.zeros((n_targets, 2 * radius + 1, 2, 2, 4), dtype=np.int64)
    for (ti, r, o), four in cells.items():
        t[ti, o + radius, 0, r] = four
        t[ti, o + radius, 1, r] = [x // 10 for x in four]
    return t


def _cand(bin, motif, mod_type, pos):
    from nanomotif_amd.motif_sites import SiteCandidate
    return SiteCandidate(bin, motif, mod_type, pos)


def _files(cands, targets, tables, bg_keys, bg_tables, min_called=20, sites=None):
    from nanomotif_amd.motif_profile import format_files
    site = lambda ts: np.array([[int(t[0, 0, 0, 0].sum()), int(t[0, 0, 1, 0].sum())] for t in ts], dtype=np.int64).reshape(-1, 2)
    texts = format_files(cands, targets, site(tables) if sites is None else sites, tables, bg_keys, site(bg_tables), bg_tables, min_called)
    out = []
    for text in texts:
        lines = text.split("\n")
        assert lines[-1] == ""
        out.append([line.split("\t") for line in lines[:-1]])
    return out


def test_rows_fractions_and_background_blocks():
    from nanomotif_amd.motif_profile import MAIN_HEADER, SUMMARY_HEADER, background_keys
    assert MAIN_HEADER == ["bin", "motif", "mod_type", "mod_position", "target", "strand", "offset", "n_sites", "n_mod", "n_nomod", "n_nocall", "n_other",
                           "frac_mod", "bg_frac_mod"]
    assert SUMMARY_HEADER == ["bin", "motif", "mod_type", "mod_position", "own_frac_mod", "own_called", "best_target", "best_strand", "best_offset",
                              "best_frac_mod", "best_bg_frac_mod", "best_called", "flag"]
    targets = ["a", "m", "21839"]                                       # A, C, C
    assert background_keys(["b1", "b2"], targets) == [("b1", "A"), ("b1", "C"), ("b2", "A"), ("b2", "C")]
    assert background_keys(["b1"], ["m", "21839"]) == [("b1", "C")] and background_keys([], targets) == []
    R = 1
    every = lambda four: {(ti, r, o): four for ti in range(3) for r in (0, 1) for o in (-1, 0, 1)}
    t_gatc = _table(3, R, {**every((0, 0, 10, 30)), (0, 0, 0): (30, 10, 0, 0), (1, 1, 1): (0, 0, 0, 40), (2, 0, -1): (1, 2, 3, 34)})
    t_ccwgg = _table(3, R, every((10, 10, 10, 10)))
    cands = [_cand("b2", "GATC", "a", 1), _cand("b1", "CCWGG", "m", 1)]
    # four background blocks, told apart by their mod counts: b1/A 1, b1/C 2, b2/A 3, b2/C 4 of 10 called
    bg_keys = background_keys(["b1", "b2"], targets)
    bg_tables = [_table(3, R, every((k + 1, 9 - k, 5, 5))) for k in range(4)]
    main, bins_file, summary = _files(cands, targets, [t_gatc, t_ccwgg], bg_keys, bg_tables)
    assert main[0] == MAIN_HEADER and bins_file[0] == MAIN_HEADER and summary[0] == SUMMARY_HEADER
    # row order: candidates in file order, targets in slot order, same before opposite, ascending offset
    assert [r[:7] for r in main[1:]] == [[c.bin, c.motif, c.mod_type, str(c.mod_position), t, s, str(o)]
                                         for c in cands for t in targets for s in ("same", "opposite") for o in (-1, 0, 1)]
    row = {tuple(r[:7]): r for r in main[1:]}
    assert row[("b2", "GATC", "a", "1", "a", "same", "0")][7:] == ["44", "33", "11", "0", "0", "0.750000", "0.300000"]       # pooled over both strands
    assert row[("b2", "GATC", "a", "1", "m", "opposite", "1")][7:] == ["44", "0", "0", "0", "44", "", "0.400000"]           # nothing called: empty
    assert row[("b2", "GATC", "a", "1", "21839", "same", "-1")][7:] == ["44", "1", "2", "3", "37", "0.333333", "0.400000"]
    assert row[("b2", "GATC", "a", "1", "a", "same", "1")][7:] == ["44", "0", "0", "11", "33", "", "0.300000"]
    # the background comes from the block of the candidate's bin and the target's base
    assert {r[13] for r in main[1:] if r[0] == "b1" and r[4] == "a"} == {"0.100000"}
    assert {r[13] for r in main[1:] if r[0] == "b1" and r[4] in ("m", "21839")} == {"0.200000"}
    assert {r[13] for r in main[1:] if r[0] == "b2" and r[4] == "a"} == {"0.300000"}
    # the bins file: per block only the targets of its base, the target in the mod_type column, its own share as background
    assert [r[:7] for r in bins_file[1:]] == [[b, base, t, "0", t, s, str(o)] for b, base in bg_keys for t in targets if CANONICAL[t] == base
                                              for s in ("same", "opposite") for o in (-1, 0, 1)]
    assert all(r[12] == r[13] for r in bins_file[1:]) and bins_file[1][7:] == ["20", "1", "9", "5", "5", "0.100000", "0.100000"]
    # without a background block (a bin the background does not hold) the column is empty and no cell qualifies
    main, _, summary = _files([_cand("b9", "GATC", "a", 1)], targets, [t_gatc], bg_keys, bg_tables)
    assert {r[13] for r in main[1:]} == {""} and summary[1][4:] == ["0.750000", "44", "", "", "", "", "", "", "none"]


def test_flag_and_its_tie_rules():
    targets = ["a", "m"]
    R = 2
    cells = lambda four: {(ti, r, o): four for ti in range(2) for r in (0, 1) for o in range(-R, R + 1)}
    bg_keys = [("b", "A"), ("b", "C")]
    bg = [_table(2, R, cells((100, 900, 0, 0)))] * 2                   # 10 % everywhere
    flat = cells((110, 890, 0, 0))                                      # 11 %: excess 0.01
    own = {(0, 0, 0): (600, 400, 0, 0)}

    def summary_of(extra, mod_type="a", min_called=20):
        return _files([_cand("b", "GATC", mod_type, 1)], targets, [_table(2, R, {**flat, **own, **extra})], bg_keys, bg, min_called)[2][1][4:]
    # a neighbour on the same strand that exceeds the own share: shifted
    assert summary_of({(0, 0, 1): (950, 50, 0, 0)}) == ["0.600000", "1100", "a", "same", "1", "0.950000", "0.100000", "1100", "shifted"]
    # ... that does not exceed it: best, but no flag
    assert summary_of({(0, 0, 1): (500, 500, 0, 0)}) == ["0.600000", "1100", "a", "same", "1", "0.500000", "0.100000", "1100", "none"]
    # the other mod type at the own position
    assert summary_of({(1, 0, 0): (900, 100, 0, 0)}) == ["0.600000", "1100", "m", "same", "0", "0.900000", "0.100000", "1100", "other_mod_type"]
    # the opposite strand, or another target off the centre: never a flag
    assert summary_of({(0, 1, 1): (990, 10, 0, 0)})[-3:] == ["0.100000", "1100", "none"] and summary_of({(0, 1, 1): (990, 10, 0, 0)})[2:5] == ["a", "opposite", "1"]
    assert summary_of({(1, 0, 1): (990, 10, 0, 0)})[2:5] == ["m", "same", "1"] and summary_of({(1, 0, 1): (990, 10, 0, 0)})[-1] == "none"
    # the own cell is never the best cell, however high
    assert summary_of({(0, 0, 0): (1000, 0, 0, 0)})[2:5] == ["a", "same", "-1"]
    # ties, all at 95 %: lowest target, same before opposite, smallest |offset|, negative before positive
    tie = (950, 50, 0, 0)
    assert summary_of({(1, 0, 0): tie, (0, 1, 2): tie})[2:5] == ["a", "opposite", "2"]
    assert summary_of({(0, 1, 0): tie, (0, 0, 2): tie})[2:5] == ["a", "same", "2"]
    assert summary_of({(0, 0, 2): tie, (0, 0, -1): tie, (0, 0, 1): tie})[2:5] == ["a", "same", "-1"]
    assert summary_of({(0, 0, 2): tie, (0, 0, -2): tie})[2:5] == ["a", "same", "-2"]
    assert summary_of({})[2:5] == ["a", "same", "-1"]                   # everything ties at 11 %
    # --min_called: a cell with 109 called sites (95 + 5, and 9 + 0 on '-') qualifies at 109 and not at 110
    assert summary_of({(0, 0, 1): (95, 5, 0, 0)}, min_called=110)[2:5] == ["a", "same", "-1"]
    assert summary_of({(0, 0, 1): (95, 5, 0, 0)}, min_called=109)[2:5] == ["a", "same", "1"]
    assert summary_of({}, min_called=5000)[2:] == ["", "", "", "", "", "", "none"]
    # a candidate whose mod type is not a target: own columns empty, a best cell, no flag
    assert summary_of({(0, 0, 1): tie}, mod_type="21839") == ["", "", "a", "same", "1", "0.950000", "0.100000", "1100", "none"]
    # an own cell without a called site is exceeded by any
    own[(0, 0, 0)] = (0, 0, 700, 300)
    assert summary_of({(0, 0, 1): tie}) == ["", "0", "a", "same", "1", "0.950000", "0.100000", "1100", "shifted"]


# ------------------------------------------------------------------------------------------------ exports
def test_exports_are_declared_bound_and_built():
    from nanomotif_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nmscan.h")).read()
    assert "int nm_motif_profile_count(" in header and "nm_motif_profile_count" in _lib.SYMBOLS
    assert "#define NM_PROFILE_MAX_RADIUS 31" in header
    assert any(os.path.basename(s) == "nmprofile.hip" for s in build.SRC_HIP)
    lib = _lib.load()
    assert lib.nm_abi_version() == 1
    q = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    bins, lens, modpos, off, masks = np.zeros(1, np.uint32), np.array([1], np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint32), np.array([1], np.uint8)
    slots, sites, counts = np.zeros(9, np.uint8), np.zeros(2, np.uint64), np.zeros(9 * 63 * 12, np.int64)
    cand = (q(bins, C.c_uint32), q(lens, C.c_uint8), q(modpos, C.c_uint8), q(off, C.c_uint32), q(masks, C.c_uint8))
    out = (q(sites, C.c_uint64), q(counts, C.c_int64))
    call = lambda cand=cand, nt=1, slots=q(slots, C.c_uint8), radius=10, out=out: lib.nm_motif_profile_count(None, 1, *cand, nt, slots, radius, *out)
    # refused with a NULL ctx, before any device call, and by name
    for kw, word in ((dict(cand=(None,) * 5), "NULL"), (dict(slots=None), "NULL"), (dict(out=(None, None)), "NULL"), (dict(out=(out[0], None)), "NULL"),
                     (dict(cand=cand[:2] + (None,) + cand[3:]), "NULL"), (dict(radius=32), "radius"), (dict(radius=1 << 31), "radius"),
                     (dict(nt=0), "n_targets"), (dict(nt=9), "n_targets"), (dict(), "ctx")):
        assert call(**kw) == -1, kw                                     # NM_EINVAL
        assert word in lib.nm_last_error().decode(), (kw, lib.nm_last_error())
    assert lib.nm_motif_profile_count(None, 0, None, None, None, None, None, 1, q(slots, C.c_uint8), 10, None, None) == -1      # n_cand = 0 still needs a ctx


def test_the_reverse_complement_candidate_is_the_mirror():
    """The occurrences of the reverse-complement candidate are the same duplex sites read from the other strand: the occurrence strands
    change places, offsets change sign, and `same` / `opposite` change places with the strand they are relative to."""
    from oracle.motif import Motif as OMotif
    names, seqs, bins, _, _, _ = profile_input()
    contigs = bin_contigs_of(names, bins)
    cands, exp = profile_cands(), profile_expected()
    for m, i in (("GATC", 1), ("AATT", 0), ("G[AG]TC", 1), ("C..GG", 0), ("A" + "." * 40 + "C", 0)):
        rc = OMotif(m, i).reverse_compliment()
        sites, table = exp[[c[2:] for c in cands].index((m, i))]
        s_rc, t_rc = profile_of(profile_classes(), contigs["b1"], rc.string, rc.mod_position, 31)
        assert np.array_equal(s_rc, sites[::-1]) and np.array_equal(t_rc, table[:, ::-1, ::-1, ::-1]), m
        assert not np.array_equal(t_rc, table[:, ::-1, ::-1]), m
