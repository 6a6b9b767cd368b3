"""GPU: the methylation profile around motif sites (nm_motif_profile_count, ``ScanEngine.motif_profile``, ``nanomotif motif_profile``)
against the brute force of ``test_motif_profile_host`` (built only from ``oracle.scan.subseq_indices``, ``oracle.scan.split_positions`` and
``oracle.motif.Motif``).  Counts are integers: every comparison is an equality over the WHOLE table of every candidate.  The conditions on
the input (``test_motif_profile_host.test_the_input_is_not_degenerate``) need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from nanomotif_amd import synth
from nanomotif_amd.motif import Motif
from test_gpu_motif_compare import _body, _filtered_piles, _run
from test_gpu_motif_strands import _rows
from test_motif_profile_host import (CANONICAL, PARTNERS, PROFILE_MOTIFS, TARGETS, Classes, middle, offset_of, profile_cands, profile_expected,
                                     profile_input, profile_of)

gpu = pytest.mark.gpu
STRANDS = ("same", "opposite")


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


@pytest.fixture(scope="module")
def profile_engine(engine_cls):
    names, seqs, bins, bin_names, rows, _ = profile_input()
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names], bin_names=bin_names)
    for t in TARGETS:
        eng.upload_pileup(t, *rows[t])
    yield eng
    eng.close()


def engine_cands(cands):
    return [(Motif(m, i), mt, b) for b, mt, m, i in cands]


# ------------------------------------------------------------------------------------------------ 1. a literal case
HAND_A = [[[[0, 0, 0, 2], [0, 0, 0, 2]], [[0, 0, 0, 2], [0, 0, 0, 2]]],          # o = -2: '+' sites probe -1 (outside) and 3, '-' sites 4 and 8 (outside)
          [[[0, 0, 0, 2], [0, 0, 0, 2]], [[0, 0, 0, 2], [0, 0, 0, 2]]],          # o = -1: G / C either way
          [[[2, 0, 0, 0], [0, 0, 0, 2]], [[0, 1, 1, 0], [0, 0, 0, 2]]],          # o = 0: (1, +) and (5, +) mod | (2, -) nomod, (6, -) an A without a call
          [[[0, 0, 0, 2], [0, 1, 1, 0]], [[0, 0, 0, 2], [2, 0, 0, 0]]],          # o = 1: the partner: '+' sites see (2, -), (6, -), '-' sites (1, +), (5, +)
          [[[0, 0, 0, 2], [0, 0, 0, 2]], [[0, 0, 0, 2], [0, 0, 0, 2]]]]          # o = 2
HAND_M = [[[[1, 0, 0, 1], [1, 0, 0, 1]], [[0, 0, 1, 1], [0, 0, 0, 2]]],          # o = -2: (3, +) mod, (3, -) mod, -1 outside | (4, -) a C without a call, 8 outside
          [[[0, 0, 0, 2], [0, 1, 1, 0]], [[1, 0, 0, 1], [1, 0, 1, 0]]],          # o = -1: (0, -) nomod, (4, -) nocall | (3, -) mod, (7, -) G; (3, +) mod, (7, +) nocall
          [[[0, 0, 0, 2], [0, 0, 0, 2]], [[0, 0, 0, 2], [0, 0, 0, 2]]],          # o = 0: A / T
          [[[0, 0, 0, 2], [0, 0, 0, 2]], [[0, 0, 0, 2], [0, 0, 0, 2]]],          # o = 1
          [[[1, 0, 1, 0], [1, 0, 0, 1]], [[0, 1, 1, 0], [0, 0, 0, 2]]]]          # o = 2: (3, +) mod, (7, +) nocall; (3, -) mod | (0, -) nomod, (4, -) nocall


@gpu
def test_literal_case_by_hand(engine_cls):
    """GATCGATC, GATC @ 1, radius 2: the motif occurs on '+' with its A at 1 and 5 and on '-' with its A at 2 and 6.  Classification "a":
    (1, +) 0.9, (2, -) 0.1, (5, +) 0.95.  Classification "m": (0, -) 0.0, (3, +) 1.0, (3, -) 0.8, (7, +) 0.5 (no call).  Layout
    [target][offset][occurrence strand][relative strand][mod, nomod, nocall, other]."""
    eng = engine_cls()
    eng.upload_assembly(["c"], ["GATCGATC"], ["b"])
    eng.upload_pileup("a", [0, 0, 0], [1, 2, 5], np.frombuffer(b"+-+", np.uint8), [0.9, 0.1, 0.95])
    eng.upload_pileup("m", [0, 0, 0, 0], [0, 3, 3, 7], np.frombuffer(b"-+-+", np.uint8), [0.0, 1.0, 0.8, 0.5])
    labels, sites, table = eng.motif_profile([(Motif("GATC", 1), "a", "b")], radius=2)
    assert labels == ["a", "m"] and sites.tolist() == [[2, 2]] and table.shape == (1, 2, 5, 2, 2, 4)
    assert table[0, 0].tolist() == HAND_A and table[0, 1].tolist() == HAND_M
    assert (table.sum(axis=-1) == 2).all()
    labels, sites, table = eng.motif_profile([], radius=2)
    assert labels == ["a", "m"] and sites.shape == (0, 2) and table.shape == (0, 2, 5, 2, 2, 4)
    from nanomotif_amd.engine import _ptr
    slots = np.zeros(1, np.uint8)
    assert eng.lib.nm_motif_profile_count(eng.ctx, 0, None, None, None, None, None, 1, _ptr(slots, C.c_uint8), 2, None, None) == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. geometry
@gpu
@pytest.mark.parametrize("radius", [0, 1, 10, 31])
def test_layouts_and_offsets_that_break_naive_shifting(profile_engine, radius):
    """Every candidate of the host file's input (G = 1, 2, 3; own base and probe across word, lane and chunk borders; an N run across a chunk
    border; contigs shorter than the motif; probes before the start and past the end of a contig) under both targets: ``sites`` and the
    whole table equal the brute force."""
    eng = profile_engine
    cands, exp = profile_cands(), profile_expected()
    labels, sites, table = eng.motif_profile(engine_cands(cands), targets=list(TARGETS), radius=radius)
    assert labels == list(TARGETS) and table.shape == (len(cands), 2, 2 * radius + 1, 2, 2, 4)
    for k, c in enumerate(cands):
        want = middle(exp[k][1], radius)
        assert np.array_equal(sites[k], exp[k][0]), (c, sites[k].tolist(), exp[k][0].tolist())
        assert np.array_equal(table[k], want), (c, np.argwhere(table[k] != want)[:5].tolist())
    if radius != 10:
        return
    # a candidate in the empty bin gives zeros, also between two others in the same call
    three = [("b0_empty", "a", "GATC", 1), ("b2", "a", "GATC", 1), ("b0_empty", "a", "A", 0), ("b1", "m", "C..GG", 0)]
    _, s3, t3 = eng.motif_profile(engine_cands(three), targets=list(TARGETS), radius=radius)
    assert not s3[0].any() and not t3[0].any() and not s3[2].any() and not t3[2].any()
    for k, c in ((1, three[1]), (3, three[3])):
        assert np.array_equal(s3[k], sites[cands.index(c)]) and np.array_equal(t3[k], table[cands.index(c)])
    _, s1, t1 = eng.motif_profile(engine_cands(three[:1]), radius=radius)
    assert not s1.any() and not t1.any()
    # targets in reversed order give the permuted table, a single target its slice, slot numbers are labels
    labels, s_r, t_r = eng.motif_profile(engine_cands(cands), targets=["m", "a"], radius=radius)
    assert labels == ["m", "a"] and np.array_equal(s_r, sites) and np.array_equal(t_r, table[:, ::-1])
    for ti, target in enumerate(TARGETS):
        labels, s_1, t_1 = eng.motif_profile(engine_cands(cands), targets=[target], radius=radius)
        assert labels == [target] and np.array_equal(s_1, sites) and np.array_equal(t_1, table[:, ti:ti + 1])
    labels, _, t_n = eng.motif_profile(engine_cands(cands[:3]), targets=[eng.slot_of_mod["m"], "a", "m"], radius=radius)
    assert labels == ["m", "a", "m"] and np.array_equal(t_n, table[:3][:, [1, 0, 1]])
    # one launch per width, whatever the targets and the radius
    before = eng.stats()["launches"]
    eng.motif_profile(engine_cands(cands), radius=31)
    assert eng.stats()["launches"] - before == 3


# ------------------------------------------------------------------------------------------------ 3. identities
@gpu
def test_identities_on_the_device_results(profile_engine):
    """(a) (own target, same, 0) is ``motif_site_counts``; (b) (own target, opposite, d) gives the partner marginals of
    ``motif_strand_counts``; (c) radius 10 is the middle of radius 31; (d) the reverse-complement candidate is the mirror: offsets
    negated, the occurrence strands exchanged — and with them what `same` and `opposite` mean."""
    eng = profile_engine
    cands = profile_cands()
    ecands = engine_cands(cands)
    _, sites, table = eng.motif_profile(ecands, targets=list(TARGETS), radius=31)
    own = eng.motif_site_counts(ecands)
    for k, (c, (_, six)) in enumerate(zip(cands, own)):
        six = six.sum(axis=0).reshape(2, 3)
        cell = table[k, TARGETS.index(c[1]), 31, :, 0]
        assert six.sum() > 0 and np.array_equal(sites[k], six.sum(axis=1)), c
        assert np.array_equal(cell[:, :2], six[:, :2]) and np.array_equal(cell[:, 2] + cell[:, 3], six[:, 2]), c
        if "[" not in c[2] and c[2] != "G.TC":                           # the motif fixes the modified base: no call there is nocall, never other
            assert np.array_equal(cell[:, :3], six), c
    checked = 0
    for b in ("b1", "b2"):
        for m, i, j in PARTNERS:
            mt = next(t for mm, ii, t in PROFILE_MOTIFS if (mm, ii) == (m, i))
            d = offset_of(m, i, j)
            nine = eng.motif_strand_counts([(Motif(m, i), mt, b, j)])[0][1].sum(axis=0).reshape(2, 3, 3).sum(axis=1)        # [s][partner state]
            cell = table[cands.index((b, mt, m, i)), TARGETS.index(mt), 31 + d, :, 1]
            assert np.array_equal(cell[:, :2], nine[:, :2]) and np.array_equal(cell[:, 2] + cell[:, 3], nine[:, 2]), (b, m, i, j)
            checked += int(nine.sum() > 0)
    assert checked >= 12
    _, s10, t10 = eng.motif_profile(ecands, targets=list(TARGETS), radius=10)
    assert np.array_equal(s10, sites) and np.array_equal(t10, table[:, :, 21:42])
    mirrored = []
    for b, mt, m, i in cands:
        rc = Motif(m, i).reverse_compliment()
        mirrored.append((rc, mt, b))
    _, s_m, t_m = eng.motif_profile(mirrored, targets=list(TARGETS), radius=31)
    assert np.array_equal(s_m, sites[:, ::-1]) and np.array_equal(t_m, table[:, :, ::-1, ::-1, ::-1])
    assert not np.array_equal(t_m, table)


# ------------------------------------------------------------------------------------------------ 4. refusals
@gpu
def test_errors_are_loud_and_leave_the_engine_usable(profile_engine):
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.engine import _ptr
    eng = profile_engine
    cands, exp = profile_cands(), profile_expected()
    k = cands.index(("b1", "a", "GATC", 1))
    b = eng.make_batch(engine_cands([cands[k]]), slot_of=lambda mt: 0)
    sites, counts = np.zeros((1, 2), np.uint64), np.zeros((1, 2, 63, 2, 2, 3), np.int64)

    def call(bins=b.bins, slots=(eng.slot_of_mod["a"], eng.slot_of_mod["m"]), radius=31):
        slots, bins = np.asarray(slots, np.uint8), np.asarray(bins, np.uint32)
        return eng.lib.nm_motif_profile_count(eng.ctx, 1, _ptr(bins, C.c_uint32), _ptr(b.lens, C.c_uint8), _ptr(b.modpos, C.c_uint8),
                                              _ptr(b.offsets, C.c_uint32), _ptr(b.masks, C.c_uint8), len(slots), _ptr(slots, C.c_uint8), radius,
                                              _ptr(sites, C.c_uint64), _ptr(counts, C.c_int64))
    last = lambda: eng.lib.nm_last_error().decode()
    assert call(radius=32) == -1 and "radius" in last()                 # NM_EINVAL
    assert call(slots=(eng.slot_of_mod["a"], 5)) == -3 and "target_slot[1]" in last()      # NM_ESTATE: nothing uploaded there
    assert call(slots=(200,)) == -3 and "target_slot[0]" in last()
    assert call(bins=[7]) == -1 and "cand_bin" in last() and "candidate 0" in last()
    with pytest.raises(ValueError):
        eng.motif_profile(engine_cands([cands[k]]), radius=32)
    with pytest.raises(ValueError):
        eng.motif_profile(engine_cands([cands[k]]), targets=["21839"])
    with pytest.raises(NmScanError) as e:                               # beyond the reach limit: nm_motif_sites' code
        eng.motif_profile([(Motif("A" + "." * 100 + "T", 0), "a", "b1")])
    assert e.value.code == -5
    assert not sites.any() and not counts.any()                         # a refused call has written nothing
    assert call() == 0
    assert np.array_equal(sites[0].astype(np.int64), exp[k][0]) and np.array_equal(counts[0], exp[k][1][..., :3])
    _, s, t = eng.motif_profile(engine_cands([cands[k]]), targets=list(TARGETS), radius=31)
    assert np.array_equal(s[0], exp[k][0]) and np.array_equal(t[0], exp[k][1])


# ------------------------------------------------------------------------------------------------ 5. the command
HEAD = "reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement\n"
COMMAND_SPEC = synth.SynthSpec(n_contigs=4, total_bp=300_000, n_bins=2, mod_types=("a", "m"), seed=61, min_contig_bp=40_000,
                               fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m")))
COMMAND_RADIUS = 8


def _frac(n_mod, n_nomod):
    return "%.6f" % (n_mod / (n_mod + n_nomod)) if n_mod + n_nomod else ""


def candidates_of_texts(texts):
    """[(bin, motif, mod type, position)] of several bin-motifs.tsv: rows in file order, complements included, repeats dropped."""
    out = []
    for text in texts:
        for row in _rows(text)[1]:
            both = [(row["reference"], row["motif"], row["mod_type"], int(row["mod_position"]))]
            if row["motif_complement"]:
                both.append((row["reference"], row["motif_complement"], row["mod_type"], int(row["mod_position_complement"])))
            for c in both:                                               # (a palindrome's complement is the row itself)
                if c not in out:
                    out.append(c)
    return out


def expected_files(mg, cands, radius, min_called=20):
    """The bodies of the three files from the brute force over the pre-filtered pileup, the test's own way."""
    from nanomotif_amd.motif import iupac_to_regex
    from nanomotif_amd.pileup import MOD_TYPES
    piles = _filtered_piles(mg)
    seqs = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    targets = [mt for mt in MOD_TYPES if piles[mt]]                      # slot order
    classes = Classes(seqs, piles, targets)
    bins = sorted(set(mg.bin_names))
    contigs = {bn: [n for i, n in enumerate(mg.names) if mg.bin_names[i] == bn] for bn in bins}
    bases = []
    for t in targets:
        bases += [CANONICAL[t]] if CANONICAL[t] not in bases else []
    pool = lambda table: table.sum(axis=2)                               # [target][offset][relative strand][class]
    bg, f_bins = {}, []
    cell_rows = lambda key, t, sites, cells, bg_cells: [
        key + [t, STRANDS[r], str(o), str(sites)] + [str(int(x)) for x in cells[o + radius, r]] +
        [_frac(*cells[o + radius, r, :2].tolist()), _frac(*bg_cells[o + radius, r, :2].tolist()) if bg_cells is not None else ""]
        for r in (0, 1) for o in range(-radius, radius + 1)]
    for bn in bins:
        for base in bases:
            sites, table = profile_of(classes, contigs[bn], base, 0, radius)
            for ti, t in enumerate(targets):
                if CANONICAL[t] == base:
                    bg[(bn, t)] = pool(table)[ti]
                    f_bins += cell_rows([bn, base, t, "0"], t, int(sites.sum()), bg[(bn, t)], bg[(bn, t)])
    f_main, f_summary = [], []
    for bn, m, mt, p in cands:
        sites, table = profile_of(classes, contigs[bn], iupac_to_regex(m), p, radius)
        cells = pool(table)
        key = [bn, m, mt, str(p)]
        for ti, t in enumerate(targets):
            f_main += cell_rows(key, t, int(sites.sum()), cells[ti], bg.get((bn, t)))
        own = cells[targets.index(mt), radius, 0] if mt in targets else None
        best, best_rank = None, None
        for ti, t in enumerate(targets):
            for r in (0, 1):
                for o in range(-radius, radius + 1):
                    n_mod, n_nomod = (int(x) for x in cells[ti, o + radius, r, :2])
                    b_mod, b_nomod = (int(x) for x in bg[(bn, t)][o + radius, r, :2])
                    if (t, r, o) == (mt, 0, 0) or n_mod + n_nomod < min_called or b_mod + b_nomod == 0:
                        continue
                    rank = (-(n_mod / (n_mod + n_nomod) - b_mod / (b_mod + b_nomod)), ti, r, abs(o), o)
                    if best_rank is None or rank < best_rank:
                        best, best_rank = (t, r, o, n_mod, n_nomod, b_mod, b_nomod), rank
        row = key + ([_frac(int(own[0]), int(own[1])), str(int(own[0] + own[1]))] if own is not None else ["", ""])
        if best is None:
            f_summary.append(row + [""] * 6 + ["none"])
            continue
        t, r, o, n_mod, n_nomod, b_mod, b_nomod = best
        above = own is not None and (own[0] + own[1] == 0 or n_mod * int(own[0] + own[1]) > int(own[0]) * (n_mod + n_nomod))
        flag = "shifted" if above and r == 0 and t == mt and o != 0 else "other_mod_type" if above and r == 0 and t != mt and o == 0 else "none"
        f_summary.append(row + [t, STRANDS[r], str(o), _frac(n_mod, n_nomod), _frac(b_mod, b_nomod), str(n_mod + n_nomod), flag])
    return f_main, f_bins, f_summary, targets


def shifted_row_of(mg):
    """The hand-written candidate: GATC with mod_position 0, the G next to the methylated A, in the first bin."""
    return (sorted(set(mg.bin_names))[0], "GATC", "a", 0)


def test_the_shifted_candidate_is_decided_by_the_brute_force():
    """No GPU.  For the palindrome GATC the cells (same, +1) and (opposite, +2) of GATC @ 0 hold the same calls — the two methylated A of
    every site — and differ in their background only; this input is one whose background is lower at (same, +1), so the brute force
    itself names that cell, and the flag."""
    mg = synth.make_metagenome(COMMAND_SPEC)
    _, _, f_summary, targets = expected_files(mg, [shifted_row_of(mg)], COMMAND_RADIUS)
    assert targets == ["m", "a"]
    print(f_summary[0])
    assert f_summary[0][4:6] == ["", "0"] and f_summary[0][6:9] == ["a", "same", "1"] and f_summary[0][-1] == "shifted"
    assert float(f_summary[0][9]) > 0.9 and int(f_summary[0][11]) > 100


@gpu
def test_command_on_a_synthetic_metagenome(tmp_path):
    """motif_discovery, then motif_profile --radius 8 on its bin-motifs.tsv plus a hand-written one, each in a child process, on the plain
    and the bgzip + tabix pileup: the three files equal the text derived from the brute force over the pre-filtered pileup; own_frac_mod of
    the planted motifs is n_mod / (n_mod + n_nomod) of bin-motifs.tsv and their flag is none; GATC @ 0 is flagged shifted by one."""
    from helpers import write_bgzf_tabix
    mg = synth.make_metagenome(COMMAND_SPEC)
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    mg.write_bed(tmp + "/pileup.bed")
    write_bgzf_tabix(open(tmp + "/pileup.bed", "rb").read(), tmp + "/pileup.bed.gz", block_size=50_000)
    _run(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    found = open(tmp + "/out/bin-motifs.tsv").read()
    planted = [r for r in _rows(found)[1] if (r["motif"], r["mod_type"], r["mod_position"]) in (("GATC", "a", "1"), ("CCWGG", "m", "1"))]
    assert {r["motif"] for r in planted} == {"GATC", "CCWGG"}
    shifted = shifted_row_of(mg)
    extra = HEAD + f"{shifted[0]}\tGATC\t0\ta\t1\t1\tpalindrome\t\t\t\t\n"
    open(tmp + "/extra.tsv", "w").write(extra)
    cands = candidates_of_texts([found, extra])
    assert shifted in cands and len(cands) > len(planted)
    f_main, f_bins, f_summary, targets = expected_files(mg, cands, COMMAND_RADIUS)
    assert len(f_main) == len(cands) * len(targets) * 2 * (2 * COMMAND_RADIUS + 1) and len(f_bins) == 2 * len(targets) * 2 * (2 * COMMAND_RADIUS + 1)
    for pileup, out in (("pileup.bed", "pr"), ("pileup.bed.gz", "pr_gz")):
        _run(tmp, "motif_profile", ["assembly.fasta", pileup, "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "extra.tsv", "--out", out,
                                    "--radius", str(COMMAND_RADIUS)])
        head, body = _body(f"{tmp}/{out}/motif-profile.tsv")
        assert head[:7] == ["bin", "motif", "mod_type", "mod_position", "target", "strand", "offset"]
        assert head[7:] == ["n_sites", "n_mod", "n_nomod", "n_nocall", "n_other", "frac_mod", "bg_frac_mod"]
        assert body == f_main
        assert _body(f"{tmp}/{out}/motif-profile-bins.tsv") == (head, f_bins)
        head, body = _body(f"{tmp}/{out}/motif-profile-summary.tsv")
        for row in body:
            print(out, "\t".join(row))
        assert head[4:] == ["own_frac_mod", "own_called", "best_target", "best_strand", "best_offset", "best_frac_mod", "best_bg_frac_mod", "best_called", "flag"]
        assert body == f_summary
        assert os.path.exists(f"{tmp}/{out}/args.motif_profile.json") and os.path.exists(f"{tmp}/{out}/logs/timings.motif_profile.json")
        summary = {tuple(r[:4]): r for r in body}
        for r in planted:
            row = summary[(r["reference"], r["motif"], r["mod_type"], r["mod_position"])]
            n_mod, n_nomod = int(r["n_mod"]), int(r["n_nomod"])
            assert row[4] == "%.6f" % (n_mod / (n_mod + n_nomod)) and int(row[5]) == n_mod + n_nomod, (r, row)
            assert row[-1] == "none", row
        row = summary[(shifted[0], "GATC", "a", "0")]
        assert row[-1] == "shifted" and row[6:9] == ["a", "same", "1"], row
    # a selection of targets: the same rows of those targets
    _run(tmp, "motif_profile", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "extra.tsv", "--out", "pr_a",
                                "--radius", str(COMMAND_RADIUS), "--targets", "a"])
    assert _body(f"{tmp}/pr_a/motif-profile.tsv")[1] == [r for r in f_main if r[4] == "a"]
    assert _body(f"{tmp}/pr_a/motif-profile-bins.tsv")[1] == [r for r in f_bins if r[4] == "a"]
