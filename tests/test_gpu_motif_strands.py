"""GPU: both-strand state of motif sites (nm_motif_strands_count / nm_motif_strands_sites, ``ScanEngine.motif_strand_counts`` /
``motif_strand_sites``, ``nanomotif motif_strands``) against the brute force of ``test_motif_strands_host`` (Python sets built only from
``oracle.scan.subseq_indices``, ``oracle.scan.split_positions`` and ``oracle.motif.Motif``).  Counts and records are integers: every
comparison is an equality over ALL candidates, contigs and records of its input.  The conditions on the input
(``test_motif_strands_host.test_the_input_is_not_degenerate``) need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from nanomotif_amd import synth
from nanomotif_amd.motif import Motif
from test_gpu_motif_compare import _body, _filtered_piles, _run, exact_p, reach_class
from test_motif_strands_host import (GEOMETRY_MOTIFS, HEMI, PAIRS, Expected, geometry_cands, geometry_expected, geometry_input)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


@pytest.fixture(scope="module")
def geometry_engine(engine_cls):
    names, seqs, bins, bin_names, rows, _ = geometry_input()
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names], bin_names=bin_names)
    eng.upload_pileup("a", *rows)
    yield eng
    eng.close()


def engine_cands(cands):
    return [(Motif(m, i), mt, b, j) for b, mt, m, i, j in cands]


def records_of(eng, cands, pairs, max_records=None):
    """All records of ``eng.motif_strand_sites`` as a list of (candidate, contig, pos, code), and the number of deliveries."""
    parts = list(eng.motif_strand_sites(engine_cands(cands), pairs=pairs, max_records=max_records))
    assert max_records is None or all(len(p.records) <= max_records for p in parts)
    rec = np.concatenate([p.records for p in parts]) if parts else np.zeros(0, dtype=[("candidate", "u4"), ("contig", "u4"), ("pos", "u4"), ("code", "u1")])
    return list(zip(rec["candidate"].tolist(), rec["contig"].tolist(), rec["pos"].tolist(), rec["code"].tolist())), len(parts)


def transposed(nine):
    return nine.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)


# ------------------------------------------------------------------------------------------------ 1. a literal case
@gpu
def test_literal_case_by_hand(engine_cls):
    """GATCGATC, GATC @ 1 with its partner at 1 of the reverse complement (d = 1): the motif occurs on '+' with its A at 1 and 5 (partners
    on '-' at 2 and 6) and on '-' with its A at 2 and 6 (partners on '+' at 1 and 5).  Classification "a": site one is hemimethylated
    ((1, +) mod, (2, -) nomod), site two has no row on '-'.  Classification "a@2": site one fully methylated, site two unmethylated."""
    eng = engine_cls()
    eng.upload_assembly(["c"], ["GATCGATC"], ["b"])
    eng.upload_pileup("a", [0, 0, 0], [1, 2, 5], np.frombuffer(b"+-+", np.uint8), [0.9, 0.1, 0.95])
    eng.upload_pileup("a", [0, 0, 0, 0], [1, 2, 5, 6], np.frombuffer(b"+-+-", np.uint8), [1.0, 0.9, 0.1, 0.0], label="a@2")
    cand = [("b", "a", "GATC", 1, 1)]
    names, table = eng.motif_strand_counts(engine_cands(cand))[0]
    #                                        '+': hemi-own (1), mod-nocall (5)      '-': hemi-partner (2), nocall-mod (6)
    assert names == ["c"] and table.tolist() == [[0, 1, 1, 0, 0, 0, 0, 0, 0] + [0, 0, 0, 1, 0, 0, 1, 0, 0]]
    assert records_of(eng, cand, HEMI)[0] == [(0, 0, 1, 1), (0, 0, 2, 16 + 3)]
    assert records_of(eng, cand, PAIRS)[0] == [(0, 0, 1, 1), (0, 0, 2, 16 + 3), (0, 0, 5, 2), (0, 0, 6, 16 + 6)]
    assert records_of(eng, cand, ("nocall-mod",))[0] == [(0, 0, 6, 16 + 6)]
    full = [("b", "a@2", "GATC", 1, 1)]
    assert eng.motif_strand_counts(engine_cands(full))[0][1].tolist() == [[1, 0, 0, 0, 1, 0, 0, 0, 0] * 2]
    assert records_of(eng, full, HEMI)[0] == []
    assert records_of(eng, full, ("mod-mod", "nomod-nomod"))[0] == [(0, 0, 1, 0), (0, 0, 2, 16), (0, 0, 5, 4), (0, 0, 6, 16 + 4)]
    # the same position on the other strand (d = 0): GATC @ 1 against (1, -) and (5, -), where no row is
    assert eng.motif_strand_counts(engine_cands([("b", "a", "GATC", 1, 2)]))[0][1].tolist() == [[0, 0, 2, 0, 0, 0, 0, 0, 0] + [0, 0, 0, 0, 0, 1, 0, 0, 1]]
    assert eng.motif_strand_counts([]) == [] and list(eng.motif_strand_sites([])) == []
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. geometry
@gpu
def test_layouts_and_offsets_that_break_naive_shifting(geometry_engine):
    """Every candidate of the geometry input (offsets 0, 1, 2, 3, -3, 31, 32, 33, 41, 63, 64, 71, 94 and more at G = 1, 2, 3; partners across
    word, lane and chunk borders; an N run across a chunk border; contigs shorter than the motif; a contig that ends in the motif): tables and
    records equal the brute force."""
    eng = geometry_engine
    cands, exp = geometry_cands(), geometry_expected()
    got = eng.motif_strand_counts(engine_cands(cands))
    assert len(got) == len(cands)
    for k, (names, table) in enumerate(got):
        assert names == eng.bin_contigs(cands[k][0])
        assert table.shape == exp.tables[k].shape and np.array_equal(table, exp.tables[k]), (cands[k], table.tolist(), exp.tables[k].tolist())
    total = np.concatenate([t for _, t in got]).sum(axis=0)
    print("columns", total.tolist())
    assert (total > 1500).all()
    for sel in (HEMI, PAIRS, ("nocall-nocall",), ("mod-mod", "nocall-mod")):
        rec, _ = records_of(eng, cands, sel)
        want = exp.selected(sel)
        assert len(rec) == len(want) and rec == want, (sel, len(rec), len(want))
    rows = eng.bin_contigs("b1")
    k = cands.index(("b1", "a", "GATC", 1, 1))
    for n in ("tiny1", "tiny2", "tiny3"):
        assert got[k][1][rows.index(n)].sum() == 0
    # a bin without contigs: no rows, no records, also next to other candidates; and an empty batch through the ABI
    assert eng.bin_contigs("b0_empty") == []
    three = [("b0_empty", "a", "GATC", 1, 1), ("b2", "a", "GATC", 1, 1), ("b0_empty", "a", "A", 0, 0)]
    res = eng.motif_strand_counts(engine_cands(three))
    assert res[0][0] == [] and res[0][1].shape == (0, 18) and res[2][1].shape == (0, 18)
    assert np.array_equal(res[1][1], got[cands.index(("b2", "a", "GATC", 1, 1))][1])
    rec, _ = records_of(eng, three, PAIRS)
    assert {r[0] for r in rec} == {1} and len(rec) == int(res[1][1].sum())
    assert records_of(eng, three[:1], PAIRS)[0] == []
    from nanomotif_amd.engine import _ptr
    rows0, tot, nw = np.zeros(1, np.uint64), np.zeros(1, np.uint64), C.c_uint64(5)
    assert eng.lib.nm_motif_strands_count(eng.ctx, 0, None, None, None, None, None, None, None, 0x1FF, _ptr(rows0, C.c_uint64), None, None) == 0
    assert eng.lib.nm_motif_strands_sites(eng.ctx, 0, None, None, None, None, None, None, None, 0x1FF, 0, 0, None, None, None, _ptr(tot, C.c_uint64),
                                          C.byref(nw)) == 0 and nw.value == 0


# ------------------------------------------------------------------------------------------------ 3. identities
@gpu
def test_identities_on_the_device_results(geometry_engine):
    """(a) the marginals are ``motif_site_counts`` of the motif and of (reverse complement, j); (b) the '-' nine of (M, i | j) is the
    transposed '+' nine of (reverse complement of M, j | i); (c) for a palindrome with j = i the '-' nine is the transpose of the '+' nine."""
    eng = geometry_engine
    cands = [c for c in geometry_cands() if c[0] == "b1"]
    got = eng.motif_strand_counts(engine_cands(cands))
    own = eng.motif_site_counts([(Motif(m, i), mt, b) for b, mt, m, i, j in cands])
    rcs = [Motif(m, i).reverse_compliment().string for _, _, m, i, _ in cands]
    partner = eng.motif_site_counts([(Motif(rc, j), mt, b) for rc, (b, mt, m, i, j) in zip(rcs, cands)])
    mirrored = eng.motif_strand_counts([(Motif(rc, j), mt, b, i) for rc, (b, mt, m, i, j) in zip(rcs, cands)])
    for c, (_, t), (_, s_own), (_, s_partner), (_, u) in zip(cands, got, own, partner, mirrored):
        assert t.sum() > 0
        nine = t.reshape(-1, 2, 3, 3)
        assert np.array_equal(nine.sum(axis=3).reshape(-1, 6), s_own), c                                 # (a) over the partner's state
        assert np.array_equal(nine[:, 0].sum(axis=1), s_partner[:, 3:]), c                              # (a) '+' nine over the own state
        assert np.array_equal(nine[:, 1].sum(axis=1), s_partner[:, :3]), c                              # (a) mirrored
        assert np.array_equal(transposed(t[:, 9:]), u[:, :9]) and np.array_equal(transposed(t[:, :9]), u[:, 9:]), c      # (b)
    palindromes = [("GATC", 1, 1), ("AATT", 0, 0), ("AATT", 3, 3)]
    assert all(p in GEOMETRY_MOTIFS for p in palindromes)
    for m, i, j in palindromes:
        t = got[cands.index(("b1", "a", m, i, j))][1]
        assert t[:, :9].sum() > 100 and np.array_equal(transposed(t[:, 9:]), t[:, :9]), (m, i, j)       # (c)
    t = got[cands.index(("b1", "a", "AATT", 1, 0))][1]                                                  # ... and not when j != i
    assert not np.array_equal(transposed(t[:, 9:]), t[:, :9])


# ------------------------------------------------------------------------------------------------ 4. windows
@gpu
def test_windows_do_not_change_the_result(geometry_engine):
    eng = geometry_engine
    every = geometry_cands()
    picked = [("b1", "a", "GATC", 1, 1), ("b2", "a", "A" + "." * 30 + "T", 0, 0), ("b0_empty", "a", "GATC", 1, 1), ("b1", "a", "A" + "." * 70 + "T", 71, 71),
              ("b2", "a", "AATT", 1, 0)]
    full = geometry_expected()
    want, per_cand, hemi = [], [], full.selected(HEMI)
    for k, c in enumerate(picked):
        mine = [(k,) + r[1:] for r in hemi if r[0] == every.index(c)] if c[0] != "b0_empty" else []
        want += mine
        per_cand.append(len(mine))
    total = len(want)
    assert 200 < total < 2000 and per_cand[2] == 0
    whole, n = records_of(eng, picked, HEMI)
    assert n == 1 and whole == want
    prime = next(q for q in range(total // 10, total) if all(q % d for d in range(2, int(q ** 0.5) + 1)))
    for budget in (prime, 7, 1):
        rec, n_b = records_of(eng, picked, HEMI, max_records=budget)
        assert rec == want, budget
        assert n_b >= total // budget
    with pytest.raises(ValueError):
        list(eng.motif_strand_sites(engine_cands(picked), max_records=0))
    # the ABI's windows: odd sizes tile the call, nothing beyond what was reported is touched
    from nanomotif_amd import _lib
    from nanomotif_amd.engine import _ptr
    bt, d = eng._strands_batch(engine_cands(picked))
    args = eng._strands_args(bt, d)
    at, parts = 0, []
    while at < total:
        cap = 133
        contig, pos, code = (np.full(cap + 8, 0xEE, dtype=t) for t in (np.uint32, np.uint32, np.uint8))
        off = np.zeros(len(picked) + 1, dtype=np.uint64)
        nw = C.c_uint64(99)
        _lib.check(eng.lib.nm_motif_strands_sites(eng.ctx, *args, 10, at, cap, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8),
                                                  _ptr(off, C.c_uint64), C.byref(nw)))
        assert nw.value == min(cap, total - at) and (code[nw.value:] == 0xEE).all() and (pos[nw.value:] == 0xEE).all() and (contig[nw.value:] == 0xEE).all()
        assert off.tolist() == [sum(per_cand[:k]) for k in range(len(picked) + 1)]
        parts += list(zip(contig[:nw.value].tolist(), pos[:nw.value].tolist(), code[:nw.value].tolist()))
        at += int(nw.value)
    assert parts == [r[1:] for r in want]
    nw = C.c_uint64(99)
    _lib.check(eng.lib.nm_motif_strands_sites(eng.ctx, *args, 10, total + 5, 10, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8),
                                              _ptr(off, C.c_uint64), C.byref(nw)))
    assert nw.value == 0 and int(off[-1]) == total


# ------------------------------------------------------------------------------------------------ 5. errors, launches
@gpu
def test_errors_are_loud_and_leave_the_engine_usable(engine_cls):
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.engine import _ptr
    eng = engine_cls()
    eng.slot_of_mod["a"] = 0
    bt, d = eng._strands_batch([(Motif("GATC", 1), "a", 0, 1)])
    rows, tot, tab = np.array([0, 1], np.uint64), np.zeros(1, np.uint64), np.zeros((1, 18), np.int64)
    count = lambda args, pset=0x1FF, r=rows: eng.lib.nm_motif_strands_count(eng.ctx, *args, pset, _ptr(r, C.c_uint64) if r is not None else None,
                                                                              _ptr(tot, C.c_uint64), _ptr(tab, C.c_int64))
    assert count(eng._strands_args(bt, d)) == -3                        # NM_ESTATE: no assembly
    eng.upload_assembly(["c"], ["GATCGATC"], ["b"])
    eng.upload_pileup("a", [0, 0], [1, 2], np.frombuffer(b"+-", np.uint8), [1.0, 0.0])
    far = Motif("A" + "." * 100 + "T", 0)
    with pytest.raises(NmScanError) as e:
        eng.motif_site_counts([(far, "a", "b")])
    sites_code = e.value.code
    assert sites_code == -5                                             # NM_ERANGE
    good = (Motif("GATC", 1), "a", "b", 1)
    for call in (lambda c: eng.motif_strand_counts(c), lambda c: list(eng.motif_strand_sites(c))):
        with pytest.raises(NmScanError) as e:                           # no such bin
            call([(Motif("GATC", 1), "a", 7, 1)])
        assert e.value.code == -1
        with pytest.raises(NmScanError) as e:                           # beyond the reach limit: nm_motif_sites' code
            call([good, (far, "a", "b", 0)])
        assert e.value.code == sites_code
        for motif, j in ((Motif("GATC", 1), 5), (Motif("GATC", 1), -2), (Motif("..GATC..", 3), 0), (Motif("GATC" + "." * 200, 1), 0)):
            with pytest.raises(NmScanError) as e:                       # a partner outside the stripped motif: NM_EINVAL, the candidate is named
                call([good, (motif, "a", "b", j)])
            assert e.value.code == -1 and "candidate 1" in str(e.value), (motif, j)
    bt, d = eng._strands_batch([good])
    args = eng._strands_args(bt, d)
    empty_slot = bt.slots.copy()
    for slot in (5, 8, 200):                                            # a slot without a pileup; a slot beyond the eight
        empty_slot[:] = slot
        assert count((len(bt), _ptr(bt.bins, C.c_uint32), _ptr(empty_slot, C.c_uint8)) + args[3:]) == -3, slot
    no_bin = np.full(len(bt), 7, np.uint32)                             # no such bin and no pileup in the slot: the bin is refused first
    assert count((len(bt), _ptr(no_bin, C.c_uint32), _ptr(empty_slot, C.c_uint8)) + args[3:]) == -1
    contig, pos, code, off, nw = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(8, np.uint8), np.zeros(2, np.uint64), C.c_uint64(0)
    sites = lambda args, pset=0x1FF, out=True: eng.lib.nm_motif_strands_sites(
        eng.ctx, *args, pset, 0, 8, *((_ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8)) if out else (None, None, None)), _ptr(off, C.c_uint64),
        C.byref(nw))
    for bad in (0, 512, 513, 0x1FF | 1 << 16, 1 << 31):
        assert count(args, bad) == -1 and sites(args, bad) == -1, bad
    assert count(args, r=None) == -1
    assert count(args, r=np.array([0, 0], np.uint64)) == -1
    assert count((1,) + (None,) * 7) == -1 and count(args[:3] + (None,) + args[4:]) == -1
    assert sites(args, out=False) == -1
    # the engine is usable afterwards: '+' 1 mod with its partner (2, -) nomod, '+' 5 without calls; '-' 2 nomod with partner mod, '-' 6 without
    assert count(args, 2) == 0
    assert tab.tolist() == [[0, 1, 0, 0, 0, 0, 0, 0, 1] + [0, 0, 0, 1, 0, 0, 0, 0, 1]] and tot.tolist() == [1]
    assert records_of(eng, [("b", "a", "GATC", 1, 1)], PAIRS)[0] == [(0, 0, 1, 1), (0, 0, 2, 16 + 3), (0, 0, 5, 8), (0, 0, 6, 16 + 8)]
    eng.close()


@gpu
def test_launches_do_not_grow_with_the_batch(geometry_engine):
    eng = geometry_engine
    cands = [c for c in geometry_cands() if c[0] == "b1"]
    assert {reach_class(m, i) for _, _, m, i, _ in cands} == {0, 1, 2}
    counted = {}
    for reps in (1, 3):
        batch = engine_cands(cands * reps)
        before = eng.stats()["launches"]
        eng.motif_strand_counts(batch)
        mid = eng.stats()["launches"]
        parts = list(eng.motif_strand_sites(batch, pairs=PAIRS))
        counted[reps] = (mid - before, eng.stats()["launches"] - mid, len(parts))
    # count: one launch per width; the export counts once for its budget, then per delivery count (3) + scan + gather + fill (3)
    assert counted[1] == (3, 3 + (3 + 2 + 3), 1) and counted[3] == counted[1]
    narrow = engine_cands([c for c in cands if reach_class(c[2], c[3]) == 0])
    before = eng.stats()["launches"]
    eng.motif_strand_counts(narrow)
    assert eng.stats()["launches"] - before == 1


# ------------------------------------------------------------------------------------------------ 6. the command
def _rows(text):
    """(header, rows as dicts) of a tab-separated table; trailing empty fields of a line are kept (a row without a complement ends in them)."""
    lines = [line for line in text.split("\n") if line.strip()]
    head = lines[0].split("\t")
    return head, [dict(zip(head, line.split("\t") + [""] * len(head))) for line in lines[1:]]


def _derived(n):
    n = [int(x) for x in n]
    both = n[0] + n[1] + n[3] + n[4]
    shares = ["%.6f" % (n[0] / both), "%.6f" % ((n[1] + n[3]) / both), "%.6f" % (n[4] / both)] if both else ["nan"] * 3
    p = "nan" if n[1] + n[3] == 0 else "%.6g" % exact_p(n[3], n[1])
    return [str(n[0]), str(n[1]), str(n[3]), str(n[4])] + shares + [p]


def _expected_files(mg, bin_motifs_texts, pairs=HEMI):
    """The three files the brute force gives for the candidates of several bin-motifs.tsv under the partner rule, the test's own way: rows in
    file order, complements included, a (bin, motif, mod type, position) seen before dropped; a row's complement names the partner, else
    every position of the IUPAC reverse complement that holds the canonical letter."""
    from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL, iupac_to_regex, reverse_compliment
    piles = _filtered_piles(mg)
    seqs = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    four, seen, partner_of = [], set(), {}
    for text in bin_motifs_texts:
        for row in _rows(text)[1]:
            both = [(row["reference"], row["motif"], row["mod_type"], int(row["mod_position"]))]
            if row["motif_complement"]:
                both.append((row["reference"], row["motif_complement"], row["mod_type"], int(row["mod_position_complement"])))
                partner_of.setdefault(both[0], []).append(both[1][3])
                partner_of.setdefault(both[1], []).append(both[0][3])
            for c in both:
                if c not in seen:
                    seen.add(c)
                    four.append(c)
    cands = []
    for c in four:
        js = sorted(set(partner_of[c]), key=partner_of[c].index) if c in partner_of else \
            [j for j, letter in enumerate(reverse_compliment(c[1])) if letter == MOD_TYPE_TO_CANONICAL[c[2]]]
        cands += [c + (j,) for j in js]
    bins = sorted(set(mg.bin_names))
    bin_contigs = {bn: [n for i, n in enumerate(mg.names) if mg.bin_names[i] == bn] for bn in bins}      # contig_bin.tsv order
    index = {n: i for i, n in enumerate(mg.names)}
    exp = Expected([(bn, mt, iupac_to_regex(m), p, j) for bn, m, mt, p, j in cands], bin_contigs, index, seqs, piles)
    f_main, f_contigs, offsets = [], [], []
    for k, (bn, m, mt, p, j) in enumerate(cands):
        pal = int(reverse_compliment(m) == m and p == j)
        t = exp.tables[k].sum(axis=0)
        nine = (t[:9] if pal else t[:9] + t[9:]).tolist()
        f_main.append([bn, m, mt, str(p), str(j), str(pal)] + [str(x) for x in nine] + _derived(nine))
        f_contigs += [[bn, name, m, mt, str(p), str(j)] + [str(int(x)) for x in exp.tables[k][r]] for r, name in enumerate(bin_contigs[bn])]
        offsets.append(len(m) - 1 - p - j)
    want = {PAIRS.index(t) for t in pairs}
    bed = "".join(f"{mg.names[c]}\t{p}\t{p + 1}\t{cands[k][1]}_{cands[k][2]}_{cands[k][3]}\t0\t{'-' if code & 16 else '+'}\t{PAIRS[code & 15]}\t{cands[k][0]}\t{q}\n"
                  for k, c, p, code, q in exp.records if (code & 15) in want)
    return f_main, f_contigs, bed, cands, exp


HEAD = "reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement\n"


@gpu
def test_command_on_a_synthetic_metagenome(tmp_path):
    """motif_discovery, then motif_strands --hemi_sites on its bin-motifs.tsv plus a hand-written one (a complement pair, a motif whose
    reverse complement holds two candidate positions, one with none), each in a child process, plain and bgzip + tabix: the three files equal
    the text derived from the brute force over the pre-filtered pileup, and every row's n_mod / n_nomod and n_mod_complement /
    n_nomod_complement of the discovered bin-motifs.tsv are the marginals of its table."""
    from helpers import write_bgzf_tabix
    from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL, reverse_compliment
    spec = synth.SynthSpec(n_contigs=4, total_bp=400_000, n_bins=2, mod_types=("a", "m"), seed=61, min_contig_bp=60_000,
                           fixed_motifs=(("GATC", 1, "a"), ("GAACT", 1, "a"), ("AGTTC", 0, "a"), ("CCWGG", 1, "m")))
    mg = synth.make_metagenome(spec)
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    mg.write_bed(tmp + "/pileup.bed")
    write_bgzf_tabix(open(tmp + "/pileup.bed", "rb").read(), tmp + "/pileup.bed.gz", block_size=50_000)
    _run(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    found = open(tmp + "/out/bin-motifs.tsv").read()
    assert ("bin_001", "GATC") in {(r["reference"], r["motif"]) for r in _rows(found)[1]}
    extra = HEAD + "bin_000\tGAACT\t1\ta\t1\t1\tnon-palindrome\tAGTTC\t0\t1\t1\nbin_001\tATTG\t0\ta\t1\t1\tnon-palindrome\t\t\t\t\n" \
                   "bin_001\tACCCA\t4\ta\t1\t1\tnon-palindrome\t\t\t\t\nbin_000\tCCWGG\t1\tm\t1\t1\tpalindrome\t\t\t\t\n"
    open(tmp + "/extra.tsv", "w").write(extra)
    f_main, f_contigs, bed, cands, exp = _expected_files(mg, [found, extra])
    assert len(bed) > 0 and len(f_main) > len(_rows(found)[1])
    assert ("bin_000", "GAACT", "a", 1, 0) in cands and ("bin_000", "AGTTC", "a", 0, 1) in cands and ("bin_001", "ATTG", "a", 0, 2) in cands
    assert not any(c[1] == "ACCCA" for c in cands)
    for pileup, out in (("pileup.bed", "st"), ("pileup.bed.gz", "st_gz")):
        r = _run(tmp, "motif_strands", ["assembly.fasta", pileup, "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "extra.tsv", "--out", out,
                                        "--hemi_sites"])
        assert "ACCCA_a_4" in r.stdout + r.stderr                        # the motif without a partner is named
        head, body = _body(f"{tmp}/{out}/motif-strands.tsv")
        assert head[:6] == ["bin", "motif", "mod_type", "mod_position", "partner_position", "palindrome"] and head[6:15] == ["n_" + t.replace("-", "_") for t in PAIRS]
        assert head[15:] == ["n_full", "n_hemi_own", "n_hemi_partner", "n_unmethylated", "frac_full", "frac_hemi", "frac_unmethylated", "strand_bias_p"]
        for row in body:
            print(out, "\t".join(row))
        assert body == f_main
        head, body = _body(f"{tmp}/{out}/motif-strands-contigs.tsv")
        assert len(head) == 24 and body == f_contigs
        got_bed = open(f"{tmp}/{out}/hemi-sites.bed").read()
        assert len(got_bed) == len(bed) and got_bed == bed
        assert os.path.exists(f"{tmp}/{out}/args.motif_strands.json") and os.path.exists(f"{tmp}/{out}/logs/timings.motif_strands.json")
        assert not os.path.exists(f"{tmp}/{out}/motif-strands-bins.tsv")
        # every row of the discovered bin-motifs.tsv finds its counts in the marginals of its table (both occurrence strands, all contigs)
        table = {}
        for row in body:
            key = (row[0], row[2], row[3], int(row[4]), int(row[5]))
            table[key] = table.get(key, 0) + np.array([int(x) for x in row[6:]]).reshape(2, 3, 3).sum(axis=0)
        checked = 0
        for r in _rows(found)[1]:
            i = int(r["mod_position"])
            js = [int(r["mod_position_complement"])] if r["motif_complement"] else [c[4] for c in cands if c[:4] == (r["reference"], r["motif"], r["mod_type"], i)]
            if not js:                                                  # (a discovered motif the other strand cannot be modified in)
                assert MOD_TYPE_TO_CANONICAL[r["mod_type"]] not in reverse_compliment(r["motif"]), r
            for j in js:
                nine = table[(r["reference"], r["motif"], r["mod_type"], i, j)]
                assert (int(nine[0].sum()), int(nine[1].sum())) == (int(r["n_mod"]), int(r["n_nomod"])), (r, nine.tolist())
                if r["motif_complement"]:
                    assert (int(nine[:, 0].sum()), int(nine[:, 1].sum())) == (int(r["n_mod_complement"]), int(r["n_nomod_complement"])), (r, nine.tolist())
                checked += 1
        assert checked >= 2
    # the planted palindrome is fully methylated on both strands; the planted pair GAACT / AGTTC as well
    main = {(r[0], r[1], r[2], int(r[3]), int(r[4])): r for r in f_main}
    for key in (("bin_001", "GATC", "a", 1, 1), ("bin_000", "GAACT", "a", 1, 0)):
        row = main[key]
        assert float(row[19]) > 0.8 and int(row[15]) > 100, row
    # other pairs: the same tables, other records; without --hemi_sites no BED
    _run(tmp, "motif_strands", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "extra.tsv", "--out", "st_lost",
                                "--hemi_sites", "--pairs", "mod-nocall,nocall-mod,mod-nomod"])
    lost = ("mod-nomod", "mod-nocall", "nocall-mod")
    assert open(tmp + "/st_lost/hemi-sites.bed").read() == _expected_files(mg, [found, extra], pairs=lost)[2]
    _run(tmp, "motif_strands", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "extra.tsv", "--out", "st_plain"])
    assert not os.path.exists(tmp + "/st_plain/hemi-sites.bed")
    for name in ("motif-strands.tsv", "motif-strands-contigs.tsv"):
        assert open(f"{tmp}/st_plain/{name}").read() == open(f"{tmp}/st/{name}").read() == open(f"{tmp}/st_lost/{name}").read()
