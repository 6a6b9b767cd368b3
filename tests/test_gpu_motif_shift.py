"""nm_motif_shift_count / nm_motif_shift_sites (csrc/nmshift.hip), ``ScanEngine.motif_shift_counts`` / ``motif_shift`` and the ``motif_shift``
command against the brute force of tests/shift_geometry.py: every comparison is equality and nothing is left out."""
import ctypes as C

import numpy as np
import pytest

import shift_geometry as S
import test_motif_fractions_host as F
import test_read_methylation_host as H
from nanomotif_amd.motif import Motif
from test_gpu_motif_fractions import _columns, _engine_candidates

pytestmark = pytest.mark.gpu
NM_EINVAL, NM_ESTATE, NM_ERANGE = -1, -3, -5
BIN_NAMES = list(F.BINS_OF)
CODES = ["m", "a", "21839"]
SLOT_B = 3


def _upload(eng, order, records, base, perm_seed=None, codes=H.CODES):
    from nanomotif_amd.contig_methylation import upload_read_statistics
    for code in codes:
        c = _columns(order, records, code, perm_seed)
        upload_read_statistics(eng, code, c["contig"], c["position"], c["strand"], c["n_valid"], c["n_mod"], c["n_diff"], H.MIN_COV, H.MIN_FRAC,
                               slot=base + CODES.index(code))


@pytest.fixture(scope="module")
def geo():
    """The geometry input resident in three bins; sample A uploaded in ascending order into the codes' own slots, sample B permuted into
    the slots from 3; the brute force's join of the candidate list, computed once per process and shared with the host suite."""
    from nanomotif_amd.engine import ScanEngine
    names, seqs, rec_a, rec_b, cands, join = S.geometry()
    assert [n for b in BIN_NAMES for n in F.BINS_OF[b]] == names
    eng = ScanEngine(0)
    eng.upload_assembly(names, [seqs[n] for n in names], [b for b in BIN_NAMES for _ in F.BINS_OF[b]], bin_names=BIN_NAMES)
    _upload(eng, names, rec_a, 0)
    _upload(eng, names, rec_b, SLOT_B, perm_seed=11)
    yield dict(eng=eng, names=names, seqs=seqs, cands=cands, join=join)
    eng.close()


def _tables(eng, cands, B, t, **kw):
    batch = _engine_candidates(cands)
    got = list(eng.motif_shift_counts(batch, bins=B, min_delta_permille=t, **kw))
    assert len(got) == len(batch) and all(g[0] is c for g, c in zip(got, batch))
    return [(names, table.copy()) for _, names, table in got]


def _assert_tables(got, want, cands, what, bins_of=F.BINS_OF):
    assert len(got) == len(want) == len(cands)
    for (names, table), w, c in zip(got, want, cands):
        assert names == bins_of[c[3]], (what, c)
        assert table.dtype == np.uint64 and table.shape == w.shape, (what, c, table.shape, w.shape)
        if not np.array_equal(table, w):
            i = int(np.flatnonzero((table != w).reshape(len(names), -1).any(axis=1))[0])
            raise AssertionError((what, c, names[i], "got", table[i].tolist(), "expected", w[i].tolist()))


def _records(eng, cands, t, select, max_records=None, **kw):
    """The concatenated records of ``ScanEngine.motif_shift``, with the batches' bookkeeping checked."""
    parts, next_cand = [], 0
    for sb in eng.motif_shift(_engine_candidates(cands), min_delta_permille=t, select=select, max_records=max_records, **kw):
        assert max_records is None or len(sb.records) <= max_records
        assert sb.records.dtype == S.RECORD and (sb.first_record == 0) == (sb.counts is not None)
        if sb.first_record == 0:
            assert sb.first_candidate == next_cand and len(sb.counts) == sb.n_candidates
            next_cand += sb.n_candidates
        parts.append(sb.records)
    assert next_cand == len(cands)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=S.RECORD)


def _assert_records(got, want, cands, what):
    assert got.dtype == want.dtype == S.RECORD
    if len(got) != len(want) or not np.array_equal(got, want):
        n = min(len(got), len(want))
        differ = np.flatnonzero(got[:n] != want[:n])
        i = int(differ[0]) if len(differ) else n
        raise AssertionError((what, "records", len(got), "expected", len(want), "first difference at", i, "got", got[i:i + 3].tolist(), "expected", want[i:i + 3].tolist()))


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("B", S.ALL_B)
def test_the_table_equals_the_brute_force(geo, B):
    for t in S.ALL_T:
        want = S.tables(geo["join"], geo["names"], F.BINS_OF, geo["cands"], B, t)
        _assert_tables(_tables(geo["eng"], geo["cands"], B, t), want, geo["cands"], (B, t))
    assert sum(int(w[:, :, B * B + 1].sum()) for w in want) > 20_000                          # paired sites


def test_the_table_does_not_depend_on_max_bytes(geo):
    want = S.tables(geo["join"], geo["names"], F.BINS_OF, geo["cands"], 3, 250)
    row = 2 * (9 + S.EXTRA) * 8
    for max_bytes in (1, 7 * row, 40 * row):
        _assert_tables(_tables(geo["eng"], geo["cands"], 3, 250, max_bytes=max_bytes), want, geo["cands"], max_bytes)
    with pytest.raises(ValueError, match="max_bytes"):
        list(geo["eng"].motif_shift_counts(_engine_candidates(geo["cands"]), max_bytes=0))
    for bad in (1, 17):
        with pytest.raises(ValueError, match="bins"):
            geo["eng"].motif_shift_counts(_engine_candidates(geo["cands"]), bins=bad)
    for bad in (-1, 1001, 2.5):
        with pytest.raises(ValueError, match="min_delta_permille"):
            geo["eng"].motif_shift_counts(_engine_candidates(geo["cands"]), min_delta_permille=bad)


# ------------------------------------------------------------------------------------------------ identities
def test_a_sample_against_itself_is_all_paired_and_its_diagonal_is_motif_fractions(geo):
    eng, cands, B = geo["eng"], geo["cands"], 10
    got = _tables(eng, cands, B, 0, slot_b=0)
    fractions = [t for _, _, t in eng.motif_fractions(_engine_candidates(cands), bins=B)]
    pileup = eng.motif_pileup_counts(_engine_candidates(cands))
    for (names, t), f, (_, p), c in zip(got, fractions, pileup, cands):
        hist, sums = t[:, :, :B * B].reshape(len(names), 2, B, B), t[:, :, B * B:]
        assert np.array_equal(np.diagonal(hist, axis1=2, axis2=3), f[:, :, :B]) and hist.sum() == f[:, :, :B].sum(), c
        assert np.array_equal(sums[:, :, 0], f[:, :, B]) and np.array_equal(sums[:, :, 1], p[:, [0, 2]]) and not sums[:, :, [2, 3, 8, 9, 10, 11]].any(), c
        assert np.array_equal(sums[:, :, [4, 5]], f[:, :, B + 1:]) and np.array_equal(sums[:, :, [6, 7]], f[:, :, B + 1:]), c
        assert np.array_equal(sums[:, :, 0] - sums[:, :, 1], p[:, [1, 3]].astype(np.uint64)), c
    assert len(_records(eng, cands, 0, ("up", "down"), slot_b=0)) == 0


def _raw_tables(eng, cands, base_a, base_b, B, t):
    """nm_motif_shift_count with sample A in the slots from ``base_a`` and sample B in the slots from ``base_b``: one call, all rows."""
    from nanomotif_amd._lib import check
    b = eng.make_batch(_engine_candidates(cands), slot_of=lambda mt: base_a + CODES.index(mt))
    slots_b = np.array([base_b + CODES.index(c[1]) for c in cands], dtype=np.uint8)
    rows = np.cumsum([0] + [len(F.BINS_OF[c[3]]) for c in cands])
    table = np.full((int(rows[-1]), 2, B * B + S.EXTRA), 77, dtype=np.uint64)                 # the caller's table need not be zeroed
    check(eng.lib.nm_motif_shift_count(eng.ctx, *eng._compare_args(b, slots_b), B, t, table.ctypes.data_as(C.POINTER(C.c_uint64))))
    return [table[rows[k]:rows[k + 1]] for k in range(len(cands))]


def test_swapping_the_samples_transposes_the_table(geo):
    eng, cands, B, t = geo["eng"], geo["cands"], 10, 250
    ab, ba = _raw_tables(eng, cands, 0, SLOT_B, B, t), _raw_tables(eng, cands, SLOT_B, 0, B, t)
    _assert_tables([(F.BINS_OF[c[3]], x) for c, x in zip(cands, ab)], S.tables(geo["join"], geo["names"], F.BINS_OF, cands, B, t), cands, "one call")
    for x, y, c in zip(ab, ba, cands):
        n = len(x)
        assert np.array_equal(x[:, :, :B * B].reshape(n, 2, B, B), y[:, :, :B * B].reshape(n, 2, B, B).transpose(0, 1, 3, 2)), c
        assert np.array_equal(x[:, :, B * B:], y[:, :, B * B:][:, :, [0, 1, 3, 2, 6, 7, 4, 5, 9, 8, 11, 10]]), c


def _pileup_records(eng, cands, base):
    b = eng.make_batch(_engine_candidates(cands), slot_of=lambda mt: base + CODES.index(mt))
    parts = [sb.records for sb in eng._pileup_windows(b, 1, 1 << 24)]
    return np.concatenate(parts)


def test_the_class_counts_and_the_records_are_the_join_of_two_pileup_exports(geo):
    """Per row n_paired + n_only_a = A's sites and n_paired + n_only_b = B's sites; the records at t = 0 in both directions plus the
    equal sites are the numpy join of two ``motif_pileup`` exports on (candidate, contig, position, strand)."""
    eng, cands = geo["eng"], geo["cands"]
    pa, pb = _pileup_records(eng, cands, 0), _pileup_records(eng, cands, SLOT_B)
    key = lambda r: (r["candidate"].astype(np.int64) << 40) | (r["contig"].astype(np.int64) << 33) | (r["pos"].astype(np.int64) << 1) | (r["code"] >> 2)
    ka, kb = key(pa), key(pb)
    assert np.all(np.diff(ka) > 0) and np.all(np.diff(kb) > 0)
    common, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    ja, jb = pa[ia], pb[ib]
    x, y = jb["n_mod"].astype(np.uint64) * ja["n_valid"], ja["n_mod"].astype(np.uint64) * jb["n_valid"]
    moved = x != y
    got = _records(eng, cands, 0, ("up", "down"))
    assert len(got) == int(moved.sum()) > 10_000 and int((~moved).sum()) > 5_000
    for f, src, g in (("candidate", ja, "candidate"), ("contig", ja, "contig"), ("pos", ja, "pos"), ("n_valid_a", ja, "n_valid"), ("n_mod_a", ja, "n_mod"),
                      ("n_valid_b", jb, "n_valid"), ("n_mod_b", jb, "n_mod")):
        assert np.array_equal(got[f], src[g][moved]), f
    assert np.array_equal(got["code"], (ja["code"][moved] & 4) | (x < y)[moved])
    tables = _tables(eng, cands, 2, 0)
    counts_a = eng.motif_pileup_counts(_engine_candidates(cands))
    for k, ((names, t), (_, a), c) in enumerate(zip(tables, counts_a, cands)):
        s = t[:, :, 4:]
        assert np.array_equal(s[:, :, 1] + s[:, :, 2], a[:, [0, 2]].astype(np.uint64)), c
        for i, name in enumerate(names):
            here = pb[(pb["candidate"] == k) & (pb["contig"] == geo["names"].index(name))]
            assert [int(x) for x in s[i, :, 1] + s[i, :, 3]] == [int((here["code"] == 0).sum()), int((here["code"] == 4).sum())], (c, name)


# ------------------------------------------------------------------------------------------------ records
@pytest.mark.parametrize("select", (("up",), ("down",), ("up", "down")), ids="+".join)
def test_the_records_equal_the_brute_force(geo, select):
    for t in (0, 250, 500, 501, 1000):
        want = S.records(geo["join"], t, select)
        _assert_records(_records(geo["eng"], geo["cands"], t, select), want, geo["cands"], (select, t))
    assert len(S.records(geo["join"], 250, select)) > 3_000


def test_the_concatenation_does_not_depend_on_the_window(geo):
    """A sub-list of a few hundred records (a window of ONE record is one library call each).  Windows of 1 and 7 records, one that ends
    inside a lane's records, one that ends between two candidates, and the default."""
    cands, t = geo["cands"], 0
    rec = S.records(geo["join"], t, ("up", "down"))
    per_cand = np.bincount(rec["candidate"], minlength=len(cands))
    small = [k for k in range(len(cands)) if per_cand[k] < 60]
    front = max((k for k in small if 20 < per_cand[k]), key=lambda k: per_cand[k])
    order = [front] + [k for k in small if k != front]
    assert 0 in per_cand[order[1:-1]] and 100 < int(per_cand[order].sum()) < 1_500 and len(order) >= 6
    sub = [cands[k] for k in order]
    want = np.concatenate([rec[rec["candidate"] == k] for k in order])
    want["candidate"] = np.repeat(np.arange(len(order), dtype=np.uint32), per_cand[order])
    first = want[want["candidate"] == 0]
    same_lane = np.flatnonzero((first["contig"][1:] == first["contig"][:-1]) & (first["pos"][1:] // 128 == first["pos"][:-1] // 128)) + 1
    inside_a_lane, between_candidates = int(same_lane[0]), len(first)
    assert 0 < inside_a_lane < between_candidates == per_cand[front]
    for limit in (1, 7, inside_a_lane, between_candidates, None):
        _assert_records(_records(geo["eng"], sub, t, ("up", "down"), max_records=limit), want, sub, limit)
    with pytest.raises(ValueError, match="max_records"):
        list(geo["eng"].motif_shift(_engine_candidates(sub), max_records=0))
    with pytest.raises(ValueError, match="direction"):
        list(geo["eng"].motif_shift(_engine_candidates(sub), select=()))


# ------------------------------------------------------------------------------------------------ saturation and large coverages
def _small_engine(names, seqs, rec_a, rec_b, bins_of):
    from nanomotif_amd.engine import ScanEngine
    eng = ScanEngine(0)
    bin_names = list(bins_of)
    eng.upload_assembly(names, [seqs[n] for n in names], [b for b in bin_names for _ in bins_of[b]], bin_names=bin_names)
    _upload(eng, names, rec_a, 0, codes=("a",))
    _upload(eng, names, rec_b, SLOT_B, codes=("a",))
    return eng


def test_one_hot_cell_under_a_record_on_every_position():
    """Two 9 000 bp poly-A contigs (two chunks each) with a record on every position and strand in both samples, the same values
    everywhere: every '+' occurrence of A adds to one cell, every site is a record."""
    L, names = 9_000, ["pa1", "pa2"]
    seqs = {n: "A" * L for n in names}
    pos, st = np.repeat(np.arange(L, dtype=np.int64), 2), np.tile(np.array([H.PLUS, H.MINUS], np.uint8), L)
    mk = lambda v, m: {(n, "a"): dict(position=pos, strand=st, n_valid=np.full(2 * L, v), n_mod=np.full(2 * L, m), n_diff=np.zeros(2 * L, np.int64)) for n in names}
    rec_a, rec_b, bins_of, cands = mk(10, 5), mk(10, 9), {"bp": names}, [("A", "a", 0, "bp")]
    join = S.join_records(names, seqs, rec_a, rec_b, bins_of, cands)
    eng = _small_engine(names, seqs, rec_a, rec_b, bins_of)
    try:
        for B, t in ((2, 400), (16, 401)):
            want = S.tables(join, names, bins_of, cands, B, t)
            _assert_tables(_tables(eng, cands, B, t), want, cands, (B, t), bins_of)
        assert want[0][:, 0, :256].max() == L and want[0][:, 0, 256 + 10].tolist() == [0, 0]
        _assert_records(_records(eng, cands, 400, ("up",), max_records=5_000), S.records(join, 400, ("up",)), cands, "saturated")
        assert len(S.records(join, 400, ("up",))) == 2 * L and len(_records(eng, cands, 401, ("up", "down"))) == 0
    finally:
        eng.close()


def test_coverages_up_to_the_last_admissible_value():
    names, seqs, rec_a, rec_b, bins_of, cands = S.large_input()
    join = S.join_records(names, seqs, rec_a, rec_b, bins_of, cands)
    assert int((join["cls"] == S.PAIRED).sum()) == len(S.LARGE_SITES)
    eng = _small_engine(names, seqs, rec_a, rec_b, bins_of)
    try:
        for t in S.ALL_T + (166, 167, 499, 999):
            _assert_tables(_tables(eng, cands, 16, t), S.tables(join, names, bins_of, cands, 16, t), cands, t, bins_of)
            for select in (("up",), ("down",), ("up", "down")):
                _assert_records(_records(eng, cands, t, select), S.records(join, t, select), cands, (t, select))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_in_the_order_of_motif_fractions_and_leave_the_engine_usable(geo):
    from nanomotif_amd._lib import NmScanError, check
    from nanomotif_amd.engine import CandidateBatch, ScanEngine
    eng = geo["eng"]
    k0 = geo["cands"].index(("GATC", "a", 1, "b0"))
    cands = geo["cands"][k0:k0 + 6]
    want = S.records(geo["join"], 250, ("up", "down"))
    want = want[(want["candidate"] >= k0) & (want["candidate"] < k0 + 6)].copy()
    want["candidate"] -= k0
    b = eng.make_batch(_engine_candidates(cands), slot_of=lambda mt: CODES.index(mt))
    slots_b = (b.slots + SLOT_B).astype(np.uint8)
    n_rows = sum(len(F.BINS_OF[c[3]]) for c in cands)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))

    def count(batch=b, sb=slots_b, B=10, t=250, null=None, n=None, ctx=None, counts=True):
        table = np.full((n_rows, 2, B * B + S.EXTRA if 2 <= B <= 16 else 1), 7, dtype=np.uint64)
        args = list(eng._compare_args(batch, sb))
        if n is not None:
            args[0] = n
        if null is not None:
            args[null] = None
        check(eng.lib.nm_motif_shift_count(eng.ctx if ctx is None else ctx, *args, B, t, p(table, C.c_uint64) if counts else None))
        return table

    def sites(batch=b, sb=slots_b, t=250, select=3, null=None, n=None, ctx=None, first=0, capacity=len(want), tail_null=None):
        cols = [np.zeros(max(capacity, 1), dtype=d) for d in (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32)]
        off, written = np.full(len(cands) + 1, 99, dtype=np.uint64), C.c_uint64(99)
        args = list(eng._compare_args(batch, sb))
        if n is not None:
            args[0] = n
        if null is not None:
            args[null] = None
        tail = [p(c, C.c_uint8 if c.dtype == np.uint8 else C.c_uint32) for c in cols] + [p(off, C.c_uint64), C.byref(written)]
        if tail_null is not None:
            tail[tail_null] = None
        check(eng.lib.nm_motif_shift_sites(eng.ctx if ctx is None else ctx, *args, t, select, first, capacity, *tail))
        return cols, off, written.value

    def still_fine():
        _assert_records(_records(eng, cands, 250, ("up", "down")), want, cands, "after a refusal")

    def refused(code, match, call, **kw):
        with pytest.raises(NmScanError, match=match) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value)
        still_fine()
        return str(e.value)

    def fractions_refusal(batch):
        with pytest.raises(NmScanError) as e:
            check(eng.lib.nm_motif_fractions_count(eng.ctx, *eng._batch_args(batch), 20, p(np.zeros((n_rows, 2, 23), np.uint64), C.c_uint64)))
        return e.value.code, str(e.value)

    for B in (0, 1, 17, 64):
        refused(NM_EINVAL, "n_bins", count, B=B)
    for call in (count, sites):
        for t in (1001, 1 << 31):
            refused(NM_EINVAL, "min_delta_permille", call, t=t)
        for null in (1, 2, 3, 4, 5, 6, 7):
            refused(NM_EINVAL, "NULL", call, null=null)
    refused(NM_EINVAL, "NULL", count, counts=False)
    for select in (0, 4, 5, 8, 1 << 31):
        refused(NM_EINVAL, "select", sites, select=select)
    for j in range(9):                                                                      # the seven columns, cand_offset, n_written
        refused(NM_EINVAL, "NULL", sites, tail_null=j)
    # the order: n_bins before min_delta_permille before select before the candidates
    assert "n_bins" in refused(NM_EINVAL, None, count, B=1, t=1001)
    assert "min_delta_permille" in refused(NM_EINVAL, None, sites, t=1001, select=0)
    k = np.arange(len(b))
    bad_bin = CandidateBatch(np.where(k == 2, 3, b.bins).astype(np.uint32), b.slots, b.lens, b.modpos, b.offsets, b.masks)
    assert "select" in refused(NM_EINVAL, None, sites, select=0, batch=bad_bin)
    # one candidate wrong in several ways: the refusal is the one nm_motif_fractions_count gives; slot A is checked before slot B
    wide = eng.make_batch(_engine_candidates(cands[:2]) + [(Motif("A" + "." * 96 + "T", 0), "a", "b0")] + _engine_candidates(cands[3:]), slot_of=lambda mt: 1)
    wrong = {
        "bin and slot": (NM_EINVAL, CandidateBatch(np.where(k == 2, 3, b.bins).astype(np.uint32), np.where(k == 2, 2, b.slots).astype(np.uint8), b.lens, b.modpos, b.offsets, b.masks)),
        "slot and reach": (NM_ESTATE, CandidateBatch(wide.bins, np.where(k == 2, 7, wide.slots).astype(np.uint8), wide.lens, wide.modpos, wide.offsets, wide.masks)),
        "reach": (NM_ERANGE, wide),
        "an earlier slot, a later bin": (NM_ESTATE, CandidateBatch(np.where(k == 4, 3, b.bins).astype(np.uint32), np.where(k == 1, 255, b.slots).astype(np.uint8), b.lens, b.modpos, b.offsets, b.masks)),
    }
    for what, (code, batch) in wrong.items():
        f_code, f_text = fractions_refusal(batch)
        assert f_code == code, (what, f_text)
        for call in (count, sites):
            assert refused(code, None, call, batch=batch) == f_text, what
    both = np.where(k == 2, 6, slots_b).astype(np.uint8)
    a_bad = CandidateBatch(b.bins, np.where(k == 2, 7, b.slots).astype(np.uint8), b.lens, b.modpos, b.offsets, b.masks)
    for call in (count, sites):
        assert "candidate 2: read-statistics slot 6 holds no pileup" in refused(NM_ESTATE, None, call, sb=both)
        assert "candidate 2: read-statistics slot 7 holds no pileup" in refused(NM_ESTATE, None, call, batch=a_bad, sb=both)
        assert "candidate 2: read-statistics slot 6 holds no pileup" in refused(NM_ESTATE, None, call, batch=wide, sb=both)     # slot B before the program
    # n_cand = 0 is NM_OK and writes nothing but the empty prefix
    assert (count(n=0) == 7).all()
    _, off, written = sites(n=0)
    assert off[0] == 0 and written == 0
    # the plain calls: windows past the end and of no capacity
    cols, off, written = sites()
    assert written == len(want) == off[-1] and off.tolist() == [0] + np.cumsum(np.bincount(want["candidate"], minlength=6)).tolist()
    for col, f in zip(cols, S.RECORD.names[1:]):
        assert np.array_equal(col[:written], want[f]), f
    assert sites(first=len(want) + 5)[2] == 0 and sites(capacity=0)[2] == 0 and sites(first=len(want) - 3)[2] == 3
    with pytest.raises(ValueError, match="no read statistics are resident for mod type.s. 21839"):
        eng.motif_shift([(Motif("GATC", 1), "21839", "b0")])
    fresh = ScanEngine(0)                                                                   # no assembly
    with pytest.raises(NmScanError) as e:
        count(ctx=fresh.ctx)
    assert e.value.code == NM_ESTATE and "nm_upload_contigs" in str(e.value)
    fresh.close()
    still_fine()


# ------------------------------------------------------------------------------------------------ the command
def _command(tmp, out, more=(), env_more=None, cb="A/cb.tsv"):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env_more or {}))
    cmd = [sys.executable, "-m", "nanomotif_amd", "motif_shift", "A/a.fasta", "A/p.bed", "B/p.bed", "-c", cb, "--bin_motifs", "A/bin-motifs.tsv", "--out", out,
           "--min_valid_read_coverage", str(H.MIN_COV), "--min_valid_cov_to_diff_fraction", str(H.MIN_FRAC)]
    return subprocess.run(cmd + list(more), cwd=tmp, env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The two samples as files, the candidate list once each plus one of a mod type neither pileup has and one of a bin the assembly
    lacks; the brute force's join of the candidates and of the backgrounds."""
    from nanomotif_amd.motif_sites import SiteCandidate
    from test_gpu_motif_pileup import _write_input
    names, seqs, rec_a, rec_b, all_cands, _ = S.geometry()
    cands = list(dict.fromkeys(all_cands))
    tmp = tmp_path_factory.mktemp("shift")
    listed = cands[:5] + [("GATC", "21839", 3, "b0"), ("GATC", "a", 1, "nowhere")] + cands[5:]
    for sub, rec in (("A", rec_a), ("B", rec_b)):
        (tmp / sub).mkdir()
        _write_input(tmp / sub, names, seqs, rec, listed)
    keys = list(dict.fromkeys((c[3], c[1]) for c in cands))
    bg = [({"a": "A", "m": "C"}[mt], mt, 0, b) for b, mt in keys]
    join = S.join_records(names, seqs, rec_a, rec_b, F.BINS_OF, cands)
    bg_join = S.join_records(names, seqs, rec_a, rec_b, F.BINS_OF, bg)
    return dict(tmp=tmp, names=names, cands=cands, site=[SiteCandidate(c[3], c[0], c[1], c[2]) for c in cands], keys=keys, bg=bg, join=join, bg_join=bg_join)


@pytest.mark.parametrize("parser", ("device", "host"))
def test_the_command_writes_the_brute_force(files, parser):
    import os
    from nanomotif_amd import fasta, motif_shift as msh
    tmp, names, cands = files["tmp"], files["names"], files["cands"]
    B, t, directions = (10, 250, ("up", "down")) if parser == "device" else (4, 500, ("down",))
    more = ["--shifted_sites"] + ([] if parser == "device" else ["--bins", "4", "--min_delta", "0.5", "--directions", "down"])
    r = _command(tmp, parser, more, {"NANOMOTIF_HOST_PARSER": "1"} if parser == "host" else {"NANOMOTIF_HOST_PARSER": "0"})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log_text = r.stdout + r.stderr
    assert "neither pileup holds rows of mod type 21839" in log_text and "the bin has no contig in the assembly" in log_text
    assert parser == "device" or "read statistics from the host parser's rows" in log_text
    k_low, k_high = msh.snap_edges(0.3, 0.7, B)
    items = [(F.BINS_OF[c[3]], x) for c, x in zip(cands, S.tables(files["join"], names, F.BINS_OF, cands, B, t))]
    backgrounds = list(zip(files["keys"], S.tables(files["bg_join"], names, F.BINS_OF, files["bg"], B, t)))
    want = msh.format_files(files["site"], items, backgrounds, B, k_low, k_high)
    for name, text in zip((msh.SUMMARY_NAME, msh.CONTIGS_NAME, msh.HIST_NAME), want):
        assert open(tmp / parser / name).read() == text, name
    bed = msh.format_bed(S.records(files["join"], t, directions), files["site"], [fasta.original_name(n) for n in names])
    assert open(tmp / parser / msh.BED_NAME).read() == bed and len(bed.splitlines()) > 1_000
    assert len(want[0].splitlines()) == len(cands) + 1 and os.path.exists(tmp / parser / "logs" / "timings.motif_shift.json")


def test_the_command_refuses_a_multi_rank_launch_and_an_aliased_contig(files):
    import os
    tmp = files["tmp"]
    r = _command(tmp, "ranks", env_more={"WORLD_SIZE": "2"})
    assert r.returncode == 2 and "one GPU" in r.stdout + r.stderr and not os.path.exists(tmp / "ranks" / "motif-shift.tsv")
    text = open(tmp / "A" / "cb.tsv").read()
    first = text.splitlines()[0].split("\t")[0]
    with open(tmp / "aliased.tsv", "w") as f:
        f.write(text + f"{first}\tanother_bin\n")
    r = _command(tmp, "aliased", cb="aliased.tsv")
    assert r.returncode == 2 and "listed under several bins" in r.stdout + r.stderr and not os.path.exists(tmp / "aliased" / "motif-shift.tsv")
