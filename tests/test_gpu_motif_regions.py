"""GPU: annotated regions as class planes and the motif sites counted and exported against them (nm_regions_*, nm_motif_regions_*,
``ScanEngine.upload_regions`` / ``motif_regions_counts`` / ``motif_regions_sites``, ``nanomotif motif_regions``) against the brute force of
``regions_geometry`` (sets of positions, a regex scan, dense state tables: nothing shared with the engine).  Every comparison is an
equality.  The conditions on the input (``test_motif_regions_host.test_the_input_is_not_degenerate``) need no GPU."""
import ctypes as C
import gzip
import itertools
import os

import numpy as np
import pytest

import regions_geometry as rg
from nanomotif_amd.motif import Motif

gpu = pytest.mark.gpu
KS = (1, 3, 8)


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


def make_engine(engine_cls):
    seqs, _, _ = rg.geometry()
    eng = engine_cls()
    eng.upload_assembly(rg.NAMES, [seqs[n] for n in rg.NAMES], [rg.BINS[n] for n in rg.NAMES], bin_names=rg.BIN_NAMES)
    for mt in ("a", "m"):
        eng.upload_pileup(mt, *rg.pileup_arrays(mt))
    return eng


@pytest.fixture(scope="module")
def engine(engine_cls):
    eng = make_engine(engine_cls)
    yield eng
    eng.close()


def upload(eng, k, intervals=None):
    iv, k = rg.region_set(k, intervals)
    eng.upload_regions(*rg.interval_arrays(iv), [f"c{c}" for c in range(k)])
    return rg.class_sets(iv, k), iv


@pytest.fixture(scope="module")
def expected():
    """K -> (class sets, whole count tables of every candidate): computed once, shared, never changed."""
    out = {}
    for k in KS:
        sets = rg.class_sets(*rg.region_set(k))
        out[k] = (sets, [rg.expected_table(c, sets, k) for c in rg.candidates()])
    return out


def engine_cands(cands):
    return [(Motif(m, i), mt, b) for b, mt, m, i in cands]


def pieces_of(intervals, p):
    """The rasteriser's cuts restated: an interval is cut at multiples of p plane words from its contig's first word."""
    return sum((e - 1) // 32 // p - s // 32 // p + 1 for _, s, e, _ in intervals)


def check_planes(eng, sets, k):
    covered = eng.region_covered()
    assert covered.shape == (k, len(rg.NAMES))
    for c in range(k):
        for i, n in enumerate(rg.NAMES):
            mask = eng.region_mask(n, c)
            assert mask.dtype == bool and mask.shape == (rg.LENGTHS[n],)
            assert set(np.flatnonzero(mask).tolist()) == sets[(n, c)], (k, c, n)
            assert covered[c, i] == len(sets[(n, c)]), (k, c, n)
    # which classes every chunk of every contig holds, chunk by chunk
    for n in rg.NAMES:
        want = [sum(1 << c for c in range(k) if any(p // rg.CHUNK == q for p in sets[(n, c)])) for q in range((rg.LENGTHS[n] + rg.CHUNK - 1) // rg.CHUNK)]
        got = eng.region_chunk_classes(n)
        assert got.dtype == np.uint8 and got.tolist() == want, (k, n)


# ------------------------------------------------------------------------------------------------ 1. the planes
@gpu
@pytest.mark.parametrize("piece", [None, "64", "1"])
@pytest.mark.parametrize("k", KS)
def test_planes_and_covered_equal_the_brute_force(engine, expected, monkeypatch, k, piece):
    if piece is None:
        monkeypatch.delenv("NM_REGIONS_PIECE_WORDS", raising=False)
    else:
        monkeypatch.setenv("NM_REGIONS_PIECE_WORDS", piece)
    sets, iv = upload(engine, k)
    assert sets == expected[k][0]
    check_planes(engine, sets, k)
    n_pieces = C.c_uint64(0)
    assert engine.lib.nm_regions_shape(engine.regions, None, None, C.byref(n_pieces)) == 0
    assert n_pieces.value == pieces_of(iv, int(piece or 2048))


@gpu
def test_a_second_set_replaces_the_first_and_zero_intervals_are_valid(engine):
    upload(engine, 8)
    sets, _ = upload(engine, 1, rg.SECOND_SET)
    check_planes(engine, sets, 1)
    assert engine.region_covered().sum() == 30 + 13 + 1
    engine.upload_regions([], [], [], [], ["a", "b"])
    assert not engine.region_covered().any() and not engine.region_mask("long", 1).any()
    assert [engine.region_chunk_classes(n).tolist() for n in rg.NAMES] == [[0], [0], [0, 0], [0], [0, 0, 0]]


# ------------------------------------------------------------------------------------------------ 2. the count tables
@gpu
@pytest.mark.parametrize("k", KS)
def test_whole_count_tables_equal_the_brute_force(engine, expected, k):
    cands = rg.candidates()
    upload(engine, k)
    before = engine.stats()["launches"]
    got = list(engine.motif_regions_counts(engine_cands(cands)))
    assert engine.stats()["launches"] - before == 3                       # one launch per width
    assert len(got) == len(cands)
    for c, (names, t), want in zip(cands, got, expected[k][1]):
        assert names == rg.contigs_of(c[0]) and t.dtype == np.int64 and t.shape == want.shape == (len(names), k + 1, 2, 3)
        assert np.array_equal(t, want), (k, c, np.argwhere(t != want)[:5].tolist())
    again = list(engine.motif_regions_counts(engine_cands(cands)))      # a second call gives the same table
    single = list(engine.motif_regions_counts(engine_cands(cands), max_bytes=1))
    for a, b, c in zip(got, again, single):
        assert a[0] == b[0] == c[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
    if k != 8:
        return
    want = expected[k][1]
    rev = list(engine.motif_regions_counts(engine_cands(cands[::-1])))
    assert all(np.array_equal(r[1], w) for r, w in zip(rev, want[::-1]))
    order = [4, 4, 0, 11, 4, 9, 0]
    dup = list(engine.motif_regions_counts(engine_cands([cands[j] for j in order])))
    assert all(np.array_equal(d[1], want[j]) for d, j in zip(dup, order))
    # a candidate of the empty bin between two others gives no rows
    three = [cands[2], ("b0_empty", "a", "GATC", 1), cands[7]]
    g3 = list(engine.motif_regions_counts(engine_cands(three)))
    assert g3[1][0] == [] and g3[1][1].shape == (0, 9, 2, 3)
    assert np.array_equal(g3[0][1], want[2]) and np.array_equal(g3[2][1], want[7])


@gpu
def test_identities_with_motif_site_counts(engine):
    cands = rg.candidates()
    ecands = engine_cands(cands)
    own = engine.motif_site_counts(ecands)
    six = lambda cell: cell.reshape(cell.shape[0], 6)
    # classes that partition the positions: the cells and outside sum to the sites
    parts = [(n, s, min(s + 1000, rg.LENGTHS[n]), (s // 1000) % 3) for n in ("one", "long", "odd") for s in range(0, rg.LENGTHS[n] - 3000, 1000)]
    engine.upload_regions(*rg.interval_arrays(parts), ["p0", "p1", "p2"])
    for (names, t), (names6, s) in zip(engine.motif_regions_counts(ecands), own):
        assert names == names6 and np.array_equal(six(t.sum(axis=1)), s) and t[:, :3].sum() > 0 and (t[:, 3].sum() > 0 or len(names) == 0)
    # one class of whole-contig intervals: inside is everything, outside nothing
    whole = [(n, 0, rg.LENGTHS[n], 0) for n in rg.NAMES]
    engine.upload_regions(*rg.interval_arrays(whole), ["all"])
    for (_, t), (_, s) in zip(engine.motif_regions_counts(ecands), own):
        assert np.array_equal(six(t[:, 0]), s) and not t[:, 1].any()
    # zero intervals: outside is everything
    engine.upload_regions([], [], [], [], ["none"])
    for (_, t), (_, s) in zip(engine.motif_regions_counts(ecands), own):
        assert np.array_equal(six(t[:, 1]), s) and not t[:, 0].any()


# ------------------------------------------------------------------------------------------------ 3. the records
def records_as_tuples(batches):
    rec = np.concatenate([sb.records for sb in batches])
    return list(zip(*(rec[f].tolist() for f in ("candidate", "contig", "pos", "code", "classes"))))


SELECTIONS = [(["c5"], 1 << 5, False), (None, 0xFF, False), (["outside"], 0, True), (["c2", "outside"], 1 << 2, True)]


@gpu
@pytest.mark.parametrize("states", [("mod",), ("nomod",), ("nocall",), ("mod", "nomod", "nocall")])
def test_records_equal_the_brute_force(engine, expected, states):
    """Every combination of states, classes and max_records on the G = 1 motifs (a window of one record is a library call per site); the
    G = 2 and G = 3 motifs, thousands of sites each, with every combination of states and classes in windows of the default size."""
    from nanomotif_amd.engine import SITE_STATES
    sets = expected[8][0]
    upload(engine, 8)
    for cands, sizes in ((rg.candidates()[:4], (1, 7, None)), (rg.candidates()[4:8], (None,))):
        for (classes, class_set, outside), max_records in itertools.product(SELECTIONS, sizes):
            want = rg.expected_records(cands, sets, 8, [SITE_STATES.index(s) for s in states], class_set, outside)
            batches = list(engine.motif_regions_sites(engine_cands(cands), states=states, classes=classes, max_records=max_records))
            assert all(len(sb.records) <= (max_records or 1 << 60) for sb in batches)
            assert records_as_tuples(batches) == want, (states, classes, max_records)
            assert len(want) > 0


@gpu
def test_overlapping_classes_need_inclusion_exclusion(engine, expected):
    """The classes byte holds ALL classes of a site, and where the selected classes overlap (c6 and c7 share 2000..2099 and 4000) the
    number of records is the union, not the sum of the cells."""
    cands = [("b1", "a", "A", 0)]
    sets = expected[8][0]
    upload(engine, 8)
    table = list(engine.motif_regions_counts(engine_cands(cands)))[0][1]
    rec = np.concatenate([sb.records for sb in engine.motif_regions_sites(engine_cands(cands), classes=["c6", "c7"])])
    both = int(((rec["classes"] >> 6 & 1) & (rec["classes"] >> 7 & 1)).sum())
    assert both > 50 and len(rec) == int(table[:, 6].sum() + table[:, 7].sum()) - both
    assert records_as_tuples([type("B", (), {"records": rec})]) == rg.expected_records(cands, sets, 8, class_set=0xC0)
    assert any(m & ~0xC0 for m in rec["classes"].tolist())               # classes outside the selection are reported too
    one = np.concatenate([sb.records for sb in engine.motif_regions_sites(engine_cands(cands), classes=["c6"])])
    assert len(one) == int(table[:, 6].sum())                             # a single class: its cell


# ------------------------------------------------------------------------------------------------ 4. refusals
def raw_create(eng, contig, start, end, cls, n_classes, nulls=()):
    from nanomotif_amd.engine import _ptr
    arrs = [np.asarray(contig, np.uint32), np.asarray(start, np.uint64), np.asarray(end, np.uint64), np.asarray(cls, np.uint8)]
    ptrs = [_ptr(a, t) if len(a) else None for a, t in zip(arrs, (C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint8))]
    for j in nulls:
        ptrs[j] = None
    h = C.c_void_p()
    rc = eng.lib.nm_regions_create(eng.ctx, len(arrs[0]), *ptrs, n_classes, C.byref(h))
    return rc, h


@gpu
def test_region_set_refusals_in_order(engine, engine_cls):
    last = lambda: engine.lib.nm_last_error().decode()
    L = rg.LENGTHS["small"]

    def fine():
        rc, h = raw_create(engine, [0], [1], [L], [1], 2)
        assert rc == 0 and h.value
        bp = np.zeros((2, len(rg.NAMES)), np.uint64)
        assert engine.lib.nm_regions_covered(h, bp.ctypes.data_as(C.POINTER(C.c_uint64))) == 0 and bp.sum() == bp[1, 0] == L - 1
        assert engine.lib.nm_regions_destroy(h) == 0
    fine()
    for j in range(4):
        assert raw_create(engine, [0], [1], [2], [0], 1, nulls=(j,))[0] == -1 and "NULL" in last()
    assert engine.lib.nm_regions_create(engine.ctx, 0, None, None, None, None, 1, None) == -1 and "NULL" in last()
    for n in (0, 9):
        assert raw_create(engine, [0], [1], [2], [0], n)[0] == -1 and "n_classes" in last()
    assert raw_create(engine, [0], [1], [2], [0], 0, nulls=(0,))[0] == -1 and "NULL" in last()           # NULL before n_classes
    bare = engine_cls()
    assert raw_create(bare, [0], [1], [2], [0], 1)[0] == -3 and "nm_upload_contigs" in last()
    assert raw_create(bare, [0], [1], [2], [0], 9)[0] == -1 and "n_classes" in last()                    # n_classes before the assembly
    bare.close()
    fine()
    ok = ([0, 0], [1, 5], [4, 9], [0, 1])
    for what, field, bad in (("contig 5 >= n_contigs 5", 0, 5), ("class 2 >= n_classes 2", 3, 2), ("start 9 >= end 9", 1, 9), (f"end {L + 1} past", 2, L + 1)):
        args = [list(a) for a in ok]
        args[field][1] = bad
        assert raw_create(engine, *args, 2)[0] == -1 and "interval 1:" in last() and what in last(), what
    # an interval wrong in two ways is refused by the earlier check; two wrong intervals by the first in call order
    assert raw_create(engine, [9, 0], [1, 5], [4, 9], [7, 1], 2)[0] == -1 and "interval 0: contig 9" in last()
    assert raw_create(engine, [0, 0], [1, 5], [4, 9], [7, 1], 2)[0] == -1 and "interval 0: class 7" in last()
    assert raw_create(engine, [0, 0], [7, 5], [4, 9], [7, 1], 2)[0] == -1 and "interval 0: class 7" in last()
    assert raw_create(engine, [0, 0], [L + 5, 5], [L + 2, 9], [1, 1], 2)[0] == -1 and "interval 0: start" in last()
    assert raw_create(engine, [0, 7], [1, 5], [L + 1, 9], [1, 1], 2)[0] == -1 and "interval 0: end" in last()
    rc, h = raw_create(engine, [], [], [], [], 3)                         # zero intervals are valid
    assert rc == 0 and engine.lib.nm_regions_destroy(h) == 0
    fine()


def entry_call(eng, which, handle, b, counts, state_set=7, class_set=1, outside=0, bins=None, slots=None, rows=None, nulls=()):
    from nanomotif_amd.engine import _ptr
    n_rows = counts.shape[0]
    bins = np.asarray(b.bins if bins is None else bins, np.uint32)
    slots = np.asarray(b.slots if slots is None else slots, np.uint8)
    rows = np.asarray((0, n_rows) if rows is None else rows, np.uint64)
    args = [_ptr(bins, C.c_uint32), _ptr(slots, C.c_uint8), _ptr(b.lens, C.c_uint8), _ptr(b.modpos, C.c_uint8), _ptr(b.offsets, C.c_uint32),
            _ptr(b.masks, C.c_uint8)]
    if which == "count":
        tail = [_ptr(rows, C.c_uint64), None, _ptr(counts, C.c_int64)]
    else:
        cap = 1 << 16
        keep = [np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(2, np.uint64), C.c_uint64(0)]
        tail = [0, cap, _ptr(keep[0], C.c_uint32), _ptr(keep[1], C.c_uint32), _ptr(keep[2], C.c_uint8), _ptr(keep[3], C.c_uint8), _ptr(keep[4], C.c_uint64),
                C.byref(keep[5])]
        entry_call.kept = keep
    full = args + [state_set, class_set, outside] + tail
    for j in nulls:
        full[j] = None
    fn = eng.lib.nm_motif_regions_count if which == "count" else eng.lib.nm_motif_regions_sites
    return fn(eng.ctx, handle, 1, *full)


@gpu
@pytest.mark.parametrize("which", ["count", "sites"])
def test_entry_point_refusals_in_order(engine, engine_cls, expected, which):
    from nanomotif_amd._lib import NmScanError
    cands = rg.candidates()
    j = cands.index(("b1", "a", "GATC", 1))
    upload(engine, 3)
    h = engine.regions
    want = expected[3][1][j]
    b = engine.make_batch(engine_cands([cands[j]]))
    far = engine.make_batch([(Motif("A" + "." * 100 + "T", 0), "a", "b1")])
    counts = np.zeros(want.shape, np.int64)
    last = lambda: engine.lib.nm_last_error().decode()
    call = lambda **kw: entry_call(engine, which, kw.pop("handle", h), kw.pop("batch", b), counts, **kw)

    def fine():
        counts[:] = -1
        assert call() == 0
        if which == "count":
            assert np.array_equal(counts, want)
        else:
            assert entry_call.kept[5].value == entry_call.kept[4][1] == want[:, 0].sum()
    fine()
    counts[:] = 0
    for k in (0, 1, 2, 3, 4, 5):
        assert call(nulls=(k,)) == -1 and "NULL" in last(), k
    assert call(handle=None) == -3 and "no region set" in last()
    assert call(state_set=0) == -1 and "state_set" in last()
    assert call(state_set=8) == -1 and "state_set" in last()
    assert call(class_set=8) == -1 and "class_set" in last() and "n_classes 3" in last()
    assert call(class_set=0) == -1 and "nothing is selected" in last()
    assert call(class_set=0, outside=1) == 0
    fine()
    counts[:] = 0
    # the order: NULL, state_set, class_set, assembly, layout, then the candidate's bin, slot, program, rows
    assert call(state_set=0, nulls=(2,)) == -1 and "NULL" in last()
    assert call(state_set=0, class_set=8) == -1 and "state_set" in last()
    assert call(class_set=8, bins=[7]) == -1 and "class_set" in last()
    assert call(bins=[7]) == -1 and "cand_bin" in last() and "candidate 0" in last()
    assert call(slots=[5]) == -3 and "cand_mod_slot[0]" in last()
    assert call(batch=far) == -5
    # a candidate with a bad bin AND a bad program gives nm_motif_sites_count's own message
    assert call(bins=[7], batch=far) == -1
    mine = last()
    rows = np.zeros(2, np.uint64)
    tot, six = np.zeros(1, np.uint64), np.zeros((4, 6), np.int64)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    assert engine.lib.nm_motif_sites_count(engine.ctx, 1, p(np.array([7], np.uint32), C.c_uint32), p(far.slots, C.c_uint8), p(far.lens, C.c_uint8),
                                           p(far.modpos, C.c_uint8), p(far.offsets, C.c_uint32), p(far.masks, C.c_uint8), 7, p(rows, C.c_uint64),
                                           p(tot, C.c_uint64), p(six, C.c_int64)) == -1
    assert last() == mine
    if which == "count":
        assert call(rows=(0, want.shape[0] - 1)) == -1 and "row_offset" in last()
        assert not counts.any()                                           # a refused call has written nothing
    # no assembly in the ctx: refused before the layouts are compared; a handle of another assembly: NM_ESTATE
    bare = engine_cls()
    assert entry_call(bare, which, h, b, counts) == -3 and "nm_upload_contigs" in last()
    assert entry_call(bare, which, h, b, counts, class_set=8) == -1 and "class_set" in last()
    bare.close()
    other = make_engine(engine_cls)
    seqs, _, _ = rg.geometry()
    rc, old = raw_create(other, [0], [0], [5], [0], 3)
    assert rc == 0
    assert entry_call(other, which, old, b, counts) == 0
    other.upload_assembly(rg.NAMES[:4], [seqs[n] for n in rg.NAMES[:4]], [rg.BINS[n] for n in rg.NAMES[:4]], bin_names=rg.BIN_NAMES)
    other.upload_pileup("a", *[a[:10] for a in rg.pileup_arrays("a")])
    assert entry_call(other, which, old, b, counts) == -3 and "another assembly" in last()
    assert other.lib.nm_regions_destroy(old) == 0
    other.close()
    fine()
    # through the engine: no region set, and after clear_regions
    e2 = make_engine(engine_cls)
    run = (lambda: list(e2.motif_regions_counts(engine_cands([cands[j]])))) if which == "count" else (lambda: list(e2.motif_regions_sites(engine_cands([cands[j]]))))
    with pytest.raises(NmScanError) as err:
        run()
    assert err.value.code == -3 and "no region set" in str(err.value)
    upload(e2, 3)
    assert len(run()) >= 1
    e2.clear_regions()
    with pytest.raises(NmScanError) as err:
        run()
    assert err.value.code == -3
    e2.close()
    fine()


@gpu
def test_a_region_set_outlives_its_engine(engine_cls):
    eng = make_engine(engine_cls)
    rc, h = raw_create(eng, [4], [0], [100], [0], 1)
    assert rc == 0
    lib = eng.lib
    eng.close()
    bp = np.zeros((1, len(rg.NAMES)), np.uint64)
    assert lib.nm_regions_covered(h, bp.ctypes.data_as(C.POINTER(C.c_uint64))) == 0 and bp[0, 4] == 100
    assert lib.nm_regions_destroy(h) == 0
    assert lib.nm_regions_destroy(None) == 0


@gpu
def test_n_cand_zero_and_python_side_refusals(engine):
    upload(engine, 3)
    assert list(engine.motif_regions_counts([])) == []
    assert list(engine.motif_regions_sites([])) == []
    rows = np.zeros(1, np.uint64)
    assert engine.lib.nm_motif_regions_count(engine.ctx, engine.regions, 0, None, None, None, None, None, None, 7, 1, 0, rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             None, None) == 0
    with pytest.raises(ValueError):
        list(engine.motif_regions_sites(engine_cands(rg.candidates()[:1]), classes=["nope"]))
    with pytest.raises(ValueError):
        engine.upload_regions([0], [1], [2], [0, 0], ["a"])


# ------------------------------------------------------------------------------------------------ 5. the command
def annotation(mg):
    """An annotation of the planted metagenome of ``test_motif_gc_host``: (contig, start, end, class, strand, id) in file order —
    overlapping classes, both strands and an unstranded interval, an interval whose upstream is clipped at 0 and one clipped at L, and
    one on a contig the assembly does not hold."""
    length = {n: len(mg.contig_str(i)) for i, n in enumerate(mg.names)}
    return [("n1", 20, 9000, "prophage", "+", "ph1"), ("n1", 8000, 12000, "gene", "-", "g1"), ("c1", 0, 500, "gene", "+", "g2"),
            ("c1", 19000, length["c1"], "gene", "-", "g3"), ("n2", 100, 30000, "prophage", ".", "ph2"), ("elsewhere", 5, 50, "gene", "+", "g4"),
            ("c2", 1000, 1031, "repeat", "+", "r1"), ("n2", 31000, 31064, "repeat", "-", "r2"), ("n1", 30000, 30010, "gene", "+", "g5")]


def expected_command_files(mg, cands, rows, upstream):
    """The five files: the brute force's tables, records and per-interval counts through the module's formatters."""
    from nanomotif_amd import motif_regions as mr
    from nanomotif_amd.motif_sites import SiteCandidate
    from nanomotif_amd.regions import RegionSet
    from test_motif_gc_host import CANONICAL, piles_of
    targets, piles = piles_of(mg)
    seq = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    bin_names = sorted(set(mg.bin_names))
    contigs = {b: [n for i, n in enumerate(mg.names) if mg.bin_names[i] == b] for b in bin_names}
    engine_names = [n for b in bin_names for n in contigs[b]]             # (only their set and lengths matter below)
    classes = []
    for r in rows:
        if r[3] not in classes:
            classes.append(r[3])
    classes.append("upstream")
    k = len(classes)
    iv = []
    for n, s, e, c, strand, ident in rows:
        if n not in seq:
            continue
        iv.append((n, s, e, classes.index(c), ident))
        up = (max(0, s - upstream), s) if strand == "+" else (e, min(len(seq[n]), e + upstream)) if strand == "-" else None
        if up and up[1] > up[0]:
            iv.append((n, up[0], up[1], k - 1, ident))
    sets = {(n, c): set() for n in seq for c in range(k)}
    for n, s, e, c, _ in iv:
        sets[(n, c)].update(range(s, e))
    known = [c for c in cands if c[2] in targets]
    bg_keys = [(b, mt) for b in bin_names for mt in targets]
    every = [(b, mt, rg.regex_of(m), p) for b, m, mt, p in known] + [(b, mt, CANONICAL[mt], 0) for b, mt in bg_keys]
    rows_of = lambda mt: (lambda n: [(p, "+-".index(s), f) for p, s, f in piles.get((mt, n), [])])
    site_lists = [rg.sites_in([(n, seq[n]) for n in contigs[b]], rows_of(mt), m, p) for b, mt, m, p in every]
    tables = [rg.table_of(sites, contigs[c[0]], sets, k) for c, sites in zip(every, site_lists)]
    results = [(contigs[c[0]], t) for c, t in zip(every, tables)]
    six = lambda sites, names: np.array([[sum(1 for x in sites if x[0] == n and x[2] == s and x[3] == st) for s in (0, 1) for st in (0, 1, 2)] for n in names])
    totals = [(contigs[c[0]], six(sites, contigs[c[0]])) for c, sites in zip(every, site_lists)]
    covered = {n: np.array([len(sets[(n, c)]) for c in range(k)]) for n in seq}
    contig_len = {n: len(s) for n, s in seq.items()}
    sc = [SiteCandidate(*c) for c in known]
    nk = len(known)
    main, per_contig, per_bin = mr.format_files(sc, results[:nk], totals[:nk], bg_keys, results[nk:], classes, covered, contig_len)
    ids = {n: j for j, n in enumerate(engine_names)}
    rec = rg.records_of(site_lists[:nk], ids, sets, k)
    dtype = [("candidate", "u4"), ("contig", "u4"), ("pos", "u4"), ("code", "u1"), ("classes", "u1")]
    sites_text = mr.format_sites(np.array(rec, dtype=dtype), sc, engine_names, classes)
    # the per-interval counts, interval by interval: every site of every candidate of the contig's bin with its position in the interval
    irows = []
    for n, s, e, c, ident in iv:
        for j, (cand, sites) in enumerate(zip(known, site_lists)):
            hit = [x for x in sites if x[0] == n and s <= x[1] < e]
            if hit:
                irows.append([classes[c], ident, n, s, e, cand[0], cand[1], cand[2], cand[3]] +
                             [sum(1 for x in hit if x[2] == st and x[3] == state) for st in (0, 1) for state in (0, 1, 2)])
    from nanomotif_amd.export_run import table_text
    bed_name = {ident: f"{n}:{s}-{e}" for n, s, e, _, _, ident in rows}   # a BED interval is named contig:start-end, its upstream after it
    bed_rows = [r[:1] + [bed_name[r[1]]] + r[2:] for r in irows]
    return (main, per_contig, per_bin, sites_text, table_text(mr.INTERVALS_HEADER, irows)), table_text(mr.INTERVALS_HEADER, bed_rows)


@gpu
def test_command_on_bed_and_gff3(tmp_path, monkeypatch):
    """The command from a fresh process, GFF3 input with the device pileup parser and BED (.gz) input with the host parser: all five
    files byte for byte against the brute force's text, and one warning line for the interval on a contig no bin holds."""
    from nanomotif_amd import motif_regions as mr
    from test_gpu_motif_compare import _run
    from test_gpu_motif_profile import HEAD
    from test_motif_gc_host import PLANTED_CANDS, planted_metagenome
    mg = planted_metagenome()
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    mg.write_bed(tmp + "/pileup.bed")
    open(tmp + "/motifs.tsv", "w").write(HEAD + "".join(f"{b}\t{m}\t{p}\t{mt}\t1\t1\tpalindrome\t\t\t\t\n" for b, m, mt, p in PLANTED_CANDS))
    rows = annotation(mg)
    with gzip.open(tmp + "/regions.bed.gz", "wt") as f:
        f.write("".join(f"{n}\t{s}\t{e}\t{c}\t0\t{strand}\n" for n, s, e, c, strand, _ in rows))
    open(tmp + "/regions.gff3", "w").write("##gff-version 3\n" + "".join(f"{n}\tx\t{c}\t{s + 1}\t{e}\t.\t{strand}\t.\tID={i};Name=y\n" for n, s, e, c, strand, i in rows))
    want, bed_intervals = expected_command_files(mg, PLANTED_CANDS, rows, 50)
    base = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "motifs.tsv", "--upstream", "50", "--region_sites", "--intervals"]
    names = (mr.MAIN_NAME, mr.CONTIGS_NAME, mr.BINS_NAME, mr.SITES_NAME, mr.INTERVALS_NAME)
    for regions, out, host_parser in (("regions.gff3", "gff", "0"), ("regions.bed.gz", "bed", "1")):
        monkeypatch.setenv("NANOMOTIF_HOST_PARSER", host_parser)
        r = _run(tmp, "motif_regions", base + ["--regions", regions, "--out", out])
        assert (r.stdout + r.stderr).count("the assembly's bins do not hold") == 1
        for name, text in zip(names, want):
            got = open(f"{tmp}/{out}/{name}").read()
            assert got == (bed_intervals if out == "bed" and name == mr.INTERVALS_NAME else text), (out, name)
        assert os.path.exists(f"{tmp}/{out}/logs/timings.motif_regions.json")
    assert len(want[3]) > 1000 and want[4].count("\n") > 5
