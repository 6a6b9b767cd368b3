"""GPU: runs of same-state motif sites along contigs (nm_motif_runs_count / nm_motif_runs_sites, ``ScanEngine.motif_run_counts`` /
``motif_runs``, ``nanomotif motif_runs``) against the brute force of ``runs_geometry`` (a regex scan, dense state tables,
``itertools.groupby``: nothing shared with the engine).  Every comparison is an equality.  That the input holds every case it was built
for (``test_motif_runs_host.test_every_planted_case_is_present``) needs no GPU."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import runs_geometry as rn
from nanomotif_amd.motif import Motif

gpu = pytest.mark.gpu
RS = (2, 16, 64)
FIELDS = ("candidate", "contig", "pos", "code", "last", "n_sites")


@pytest.fixture(scope="module")
def engine():
    from nanomotif_amd.engine import ScanEngine
    seqs, _ = rn.geometry()
    eng = ScanEngine()
    eng.upload_assembly(rn.NAMES, [seqs[n] for n in rn.NAMES], [rn.BINS[n] for n in rn.NAMES], bin_names=rn.BIN_NAMES)
    for mt in ("a", "m"):
        eng.upload_pileup(mt, *rn.pileup_arrays(mt))
    yield eng
    eng.close()


def engine_cands(cands):
    return [(Motif(m, i), mt, b) for b, mt, m, i in cands]


def records_as_tuples(batches):
    rec = [sb.records for sb in batches]
    rec = np.concatenate(rec) if rec else np.zeros(0, dtype=[(f, "u4") for f in FIELDS])
    return list(zip(*(rec[f].tolist() for f in FIELDS))) if len(rec) else []


# ------------------------------------------------------------------------------------------------ 1. the count table
@gpu
@pytest.mark.parametrize("nocall_breaks", [False, True])
@pytest.mark.parametrize("r", RS)
def test_every_cell_equals_the_brute_force(engine, r, nocall_breaks):
    cands = rn.candidates()                                               # all widths and both bins interleaved in one call
    want = [rn.expected_table(c, r, nocall_breaks) for c in cands]
    before = engine.stats()["launches"]
    got = engine.motif_run_counts(engine_cands(cands), max_run=r, nocall_breaks=nocall_breaks)
    assert engine.stats()["launches"] - before == 3 + 1                   # one launch per width, and the stitch
    assert len(got) == len(cands)
    for c, (names, t), w in zip(cands, got, want):
        assert names == rn.contigs_of(c[0]) and t.dtype == np.int64 and t.shape == w.shape == (len(names), 3, 3 + r)
        assert np.array_equal(t, w), (r, nocall_breaks, c, np.argwhere(t != w)[:8].tolist())
        if not nocall_breaks:
            assert not t[:, 2, 0].any() and not t[:, 2, 2:].any()         # the nocall row holds its site count only
    split = engine.motif_run_counts(engine_cands(cands), max_run=r, nocall_breaks=nocall_breaks, max_bytes=1)      # one call per candidate
    few = engine.motif_run_counts(engine_cands(cands), max_run=r, nocall_breaks=nocall_breaks, max_bytes=3 * (3 + r) * 8 * 11)
    for a, b, c in zip(got, split, few):
        assert a[0] == b[0] == c[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])


@gpu
def test_reversed_duplicated_and_an_empty_bin(engine):
    cands = rn.candidates()
    want = [rn.expected_table(c, 16, False) for c in cands]
    rev = engine.motif_run_counts(engine_cands(cands[::-1]))
    assert all(np.array_equal(g[1], w) for g, w in zip(rev, want[::-1]))
    order = [4, 4, 0, 11, 4, 9, 0]
    dup = engine.motif_run_counts(engine_cands([cands[j] for j in order]))
    assert all(np.array_equal(d[1], want[j]) for d, j in zip(dup, order))
    three = [cands[2], ("b0_empty", "a", "GATC", 1), cands[7]]
    g3 = engine.motif_run_counts(engine_cands(three))
    assert g3[1][0] == [] and g3[1][1].shape == (0, 3, 19)
    assert np.array_equal(g3[0][1], want[2]) and np.array_equal(g3[2][1], want[7])
    assert engine.motif_run_counts([]) == [] and list(engine.motif_runs([])) == []
    assert records_as_tuples(engine.motif_runs(engine_cands(three), states=("mod", "nomod"), min_run=1)) == rn.expected_records(three, (0, 1), 1)


# ------------------------------------------------------------------------------------------------ 2. identities on the device's results
@gpu
def test_identities(engine):
    cands = rn.candidates()
    ec = engine_cands(cands)
    six = engine.motif_site_counts(ec)
    plain, breaks = engine.motif_run_counts(ec, max_run=16), engine.motif_run_counts(ec, max_run=16, nocall_breaks=True)
    for (_, t), (_, tb), (_, s) in zip(plain, breaks, six):
        for table in (t, tb):
            assert np.array_equal(table[:, :, 3:].sum(axis=2), table[:, :, 0])                 # sum hist == n_runs
            assert np.array_equal(table[:, :, 1], s[:, :3] + s[:, 3:])                         # [s][1] == the sites of motif_site_counts
            assert (table[:, :, 2] <= table[:, :, 1]).all() and ((table[:, :, 0] > 0) == (table[:, :, 2] > 0)).all()
        assert np.array_equal(t[:, :, 1], tb[:, :, 1])                                         # the site counts are equal in both modes
        assert (tb[:, :2, 0] >= t[:, :2, 0]).all()                                             # a nocall site can only cut a run
    for nb, tables, states in ((False, plain, ("mod", "nomod")), (True, breaks, ("mod", "nomod", "nocall"))):
        rec = np.concatenate([sb.records for sb in engine.motif_runs(ec, states=states, min_run=1, nocall_breaks=nb)])
        n_states = len(states)
        assert len(rec) == sum(int(t[:, :n_states, 0].sum()) for _, t in tables)                # every run is a record
        assert int(rec["n_sites"].sum()) == sum(int(t[:, :n_states, 1].sum()) for _, t in tables)
        assert (rec["last"] >= rec["pos"]).all() and (rec["last"] - rec["pos"] + 1 >= rec["n_sites"]).all()


# ------------------------------------------------------------------------------------------------ 3. the records
STATE_SETS = [(False, s) for k in (1, 2) for s in itertools.combinations(("mod", "nomod"), k)] + \
             [(True, s) for k in (1, 2, 3) for s in itertools.combinations(("mod", "nomod", "nocall"), k)]


@gpu
@pytest.mark.parametrize("nocall_breaks,states", STATE_SETS)
def test_records_equal_the_brute_force(engine, nocall_breaks, states):
    """Every non-empty state set at min_run 1, 3 and R + 1 = 17 (65 as well, once): the G = 1 motifs in windows of 1 (a library call per
    record; not at min_run 1), 7 and the default size; the G = 2 and G = 3 motifs and the backgrounds, thousands of runs each, in windows
    of the default size."""
    from nanomotif_amd.engine import SITE_STATES
    codes = [SITE_STATES.index(s) for s in states]
    cands = rn.candidates()
    for group, sizes in ((cands[:4], (1, 7, None)), (cands[4:], (None,))):
        for min_run in (1, 3, 17, 65):
            want = rn.expected_records(group, codes, min_run, nocall_breaks)
            assert len(want) > 0 or min_run >= 17 or states == ("nocall",)
            for max_records in sizes:
                if max_records == 1 and min_run == 1 or min_run == 65 and max_records is not None:
                    continue
                batches = list(engine.motif_runs(engine_cands(group), states=states, min_run=min_run, nocall_breaks=nocall_breaks, max_records=max_records))
                assert all(len(sb.records) <= (max_records or 1 << 60) for sb in batches)
                assert records_as_tuples(batches) == want, (states, nocall_breaks, min_run, max_records)


# ------------------------------------------------------------------------------------------------ 4. refusals
def raw_call(eng, which, b, table, max_run=16, nocall_breaks=0, state_set=2, min_run=3, bins=None, slots=None, rows=None, nulls=(), ctx=True):
    from nanomotif_amd.engine import _ptr
    bins = np.asarray(b.bins if bins is None else bins, np.uint32)
    slots = np.asarray(b.slots if slots is None else slots, np.uint8)
    rows = np.asarray((0, table.shape[0]) if rows is None else rows, np.uint64)
    args = [_ptr(bins, C.c_uint32), _ptr(slots, C.c_uint8), _ptr(b.lens, C.c_uint8), _ptr(b.modpos, C.c_uint8), _ptr(b.offsets, C.c_uint32),
            _ptr(b.masks, C.c_uint8)]
    if which == "count":
        full = args + [max_run, nocall_breaks, _ptr(rows, C.c_uint64), _ptr(table, C.c_int64)]
        fn = eng.lib.nm_motif_runs_count
    else:
        cap = 1 << 16
        keep = [np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(2, np.uint64),
                C.c_uint64(0)]
        full = args + [state_set, min_run, nocall_breaks, 0, cap, _ptr(keep[0], C.c_uint32), _ptr(keep[1], C.c_uint32), _ptr(keep[2], C.c_uint8),
                       _ptr(keep[3], C.c_uint32), _ptr(keep[4], C.c_uint32), _ptr(keep[5], C.c_uint64), C.byref(keep[6])]
        raw_call.kept = keep
        fn = eng.lib.nm_motif_runs_sites
    for j in nulls:
        full[j] = None
    return fn(eng.ctx if ctx else None, 1, *full)


@gpu
@pytest.mark.parametrize("which", ["count", "sites"])
def test_refusals_with_their_text_and_in_order(engine, which):
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.engine import ScanEngine
    cand = ("b1", "a", "GATC", 1)
    want = rn.expected_table(cand, 16, False)
    n_rec = len(rn.expected_records([cand]))
    b = engine.make_batch(engine_cands([cand]))
    far = engine.make_batch([(Motif("A" + "." * 100 + "T", 0), "a", "b1")])
    table = np.zeros(want.shape, np.int64)
    last = lambda: engine.lib.nm_last_error().decode()
    call = lambda **kw: raw_call(engine, which, kw.pop("batch", b), table, **kw)

    def fine():
        table[:] = -1
        assert call() == 0
        if which == "count":
            assert np.array_equal(table, want)
        else:
            assert raw_call.kept[6].value == raw_call.kept[5][1] == n_rec > 0
        table[:] = 0
    fine()
    for k in range(6):
        assert call(nulls=(k,)) == -1 and "NULL" in last(), k
        fine()
    if which == "count":
        for bad in (0, 1, 65, 1000):
            assert call(max_run=bad) == -1 and f"max_run {bad} outside 2..64" in last()
            fine()
        assert call(nulls=(8,)) == -1 and "NULL" in last()               # row_offset
        assert call(rows=(1, 6)) == -1 and "row_offset[0] must be 0" in last()
        fine()
        assert call(rows=(0, want.shape[0] - 1)) == -1 and "row_offset gives" in last()
        assert not table.any()                                            # a refused call has written nothing
        fine()
    else:
        assert call(min_run=0) == -1 and "min_run 0: at least 1" in last()
        fine()
        for bad in (0, 8, 255):
            assert call(state_set=bad) == -1 and f"state_set {bad}" in last()
            fine()
        for bad in (4, 5, 7):
            assert call(state_set=bad) == -1 and "nocall_breaks" in last()
            fine()
            assert call(state_set=bad, nocall_breaks=1) == 0
        assert call(nulls=(16,)) == -1 and "NULL" in last()              # cand_offset
        assert call(min_run=0, state_set=0) == -1 and "min_run" in last()    # min_run before state_set
        fine()
    own = dict(max_run=1) if which == "count" else dict(state_set=0)
    word = "max_run" if which == "count" else "state_set"
    # the order: NULL, the unit's own arguments, ctx, assembly, then the candidate's bin, slot, program
    assert call(nulls=(2,), **own) == -1 and "NULL" in last()
    assert call(ctx=False, **own) == -1 and word in last()
    assert call(ctx=False) == -1 and "ctx is NULL" in last()
    assert call(bins=[7], **own) == -1 and word in last()
    fine()
    assert call(bins=[7]) == -1 and "cand_bin 7" in last() and "candidate 0" in last()
    fine()
    assert call(slots=[5]) == -3 and "cand_mod_slot[0]" in last()
    fine()
    assert call(batch=far) == -5
    fine()
    # a candidate wrong twice gives nm_motif_sites_count's own message
    assert call(bins=[7], batch=far) == -1
    mine = last()
    assert call(slots=[5], batch=far) == -3
    mine_slot = last()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rows, tot, six = np.zeros(2, np.uint64), np.zeros(1, np.uint64), np.zeros((8, 6), np.int64)
    rows[1] = 5
    for bins, slots, text in (([7], far.slots, mine), (far.bins, [5], mine_slot)):
        assert engine.lib.nm_motif_sites_count(engine.ctx, 1, p(np.asarray(bins, np.uint32), C.c_uint32), p(np.asarray(slots, np.uint8), C.c_uint8), p(far.lens, C.c_uint8),
                                               p(far.modpos, C.c_uint8), p(far.offsets, C.c_uint32), p(far.masks, C.c_uint8), 7, p(rows, C.c_uint64),
                                               p(tot, C.c_uint64), p(six, C.c_int64)) != 0
        assert last() == text
    fine()
    bare = ScanEngine()
    assert raw_call(bare, which, b, table) == -3 and "nm_upload_contigs" in last()
    assert raw_call(bare, which, b, table, **own) == -1 and word in last()
    bare.close()
    fine()
    # through the engine
    with pytest.raises(ValueError):
        engine.motif_run_counts(engine_cands([cand]), max_run=65)
    with pytest.raises(ValueError):
        list(engine.motif_runs(engine_cands([cand]), states=("nocall",)))
    with pytest.raises(ValueError):
        list(engine.motif_runs(engine_cands([cand]), min_run=0))
    with pytest.raises(NmScanError) as err:
        engine.motif_run_counts([(Motif("A" + "." * 100 + "T", 0), "a", "b1")])
    assert err.value.code == -5
    fine()
    rows0 = np.zeros(1, np.uint64)
    off, written = np.ones(1, np.uint64), C.c_uint64(9)
    assert engine.lib.nm_motif_runs_count(engine.ctx, 0, None, None, None, None, None, None, 16, 0, p(rows0, C.c_uint64), None) == 0
    assert engine.lib.nm_motif_runs_sites(engine.ctx, 0, None, None, None, None, None, None, 2, 3, 0, 0, 0, None, None, None, None, None, p(off, C.c_uint64),
                                          C.byref(written)) == 0 and off[0] == 0 and written.value == 0


# ------------------------------------------------------------------------------------------------ 5. the command
def expected_command_files(mg, cands, max_run, nocall_breaks, states, min_run):
    """The five files: the brute force's tables and records through the module's formatters."""
    from nanomotif_amd import motif_runs as mr
    from nanomotif_amd.motif_sites import SiteCandidate
    from regions_geometry import regex_of
    from test_motif_gc_host import CANONICAL, piles_of
    targets, piles = piles_of(mg)
    seq = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    bin_names = sorted(set(mg.bin_names))
    contigs = {b: [n for i, n in enumerate(mg.names) if mg.bin_names[i] == b] for b in bin_names}
    names = [n for b in bin_names for n in contigs[b]]
    known = [c for c in cands if c[2] in targets]
    bg_keys = [(b, mt) for b in bin_names for mt in targets]
    every = [(b, mt, regex_of(m), p) for b, m, mt, p in known] + [(b, mt, CANONICAL[mt], 0) for b, mt in bg_keys]
    rows_of = lambda mt: (lambda n: [(p, "+-".index(s), f) for p, s, f in piles.get((mt, n), [])])
    site_lists = [rn.sites_in([(n, seq[n]) for n in contigs[b]], rows_of(mt), m, p) for b, mt, m, p in every]
    results = [(contigs[c[0]], rn.count_table(sites, contigs[c[0]], max_run, nocall_breaks)) for c, sites in zip(every, site_lists)]
    sc = [SiteCandidate(*c) for c in known]
    nk = len(known)
    texts = mr.format_files(sc, results[:nk], bg_keys, results[nk:])
    from nanomotif_amd.engine import RUN_DTYPE, SITE_STATES
    rec = rn.run_records(site_lists[:nk], [contigs[c[0]] for c in every[:nk]], {n: j for j, n in enumerate(names)}, [SITE_STATES.index(s) for s in states], min_run,
                         nocall_breaks)
    return texts + (mr.format_runs(np.array(rec, dtype=RUN_DTYPE), sc, names),)


@gpu
def test_command_files_byte_for_byte(tmp_path):
    """The command from a fresh process, defaults and every option: the five files against the brute force's text."""
    from nanomotif_amd import motif_runs as mr
    from test_gpu_motif_compare import _run
    from test_gpu_motif_profile import HEAD
    from test_motif_gc_host import PLANTED_CANDS, planted_metagenome
    mg = planted_metagenome()
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    mg.write_bed(tmp + "/pileup.bed")
    open(tmp + "/motifs.tsv", "w").write(HEAD + "".join(f"{b}\t{m}\t{p}\t{mt}\t1\t1\tpalindrome\t\t\t\t\n" for b, m, mt, p in PLANTED_CANDS))
    base = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "motifs.tsv"]
    names = (mr.MAIN_NAME, mr.CONTIGS_NAME, mr.HIST_NAME, mr.BINS_NAME, mr.BED_NAME)
    runs = (("plain", ["--runs", "--states", "mod,nomod", "--min_run", "2"], (16, False, ("mod", "nomod"), 2)),
            ("breaks", ["--runs", "--nocall_breaks", "--max_run", "5", "--states", "nocall,mod", "--min_run", "1"], (5, True, ("mod", "nocall"), 1)))
    for out, options, spec in runs:
        want = expected_command_files(mg, PLANTED_CANDS, *spec)
        _run(tmp, "motif_runs", base + options + ["--out", out])
        for name, text in zip(names, want):
            assert open(f"{tmp}/{out}/{name}").read() == text, (out, name)
        assert len(want[4]) > 1000 and want[2].count("\n") > 10
        assert os.path.exists(f"{tmp}/{out}/logs/timings.motif_runs.json")
