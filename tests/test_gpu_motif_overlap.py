"""GPU: shared sites and nesting between the motifs of a bin (nm_motif_overlap_count, ``ScanEngine.motif_overlap``, ``nanomotif
motif_overlap``) against the brute force of ``overlap_geometry`` (Python sets over a regex scan, nothing shared with the engine).  Counts
are integers: every comparison is an equality over the WHOLE table of every candidate.  The conditions on the input
(``test_motif_overlap_host.test_the_input_has_what_the_checks_need``) need no GPU.

Refusal order pinned here, per candidate: bin, mod slot, partner prefix, P above NM_OVERLAP_MAX_PARTNERS, the partners' programs in
order, the candidate's own program, rows."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import overlap_geometry as G
from nanomotif_amd.motif import Motif
from test_gpu_motif_compare import _body, _filtered_piles, _run
from test_gpu_motif_profile import HEAD

pytestmark = pytest.mark.gpu
BIN_NAMES = ["b0", "empty", "b1"]                                        # a bin without a contig between the two others
MAX_PARTNERS = 4095


@pytest.fixture(scope="module")
def brute():
    return G.BruteForce()


@pytest.fixture(scope="module")
def engine(brute):
    from nanomotif_amd.engine import ScanEngine
    eng = ScanEngine(0)
    eng.upload_assembly(G.NAMES, [brute.seqs[n] for n in G.NAMES], [G.BIN_OF[n] for n in G.NAMES], bin_names=BIN_NAMES)
    for mt in "am":
        eng.upload_pileup(mt, *brute.rows[mt])
    assert eng.slot_of_mod == {"a": 0, "m": 1} and [eng.bin_contigs(b) for b in BIN_NAMES] == [["short", "long"], [], ["mid"]]
    yield eng
    eng.close()


def mot(m):
    return Motif(*m)


def whole_sets():
    """Every motif of every set with all other motifs of its set as partners, the mod types and bins interleaved: (bin, mod type,
    owner, partners) in call order."""
    per = {(b, mt): [(b, mt, m, G.SETS[mt][:i] + G.SETS[mt][i + 1:]) for i, m in enumerate(G.SETS[mt])] for b in G.BINS for mt in "am"}
    order = [("b0", "a"), ("b1", "m"), ("b1", "a"), ("b0", "m")]
    out = []
    for row in itertools.zip_longest(*(per[k] for k in order)):
        out += [c for c in row if c is not None]
    return out


def run(eng, calls, **kw):
    return list(eng.motif_overlap([(mot(m), mt, b) for b, mt, m, _ in calls], [[mot(p) for p in ps] for _, _, _, ps in calls], **kw))


def check(got, calls, brute):
    assert len(got) == len(calls)
    for (names, t), (b, mt, m, ps) in zip(got, calls):
        want = brute.table(b, mt, m, ps)
        assert names == G.CONTIGS[b] and t.dtype == np.int64 and t.shape == want.shape == (len(ps) + 2, len(names), 2, 3), (b, mt, m)
        assert np.array_equal(t, want), (b, mt, m, ps, np.argwhere(t != want)[:5].tolist())


# ------------------------------------------------------------------------------------------------ 1. the full table
def test_full_table_equals_the_brute_force(engine, brute):
    """Every candidate x every other motif of its set, both mod types and both bins interleaved in one call; then every ordered pair
    with ONE partner, which runs owners of G = 1 beside partners of G = 2 and 3 and the reverse at the pair's own width."""
    calls = whole_sets()
    assert [c[:2] for c in calls[:4]] == [("b0", "a"), ("b1", "m"), ("b1", "a"), ("b0", "m")] and len(calls) == 26
    before = engine.stats()["launches"]
    got = run(engine, calls)
    assert engine.stats()["launches"] - before == 2                       # the `a` sets run at G = 3 (GATC.{70}T among them), the `m` sets at G = 1
    check(got, calls, brute)
    again = run(engine, calls)                                            # no stale counters in the table
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(got, again))
    pairs = [(b, mt, G.SETS[mt][i], [G.SETS[mt][j]]) for mt, b in (("a", "b0"), ("m", "b1"), ("a", "b1")) for i, j in itertools.permutations(range(len(G.SETS[mt])), 2)]
    pairs = pairs[::2] + pairs[1::2]
    before = engine.stats()["launches"]
    got = run(engine, pairs)
    assert engine.stats()["launches"] - before == 3                       # all three widths in one call
    check(got, pairs, brute)
    by_key = {(b, mt, m, ps[0]): t for (_, t), (b, mt, m, ps) in zip(got, pairs)}
    for (b, mt, m, p), t in by_key.items():                               # pair(i, j) == pair(j, i), whatever the widths
        assert np.array_equal(t[1], by_key[(b, mt, p, m)][1]), (b, mt, m, p)
        assert np.array_equal(t[0], t[1] + t[2])                          # own = shared + rest with one partner
    g1, g3 = G.A_SET[0], G.A_SET[5]
    assert by_key[("b0", "a", g1, g3)][1].sum() == by_key[("b0", "a", g3, g1)][0].sum() > 0


# ------------------------------------------------------------------------------------------------ 2. identities
def test_identities_on_the_device_results(engine, brute):
    calls = whole_sets()
    got = run(engine, calls)
    own = engine.motif_site_counts([(mot(m), mt, b) for b, mt, m, _ in calls])
    for (names, t), (names6, six) in zip(got, own):                       # block 0 is the row of motif_site_counts
        assert names == names6 and np.array_equal(t[0].reshape(len(names), 6), six)
    # the rest with all others as partners is the exclusive table of motif_coverage on the same set
    for b, mt in itertools.product(G.BINS, "am"):
        cov = engine.motif_coverage([(b, mt, [mot(m) for m in G.SETS[mt]])])[0][2]
        mine = [t for (_, t), c in zip(got, calls) if c[:2] == (b, mt)]
        assert len(cov) == len(mine)
        for excl, t in zip(cov, mine):
            assert np.array_equal(t[-1][:, :, :2].reshape(-1, 4), excl), (b, mt)
    gatc, cc = G.A_SET[0], G.M_SET[0]
    special = [("b0", "a", gatc, [gatc]), ("b1", "a", gatc, []), ("b0", "m", cc, G.M_SET[1:]), ("b1", "m", cc, G.M_SET[1:]), ("b0", "a", gatc, [G.A_SET[9], G.A_SET[7]]),
               ("b0", "a", G.A_SET[5], [G.A_SET[5], gatc])]
    res = run(engine, special)
    check(res, special, brute)
    t = res[0][1]
    assert np.array_equal(t[1], t[0]) and not t[2].any() and t[0].sum() > 0                 # partner == owner
    assert res[1][1].shape[0] == 2 and np.array_equal(res[1][1][1], res[1][1][0])           # P = 0: the rest is block 0
    assert not res[2][1][-1].any() and not res[3][1][-1].any() and res[2][1][1].sum() and res[2][1][2].sum()   # two children that partition
    t = res[4][1]
    assert np.array_equal(t[1], t[0]) and np.array_equal(t[2], t[0]) and not t[3].any()      # the other spellings are identical
    t = res[5][1]
    assert np.array_equal(t[1], t[0]) and np.array_equal(t[2], t[0]) and not t[3].any()      # a G = 3 owner inside its G = 1 parent


def test_the_result_does_not_depend_on_max_bytes(engine, brute):
    calls = whole_sets()
    before = engine.stats()["launches"]
    single = run(engine, calls, max_bytes=1)
    assert engine.stats()["launches"] - before == len(calls)             # one candidate per call: one launch each
    whole = run(engine, calls, max_bytes=1 << 40)
    some = run(engine, calls, max_bytes=12 * 2 * 48 * 3 + 1)             # groups that end inside a set
    check(single, calls, brute)
    for a, b, c in zip(single, whole, some):
        assert a[0] == b[0] == c[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
    with pytest.raises(ValueError):
        run(engine, calls, max_bytes=0)
    with pytest.raises(ValueError):
        list(engine.motif_overlap([(mot(G.A_SET[0]), "a", "b0")], []))
    with pytest.raises(ValueError):
        list(engine.motif_overlap([(mot(G.A_SET[0]), "a", "b0")], [[mot(G.A_SET[1])] * (MAX_PARTNERS + 1)]))


def test_a_bin_without_a_contig_and_an_empty_call(engine, brute):
    assert list(engine.motif_overlap([], [])) == []
    gatc = G.A_SET[0]
    before = engine.stats()["launches"]
    alone = run(engine, [("empty", "a", gatc, [G.A_SET[1]])])
    assert engine.stats()["launches"] == before and alone[0][0] == [] and alone[0][1].shape == (3, 0, 2, 3)
    three = [("empty", "a", gatc, G.A_SET[1:3]), ("b1", "m", G.M_SET[0], G.M_SET[1:]), ("empty", "m", G.M_SET[0], []), ("b0", "a", G.A_SET[4], [gatc])]
    res = run(engine, three)
    assert res[0][1].shape == (4, 0, 2, 3) and res[2][1].shape == (2, 0, 2, 3)
    for k in (1, 3):
        assert np.array_equal(res[k][1], brute.table(*three[k]))
    rows = np.zeros(1, np.uint64)
    off = np.zeros(1, np.uint32)
    assert engine.lib.nm_motif_overlap_count(engine.ctx, 0, None, None, None, None, None, None, off.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, None,
                                             rows.ctypes.data_as(C.POINTER(C.c_uint64)), None) == 0


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_are_loud_in_one_order_and_leave_the_engine_usable(engine, brute):
    from nanomotif_amd.engine import _ptr
    eng = engine
    gatc, rgatcy, g70 = G.A_SET[0], G.A_SET[1], G.A_SET[5]
    want = np.concatenate([brute.table("b0", "a", gatc, [rgatcy, g70]).reshape(-1, 2, 3), brute.table("b1", "a", rgatcy, [gatc]).reshape(-1, 2, 3)])
    b = eng.make_batch([(mot(gatc), "a", "b0"), (mot(rgatcy), "a", "b1")])
    pb = eng.make_batch([(mot(m), 0, 0) for m in (rgatcy, g70, gatc)], slot_of=lambda mt: 0)
    far = eng.make_batch([(mot(gatc), "a", "b0"), (Motif("A" + "." * 100 + "T", 0), "a", "b1")])   # beyond the reach limit
    n_rows = len(want)
    assert n_rows == 4 * 2 + 3 * 1
    counts = np.zeros((n_rows, 2, 3), np.int64)
    u8, u32, u64 = C.c_uint8, C.c_uint32, C.c_uint64

    def call(bins=b.bins, slots=b.slots, batch=b, off=(0, 2, 3), plens=pb.lens, rows=(0, 8, 11), nulls=()):
        bins, slots, off, plens, rows = np.asarray(bins, np.uint32), np.asarray(slots, np.uint8), np.asarray(off, np.uint32), np.asarray(plens, np.uint8), np.asarray(rows, np.uint64)
        args = [_ptr(bins, u32), _ptr(slots, u8), _ptr(batch.lens, u8), _ptr(batch.modpos, u8), _ptr(batch.offsets, u32), _ptr(batch.masks, u8), _ptr(off, u32),
                _ptr(plens, u8), _ptr(pb.modpos, u8), _ptr(pb.offsets, u32), _ptr(pb.masks, u8), _ptr(rows, u64), _ptr(counts, C.c_int64)]
        for j in nulls:
            args[j] = None
        return eng.lib.nm_motif_overlap_count(eng.ctx, 2, *args)
    last = lambda: eng.lib.nm_last_error().decode()

    def fine():
        counts[:] = -1
        assert call() == 0 and np.array_equal(counts, want)
        counts[:] = 0
    fine()
    launches = eng.stats()["launches"]

    def refused(code, *words, **kw):
        assert call(**kw) == code, (kw, last())
        assert all(w in last() for w in words), (kw, last())
        assert not counts.any() and eng.stats()["launches"] == launches, kw   # refused on the host: nothing launched, nothing written
    refused(-1, "candidate 1", "cand_bin", bins=[0, 7])                   # bad bin
    refused(-3, "cand_mod_slot[1]", slots=[0, 5])                         # absent mod slot: NM_ESTATE
    refused(-1, "candidate 1", "descends", off=(0, 2, 1))                 # descending partner prefix
    refused(-1, "cand_partner_offset[0] must be 0", off=(1, 2, 3))
    refused(-1, "candidate 0", "4096 partners", "NM_OVERLAP_MAX_PARTNERS", off=(0, 4096, 4097))
    refused(-5, "candidate 0", "partner 1", "length 0", plens=[pb.lens[0], 0, pb.lens[2]])           # NM_ERANGE
    refused(-5, "candidate 1", "partner 0", "length 200", plens=[pb.lens[0], pb.lens[1], 200])      # beyond NM_MAX_MOTIF_LEN = 191
    refused(-5, batch=far)                                                # the candidate's own program
    refused(-1, "candidate 1", "row_offset", rows=(0, 8, 10))             # too few rows
    refused(-1, "candidate 0", "row_offset", rows=(0, 7, 11))
    for j in (0, 1, 2, 3, 4, 5, 6, 11, 12):
        refused(-1, "NULL", nulls=(j,))
    for j in (7, 8, 9, 10):                                               # a partner array: looked at when a candidate has partners
        refused(-1, "NULL", "partners", nulls=(j,))
    launches_now = eng.stats()["launches"]
    assert launches_now == launches
    fine()
    launches = eng.stats()["launches"]
    # a candidate wrong in two ways is refused in the pinned order
    refused(-1, "cand_bin", bins=[0, 7], slots=[0, 5])                    # bin before slot
    refused(-3, "cand_mod_slot[1]", slots=[0, 5], off=(0, 2, 1))          # slot before the partner prefix
    refused(-1, "descends", off=(0, 2, 1), plens=[pb.lens[0], pb.lens[1], 0])   # prefix before the partners' programs
    refused(-1, "4096 partners", off=(0, 2, 4098), batch=far)             # P before any program
    refused(-5, "partner 0", "length 0", plens=[pb.lens[0], pb.lens[1], 0], batch=far)   # the partners' programs before the candidate's own
    refused(-5, "offset", batch=far, rows=(0, 8, 8))                      # the candidate's program before its rows
    refused(-1, "candidate 0", "row_offset", rows=(0, 7, 11), bins=[0, 7])   # candidate 0 is refused before candidate 1 is looked at
    fine()
    # no assembly
    from nanomotif_amd.engine import ScanEngine
    bare = ScanEngine(0)
    ctx, eng.ctx = eng.ctx, bare.ctx
    try:
        assert call() == -3 and "nm_upload_contigs" in last() and not counts.any()
    finally:
        eng.ctx = ctx
        bare.close()
    fine()


# ------------------------------------------------------------------------------------------------ 4. the command
CARRIED_BIN, ALL_BIN = "bin_carried", "bin_all"
COMMAND_CANDS = [(CARRIED_BIN, "GATC", "a", 1), (CARRIED_BIN, "RGATCY", "a", 2), (CARRIED_BIN, "GTAC", "a", 2), (ALL_BIN, "GATC", "a", 1), (ALL_BIN, "RGATCY", "a", 2),
                 (ALL_BIN, "CTAG", "a", 2), (ALL_BIN, "CCWGG", "m", 1), ("bin_nowhere", "GATC", "a", 1)]


def planted():
    """Two bins of two contigs: in ``bin_carried`` only RGATCY is methylated, in ``bin_all`` every GATC; CCWGG (5mC) in both."""
    from nanomotif_amd import synth
    rng = np.random.default_rng(811)
    names = ["k1", "a1", "k2", "a2"]
    bins = [CARRIED_BIN, ALL_BIN, CARRIED_BIN, ALL_BIN]
    seqs = ["".join(rng.choice(list("ACGT"), size=n)) for n in (30_000, 25_000, 21_111, 17_001)]
    mg = synth.from_sequences(names, seqs, bins, [("CCWGG", 1, "m")], seed=5, mod_types=("a", "m"))
    mg.bin_motifs[CARRIED_BIN] = [("RGATCY", 2, "a"), ("CCWGG", 1, "m")]
    mg.bin_motifs[ALL_BIN] = [("GATC", 1, "a"), ("CCWGG", 1, "m")]
    return mg


def expected_texts(mg, cands, all_pairs=False, **kw):
    """Both files from the host formatters fed with the brute force over the pre-filtered pileup."""
    from nanomotif_amd import motif_overlap as MO
    from nanomotif_amd.motif import iupac_to_regex
    from nanomotif_amd.motif_coverage import build_sets
    from nanomotif_amd.motif_sites import SiteCandidate
    from nanomotif_amd.pileup import MOD_TYPES
    from oracle.scan import split_positions
    piles = _filtered_piles(mg)
    seqs = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    mod_types = [mt for mt in MOD_TYPES if piles[mt]]
    states = {}
    for mt in mod_types:
        states[mt] = {}
        for n in mg.names:
            st = np.full((2, len(seqs[n])), 2, np.uint8)
            if n in piles[mt]:
                mf, nf, mr, nr = split_positions(piles[mt][n], 0.3, 0.7)
                st[0, nf], st[1, nr] = 1, 1
                st[0, mf], st[1, mr] = 0, 0                               # a position called both ways is methylated
            states[mt][n] = st
    bins = sorted(set(mg.bin_names))
    bf = G.BruteForce(seqs, states, {b: [n for n, x in zip(mg.names, mg.bin_names) if x == b] for b in bins})
    sets = [s for s in build_sets(bins, mod_types, [SiteCandidate(*c) for c in cands if c[0] in bins and c[2] in mod_types]) if s.candidates]
    stats = []
    for s in sets:
        ms = [(iupac_to_regex(c.motif), c.mod_position) for c in s.candidates]
        st = MO.set_stats(bf.all_others(s.bin, s.mod_type, ms))
        kids = MO.nesting(st)[0]
        MO.add_outside(st, kids, {i: bf.table(s.bin, s.mod_type, ms[i], [ms[j] for j in kids[i]]) for i in range(len(ms)) if kids[i]})
        stats.append(st)
    return MO.format_pairs(sets, stats, all_pairs), MO.format_motifs(sets, stats, **kw)


def _bin_motifs_text(cands):
    return HEAD + "".join(f"{b}\t{m}\t{p}\t{mt}\t1\t1\tpalindrome\t\t\t\t\n" for b, m, mt, p in cands)


def test_command_on_a_planted_input(tmp_path):
    from nanomotif_amd.motif_overlap import MOTIFS_HEADER, MOTIFS_NAME, PAIRS_HEADER, PAIRS_NAME
    mg = planted()
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    mg.write_bed(tmp + "/pileup.bed")
    cands = COMMAND_CANDS + [(ALL_BIN, "GATC", "21839", 1)]
    open(tmp + "/motifs.tsv", "w").write(_bin_motifs_text(cands[:4]))
    open(tmp + "/more.tsv", "w").write(_bin_motifs_text(cands[3:]))      # the fourth row again: a repeat is dropped
    base = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "motifs.tsv", "more.tsv"]
    r = _run(tmp, "motif_overlap", base + ["--out", "ov"])
    log = r.stdout + r.stderr
    assert "the pileup holds no rows of mod type 21839" in log and "the bin has no contig in the assembly" in log and "skipped" in log
    pairs, motifs = expected_texts(mg, cands)
    assert open(f"{tmp}/ov/{PAIRS_NAME}").read() == pairs and open(f"{tmp}/ov/{MOTIFS_NAME}").read() == motifs
    head, body = _body(f"{tmp}/ov/{MOTIFS_NAME}")
    assert head == MOTIFS_HEADER
    flags = {tuple(row[:4]): row[-1] for row in body}
    assert flags == {(ALL_BIN, "a", "GATC", "1"): "none", (ALL_BIN, "a", "RGATCY", "2"): "submotif", (ALL_BIN, "a", "CTAG", "2"): "none",
                     (ALL_BIN, "m", "CCWGG", "1"): "none", (CARRIED_BIN, "a", "GATC", "1"): "carried_by_children",
                     (CARRIED_BIN, "a", "RGATCY", "2"): "none", (CARRIED_BIN, "a", "GTAC", "2"): "none"}
    head, body = _body(f"{tmp}/ov/{PAIRS_NAME}")
    assert head == PAIRS_HEADER and [row[-2:] for row in body] == [["b_in_a", "b_in_a"]] * 2 and {row[0] for row in body} == {ALL_BIN, CARRIED_BIN}
    assert os.path.exists(f"{tmp}/ov/args.motif_overlap.json") and os.path.exists(f"{tmp}/ov/logs/timings.motif_overlap.json")
    # --all_pairs adds exactly the disjoint rows; other thresholds reach the flags
    _run(tmp, "motif_overlap", base + ["--out", "ov2", "--all_pairs", "--min_called", "5", "--max_outside", "0.01", "--min_frac", "0.99"])
    pairs2, motifs2 = expected_texts(mg, cands, all_pairs=True, min_called=5, max_outside=0.01, min_frac=0.99)
    assert open(f"{tmp}/ov2/{PAIRS_NAME}").read() == pairs2 and open(f"{tmp}/ov2/{MOTIFS_NAME}").read() == motifs2
    _, body2 = _body(f"{tmp}/ov2/{PAIRS_NAME}")
    added = [row for row in body2 if row not in body]
    assert len(body2) == len(body) + 4 and [row for row in body2 if row in body] == body and all(row[-2] == "disjoint" for row in added)
    assert motifs2 != motifs
