"""What the eight export units share (csrc/nmexport.h), checked across them on one small engine: (a) they find ONE set of occurrences —
per candidate, contig and strand the same number as a regex scan of the contigs on the host, and the same mod / nomod / nocall split
wherever a unit reports one; (b) they refuse a wrong candidate with the same code, before any launch, and stay usable.  Every comparison
is an equality."""
import ctypes as C
import re

import numpy as np
import pytest

import test_read_methylation_host as H
from nanomotif_amd.motif import Motif
from test_gpu_motif_compare import reach_class
from test_gpu_motif_fractions import _upload

pytestmark = pytest.mark.gpu
NM_OK, NM_EINVAL, NM_ESTATE, NM_ERANGE = 0, -1, -3, -5
BORDER = 8192                                                            # a work item covers 8 192 bp of a contig
NAMES = ["short", "mid", "long"]
LENGTHS = {"short": 300, "mid": 9_000, "long": 17_000}
BIN_OF = {"short": "b0", "mid": "b1", "long": "b0"}
# one motif per width class: the last literal lies 3, 43 and 73 positions from the modified base
MOTIFS = [("GATC", 1), ("GATC" + "." * 40 + "T", 1), ("GATC" + "." * 70 + "T", 1)]
# (motif, mod position, mod type, bin): the bins alternate inside every width class, so no class's owner list is 0, 1, 2, ...
CANDS = [(m, p, "am"[(i + j) % 2], ("b0", "b1")[j]) for i, (m, p) in enumerate(MOTIFS) for j in range(2)]
WINDOW, RADIUS, FBINS, CAP = 1024, 2, 4, 64
COMP = str.maketrans("ACGT", "TGCA")


def sequences():
    """Random contigs with GATC planted every 470 bp, across 8 191 | 8 192 and on the last four bases, a T 44 and 74 bp after each."""
    rng = np.random.default_rng(19)
    seqs = {}
    for name in NAMES:
        L = LENGTHS[name]
        s = rng.choice(list("ACGT"), size=L)
        for q in list(range(40, L - 80, 470)) + ([BORDER - 2] if L > BORDER + 80 else []) + [L - 4]:
            s[q:q + 4] = list("GATC")
            if q + 75 <= L:
                s[q + 44] = s[q + 74] = "T"
        seqs[name] = "".join(s)
    return seqs


def host_occurrences(seq, motif, pos):
    """The '+' coordinates of the modified base of every occurrence of ``motif`` on '+' and on '-' (overlapping ones included)."""
    rx = re.compile("(?=" + motif + ")")
    plus = [m.start() + pos for m in rx.finditer(seq)]
    minus = [len(seq) - 1 - (m.start() + pos) for m in rx.finditer(seq.translate(COMP)[::-1])]
    return plus, minus


def test_the_input_has_what_the_checks_need():
    seqs = sequences()
    assert [reach_class(m, p) for m, p in MOTIFS] == [0, 1, 2]
    for m, p in MOTIFS:
        for name in ("mid", "long"):                                     # an occurrence across the work-item border, on both strands for GATC
            plus, minus = host_occurrences(seqs[name], m, p)
            assert BORDER - 1 in plus and any(q < BORDER for q in plus) and any(q > BORDER for q in plus), (m, name)
            assert minus, (m, name)
        assert host_occurrences(seqs["short"], m, p)[0], m               # and before the contig border inside bin b0
    assert BORDER in host_occurrences(seqs["mid"], "GATC", 1)[1]
    assert [c[3] for c in CANDS] == ["b0", "b1"] * 3 and {c[2] for c in CANDS[::2]} == {"a", "m"}


@pytest.fixture(scope="module")
def shared():
    """Two bins (b0: short, long; b1: mid), one pileup with the mod types a and m (a third of the rows without a call), read
    statistics for a."""
    from nanomotif_amd.engine import ScanEngine
    seqs = sequences()
    eng = ScanEngine(0)
    eng.upload_assembly(NAMES, [seqs[n] for n in NAMES], [BIN_OF[n] for n in NAMES], bin_names=["b0", "b1"])
    rng = np.random.default_rng(23)
    records = {}
    for mt in "am":
        cid, pos, strand, frac = [], [], [], []
        for i, name in enumerate(NAMES):
            for s in (H.PLUS, H.MINUS):
                p = np.flatnonzero(rng.random(LENGTHS[name]) < 0.7)
                cid.append(np.full(len(p), i)); pos.append(p); strand.append(np.full(len(p), s, np.uint8))
                frac.append(rng.choice([0.95, 0.05, 0.5], size=len(p)))
                if mt == "a":
                    r = records.setdefault((name, "a"), {k: [] for k in ("position", "strand", "n_valid", "n_mod", "n_diff")})
                    r["position"].append(p[::2]); r["strand"].append(np.full(len(p[::2]), s, np.uint8))
                    r["n_valid"].append(np.full(len(p[::2]), 10)); r["n_mod"].append(rng.integers(0, 11, len(p[::2]))); r["n_diff"].append(np.zeros(len(p[::2]), np.int64))
        eng.upload_pileup(mt, *(np.concatenate(x) for x in (cid, pos, strand, frac)))
    _upload(eng, NAMES, {k: {f: np.concatenate(v) for f, v in r.items()} for k, r in records.items()}, codes=("a",))
    assert eng.slot_of_mod == {"a": 0, "m": 1} and eng.readstats_mods == {"a"}
    yield dict(eng=eng, seqs=seqs)
    eng.close()


def engine_cands(cands=CANDS):
    return [(Motif(m, p), mt, b) for m, p, mt, b in cands]


# ------------------------------------------------------------------------------------------------ (a) one occurrence set
def test_every_unit_finds_the_same_occurrences_in_the_same_states(shared):
    eng, seqs = shared["eng"], shared["seqs"]
    ecands = engine_cands()
    contigs = {b: [n for n in NAMES if BIN_OF[n] == b] for b in ("b0", "b1")}
    host = [np.array([[len(x) for x in host_occurrences(seqs[n], m, p)] for n in contigs[b]]) for m, p, _, b in CANDS]
    sites = eng.motif_site_counts(ecands)
    six = [t.reshape(-1, 2, 3) for _, t in sites]                        # [contig][strand][mod, nomod, nocall]
    for k, c in enumerate(CANDS):
        assert sites[k][0] == contigs[c[3]], c
        assert np.array_equal(six[k].sum(axis=2), host[k]), ("sites", c, six[k].sum(axis=2).tolist(), host[k].tolist())
        assert host[k].sum(axis=0).min() > 0, c                          # occurrences on both strands
    assert sum(s.sum(axis=(0, 1)) for s in six).min() > 0                # all three states are there
    tracks = list(eng.motif_tracks(ecands, window=WINDOW))
    states, _ = eng.motif_context(ecands, radius=RADIUS)
    _, psites, _ = eng.motif_profile(ecands, radius=RADIUS)
    fractions = list(eng.motif_fractions([(mo, "a", b) for mo, _, b in ecands], bins=FBINS))
    strands = eng.motif_strand_counts([(mo, mt, b, len(mo.tokens) - 1 - mo.mod_position) for mo, mt, b in ecands])   # partner offset 0
    compare = eng.motif_compare_counts(ecands, lambda mt: (mt, mt))
    assert len(tracks) == len(fractions) == len(strands) == len(compare) == len(CANDS)
    for k, c in enumerate(CANDS):
        names, prefix, windows = tracks[k]
        per_contig = np.array([windows[int(prefix[i]):int(prefix[i + 1])].sum(axis=0) for i in range(len(names))]).reshape(-1, 2, 3)
        assert names == contigs[c[3]] and np.array_equal(per_contig, six[k]), ("tracks", c)
        assert np.array_equal(states[k], six[k].sum(axis=0)), ("context", c)
        assert np.array_equal(psites[k], host[k].sum(axis=0)), ("profile", c)
        assert fractions[k][1] == contigs[c[3]] and np.array_equal(fractions[k][2][:, :, FBINS].astype(np.int64), host[k]), ("fractions", c)
        pairs = strands[k][1].reshape(-1, 2, 3, 3)                       # [contig][strand][own state][partner state]
        assert np.array_equal(pairs.sum(axis=3), six[k]), ("strands", c)
        trans = compare[k][1].reshape(-1, 2, 3, 3)                       # a sample against itself: nothing off the diagonal
        assert np.array_equal(np.einsum("csii->csi", trans), six[k]) and trans.sum() == six[k].sum(), ("compare", c)


# ------------------------------------------------------------------------------------------------ (b) one refusal order
def entry_points(eng, rows, wrows):
    """name -> f(d) -> (return code, the arrays the call fills) for the twelve entry points; ``d``: the arguments by name
    (``arguments``).  ``rows`` / ``wrows``: the prefixes of the (candidate, contig) and (candidate, window) rows of the valid call."""
    from nanomotif_amd.engine import _ptr
    lib, u8, u32, u64, i64 = eng.lib, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int64
    n_rows, n_wrows = int(rows[-1]), int(wrows[-1])
    motif = lambda d: (_ptr(d["lens"], u8), _ptr(d["modpos"], u8), _ptr(d["offsets"], u32), _ptr(d["masks"], u8))
    head = lambda d: (d["ctx"], len(d["bins"]), _ptr(d["bins"], u32))

    def window(n):                                                       # the trailing arguments of a *_sites call, and what it fills
        out = [np.zeros(CAP, np.uint32), np.zeros(CAP, np.uint32), np.zeros(CAP, np.uint8), np.zeros(n + 1, np.uint64), np.zeros(1, np.uint64)]
        return (0, CAP, _ptr(out[0], u32), _ptr(out[1], u32), _ptr(out[2], u8), _ptr(out[3], u64), _ptr(out[4], u64)), out

    def counted(call, d, lead, selection, width):                        # sites / compare / strands *_count
        out = [np.zeros(len(d["bins"]), np.uint64), np.zeros((n_rows, width), np.int64)]
        return call(*head(d), *lead, *motif(d), selection, _ptr(rows, u64), _ptr(out[0], u64), _ptr(out[1], i64)), out

    def recorded(call, d, lead, selection):                              # sites / compare / strands *_sites
        tail, out = window(len(d["bins"]))
        return call(*head(d), *lead, *motif(d), selection, *tail), out

    slot = lambda d: (_ptr(d["slots"], u8),)
    two = lambda d: (_ptr(d["slots"], u8), _ptr(d["slots_b"], u8))
    partner = lambda d: (_ptr(d["slots"], u8), _ptr(d["partner"], C.c_int8))
    sets = lambda d: (_ptr(d["slots"], u8), _ptr(np.arange(len(d["bins"]) + 1, dtype=np.uint32), u32))   # every candidate a set of its own

    def coverage_count(d):
        n = len(d["bins"])
        out = [np.zeros(n, np.uint64), np.zeros((n_rows, 10), np.int64), np.zeros((n_rows, 4), np.int64)]
        return lib.nm_motif_coverage_count(*head(d), *sets(d), *motif(d), _ptr(rows, u64), _ptr(rows, u64), _ptr(out[0], u64), _ptr(out[1], i64),
                                           _ptr(out[2], i64)), out

    def coverage_sites(d):
        tail, out = window(len(d["bins"]))
        return lib.nm_motif_coverage_sites(*head(d), *sets(d), *motif(d), *tail), out

    def profile(d):
        n, nt = len(d["bins"]), len(d["targets"])
        out = [np.zeros((n, 2), np.uint64), np.zeros((n, nt, 2 * RADIUS + 1, 12), np.int64)]
        return lib.nm_motif_profile_count(*head(d), *motif(d), nt, _ptr(d["targets"], u8), RADIUS, _ptr(out[0], u64), _ptr(out[1], i64)), out

    def tracks(d):
        out = [np.zeros((n_wrows, 6), np.uint32)]
        return lib.nm_motif_tracks_count(*head(d), *slot(d), *motif(d), WINDOW, _ptr(wrows, u64), _ptr(out[0], u32)), out

    def fractions(d):
        out = [np.zeros((n_rows, 2, FBINS + 3), np.uint64)]
        return lib.nm_motif_fractions_count(*head(d), _ptr(d["rs"], u8), *motif(d), FBINS, _ptr(out[0], u64)), out

    def context(d):
        n = len(d["bins"])
        out = [np.zeros((n, 6), np.uint64), np.zeros((n, 2 * RADIUS + 1, 24), np.int64)]
        return lib.nm_motif_context_count(*head(d), *slot(d), *motif(d), RADIUS, _ptr(out[0], u64), _ptr(out[1], i64)), out

    return {"sites_count": lambda d: counted(lib.nm_motif_sites_count, d, slot(d), 7, 6),
            "sites": lambda d: recorded(lib.nm_motif_sites, d, slot(d), 7),
            "compare_count": lambda d: counted(lib.nm_motif_compare_count, d, two(d), 0x1FF, 18),
            "compare_sites": lambda d: recorded(lib.nm_motif_compare_sites, d, two(d), 0x1FF),
            "strands_count": lambda d: counted(lib.nm_motif_strands_count, d, partner(d), 0x1FF, 18),
            "strands_sites": lambda d: recorded(lib.nm_motif_strands_sites, d, partner(d), 0x1FF),
            "coverage_count": coverage_count, "coverage_sites": coverage_sites,
            "profile_count": profile, "tracks_count": tracks, "fractions_count": fractions, "context_count": context}


# The slot argument(s) a pileup is missing from, per unit: a mod slot (5: nothing uploaded), for fractions the read-statistics slot (0 = m:
# no statistics), for profile the per-call target list.
NO_PILEUP = {"compare": ("slots_b",), "fractions": ("rs",), "profile": ("targets",)}
# A candidate wrong in bin AND slot: the units whose answer is the same before and after the staging loop became one (bin first).  sites,
# compare, strands and coverage looked at the slot first and answered NM_ESTATE: their own suites assert the NM_EINVAL they give now.
# profile's slots belong to the call, not to a candidate: NM_ESTATE before and after.
BIN_FIRST = ("tracks_count", "fractions_count", "context_count")


def test_every_entry_point_refuses_alike_and_stays_usable(shared):
    eng = shared["eng"]
    b = eng.make_batch(engine_cands())
    n = len(b)
    far = eng.make_batch(engine_cands(CANDS[:3] + [("A" + "." * 96 + "T", 0, "a", "b1")] + CANDS[4:]))   # a reach of 97: compile_program's refusal
    per_bin = {i: len(eng.bin_contigs(i)) for i in (0, 1)}
    per_bin_w = {i: int(eng.track_windows(i, WINDOW)[-1]) for i in (0, 1)}
    rows, wrows = (np.concatenate([[0], np.cumsum([per[int(x)] for x in b.bins])]).astype(np.uint64) for per in (per_bin, per_bin_w))
    assert per_bin == {0: 2, 1: 1} and n == 6

    def arguments(batch=b, **over):
        d = dict(ctx=eng.ctx, bins=batch.bins, slots=batch.slots, slots_b=batch.slots, rs=np.full(n, 1, np.uint8), partner=np.zeros(n, np.int8),
                 targets=np.array([0, 1], np.uint8), lens=batch.lens, modpos=batch.modpos, offsets=batch.offsets, masks=batch.masks)
        d.update(over)
        return d

    at = lambda a, k, v: np.where(np.arange(len(a)) == k, v, a).astype(a.dtype)
    bad_bin = dict(bins=at(b.bins, 3, 2))                                # bin = n_bins
    launches = eng.stats()["launches"]
    for name, call in entry_points(eng, rows, wrows).items():
        unit = name.split("_")[0]
        rc, want = call(arguments())
        assert rc == NM_OK and any(w.any() for w in want), name
        launched = eng.stats()["launches"] - launches
        no_pileup = {}
        for key in NO_PILEUP.get(unit, ("slots",)):
            a = arguments()[key]
            no_pileup[key] = at(a, len(a) - 1, 0 if key == "rs" else 5)
        refusals = [("bin", NM_EINVAL, arguments(**bad_bin)), ("slot", NM_ESTATE, arguments(**no_pileup)), ("program", NM_ERANGE, arguments(far)),
                    ("ctx", NM_EINVAL, arguments(ctx=None))]
        if name in BIN_FIRST:
            both = dict(bad_bin, **{k: at(arguments()[k], 3, 0 if k == "rs" else 5) for k in no_pileup})
            refusals.append(("bin and slot", NM_EINVAL, arguments(**both)))
        if unit == "profile":                                            # the target slots are the call's: looked at before any candidate
            refusals.append(("bin and target slot", NM_ESTATE, arguments(**dict(bad_bin, **no_pileup))))
        for what, code, d in refusals:
            launches = eng.stats()["launches"]
            rc, out = call(d)
            assert rc == code, (name, what, rc, eng.lib.nm_last_error().decode())
            assert not any(o.any() for o in out) and eng.stats()["launches"] == launches, (name, what)   # refused on the host, nothing written
            rc, again = call(arguments())
            assert rc == NM_OK and all(np.array_equal(x, y) for x, y in zip(again, want)), (name, what)
            assert eng.stats()["launches"] - launches == launched, (name, what)
        launches = eng.stats()["launches"]
