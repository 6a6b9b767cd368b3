"""GPU: two-sample comparison (nm_motif_compare_count / nm_motif_compare_sites, ``ScanEngine.motif_compare_counts`` /
``motif_compare_sites``, ``nanomotif motif_compare``) against a brute-force oracle of Python sets built only from
``oracle.scan.subseq_indices``, ``oracle.scan.split_positions`` and ``oracle.motif.Motif``, applied to each sample and joined per
(position, strand).  Counts and records are integers: every comparison is an equality over ALL candidates, contigs and records of its
input.  The conditions on the input (``test_the_input_is_not_degenerate``) need no GPU."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import oracle_bin_inputs
from nanomotif_amd import synth
from nanomotif_amd.motif import Motif

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ("mod", "nomod", "nocall")
TRANSITIONS = tuple(f"{a}>{b}" for a in STATES for b in STATES)
SWITCHED = ("mod>nomod", "nomod>mod")
LABELS = lambda mt: (mt, mt + "@b")


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_cover(seq, motif_str, pos):
    """{(position, strand)} one candidate occurs at on one contig: the stripped motif on '+' (strand 0), its reverse complement on '-'
    (strand 1), every (overlapping) occurrence shifted to the modified base."""
    from oracle.motif import Motif as OMotif
    from oracle.scan import subseq_indices
    st = OMotif(motif_str, pos).new_stripped_motif()
    out = set()
    for strand, m in ((0, st), (1, st.reverse_compliment())):
        out |= {(int(p), strand) for p in subseq_indices(m.string, seq) + m.mod_position}
    return out


def oracle_calls(pile, low, high):
    """(M, U): the distinct (position, strand) calls of one contig; a position called both ways is methylated."""
    from oracle.scan import split_positions
    mf, nf, mr, nr = split_positions(pile, low, high)
    M = {(int(p), 0) for p in mf} | {(int(p), 1) for p in mr}
    U = ({(int(p), 0) for p in nf} | {(int(p), 1) for p in nr}) - M
    return M, U


def exact_p(g, l):
    """min(1, 2 P[X <= min(g, l)]), X ~ Binomial(g + l, 1/2), from integer binomials (C(n, i + 1) = C(n, i) (n - i) / (i + 1))."""
    n, term, total = g + l, 1, 0
    for i in range(min(g, l) + 1):
        total += term
        term = term * (n - i) // (i + 1)
    return min(1.0, 2 * total / 2 ** n)


def state_of(x, calls):
    return 0 if x in calls[0] else 1 if x in calls[1] else 2


class Expected:
    """What the contract says about ``cands`` = [(bin, mod type, motif string, mod position), ...] between two samples: per candidate
    the int64[n, 18] table, and all records (candidate, contig id, position, code) in contract order.  ``piles_a`` / ``piles_b``: mod
    type -> {contig name -> ContigPileup}; ``thresholds_b``: sample B's (low, high) when it differs from A's."""

    def __init__(self, cands, bin_contigs, contig_index, seqs, piles_a, piles_b, low=0.3, high=0.7, thresholds_b=None):
        from oracle.scan import _EMPTY
        low_b, high_b = thresholds_b or (low, high)
        calls = {}

        def calls_of(which, piles, mt, name, lo, hi):
            key = (which, mt, name)
            if key not in calls:
                calls[key] = oracle_calls(piles[mt].get(name, _EMPTY), lo, hi)
            return calls[key]
        self.tables, self.records = [], []
        for k, (b, mt, motif, pos) in enumerate(cands):
            names = bin_contigs[b]
            table = np.zeros((len(names), 18), dtype=np.int64)
            for r, name in enumerate(names):
                ca, cb = calls_of("a", piles_a, mt, name, low, high), calls_of("b", piles_b, mt, name, low_b, high_b)
                for x in sorted(oracle_cover(seqs[name], motif, pos)):          # ascending position, '+' before '-'
                    t = 3 * state_of(x, ca) + state_of(x, cb)
                    table[r, 9 * x[1] + t] += 1
                    self.records.append((k, contig_index[name], x[0], 16 * x[1] + t))
            self.tables.append(table)

    def selected(self, transitions):
        want = {TRANSITIONS.index(t) for t in transitions}
        return [r for r in self.records if (r[3] & 15) in want]


def engine_cands(cands):
    return [(Motif(m, p), mt, b) for b, mt, m, p in cands]


def records_of(eng, cands, transitions, max_records=None, labels=LABELS):
    """All records of ``eng.motif_compare_sites`` as a list of (candidate, contig, pos, code), and the number of deliveries."""
    parts = list(eng.motif_compare_sites(engine_cands(cands), labels, transitions=transitions, max_records=max_records))
    assert max_records is None or all(len(p.records) <= max_records for p in parts)
    rec = np.concatenate([p.records for p in parts]) if parts else np.zeros(0, dtype=[("candidate", "u4"), ("contig", "u4"), ("pos", "u4"), ("code", "u1")])
    return list(zip(rec["candidate"].tolist(), rec["contig"].tolist(), rec["pos"].tolist(), rec["code"].tolist())), len(parts)


def check(eng, cands, seqs, piles_a, piles_b, selections=(SWITCHED, TRANSITIONS), labels=LABELS, what="", **kw):
    """The 18-column tables and the records of every selection in ONE call each == the oracle; the marginals are ``motif_site_counts`` on
    either slot.  Returns (Expected, got tables)."""
    bin_contigs = {b: eng.bin_contigs(b) for b, _, _, _ in cands}
    exp = Expected(cands, bin_contigs, eng.contig_index, seqs, piles_a, piles_b, **kw)
    got = eng.motif_compare_counts(engine_cands(cands), labels)
    assert len(got) == len(cands)
    for k, (names, table) in enumerate(got):
        assert names == bin_contigs[cands[k][0]]
        assert table.shape == exp.tables[k].shape and np.array_equal(table, exp.tables[k]), (what, cands[k], table.tolist(), exp.tables[k].tolist())
    for side in (0, 1):                                                  # marginals: the six-column table of nm_motif_sites_count on that slot
        six = eng.motif_site_counts([(Motif(m, p), labels(mt)[side], b) for b, mt, m, p in cands])
        for k, ((_, table), (_, s)) in enumerate(zip(got, six)):
            t = table.reshape(-1, 2, 3, 3).sum(axis=3 - side)
            assert np.array_equal(t.reshape(-1, 6), s), (what, cands[k], "sample", "ab"[side])
    for sel in selections:
        rec, _ = records_of(eng, cands, sel, labels=labels)
        want = exp.selected(sel)
        assert len(rec) == len(want) and rec == want, (what, sel, len(rec), len(want))
    return exp, got


# ------------------------------------------------------------------------------------------------ two samples of one metagenome
class Sample(synth.SynthMetagenome):
    """The rows of a synthetic metagenome under a seeded perturbation (``role`` "a" or "b"); the sequences are the base's.
    Sample A lacks a seeded 6 % of the base's rows.  Sample B is made from sample A by
      (i)   flipping the fraction of 6 % of A's rows across both thresholds (pct -> 100 % - pct),
      (ii)  dropping 5 % of A's rows,
      (iii) adding half of the rows A lacks,
      (iv)  moving 4 % of A's rows between the thresholds (a called row to 50 %, an uncalled one to 90 %),
      (v)   switching ``off`` = (bin, motif string, mod position, mod type) off entirely: no row of B on an occurrence of that motif in that
            bin stays above the low threshold."""
    role = "a"
    off = None

    def contig_pileup(self, i, mod_type):
        base = synth.SynthMetagenome.contig_pileup(self, i, mod_type)
        n = len(base["position"])
        mt_id = ("a", "m", "21839").index(mod_type)
        lacks = np.random.default_rng((self.spec.seed, 101, i, mt_id)).random(n) < 0.06
        if self.role == "a":
            return {k: v[~lacks] for k, v in base.items()}
        rng = np.random.default_rng((self.spec.seed, 202, i, mt_id))
        u, added = rng.random(n), rng.random(n) < 0.5
        pct = base["pct_hundredths"].copy()
        flip = ~lacks & (u >= 0.05) & (u < 0.11)
        pct[flip] = 10000 - pct[flip]
        move = ~lacks & (u >= 0.11) & (u < 0.15)
        called = (pct <= 3000) | (pct >= 7000)
        pct[move & called] = 5000
        pct[move & ~called] = 9000
        keep = np.where(lacks, added, u >= 0.05)
        if self.off is not None and self.off[0] == self.bin_names[i] and self.off[3] == mod_type:
            sites = oracle_cover(self.contig_str(i), self.off[1], self.off[2])
            on_site = np.fromiter(((int(p), 0 if s == ord("+") else 1) in sites for p, s in zip(base["position"].tolist(), base["strand"].tolist())),
                                  dtype=bool, count=n)
            pct[on_site & (pct > 3000)] = 150
        out = dict(base, pct_hundredths=pct)
        return {k: v[keep] for k, v in out.items()}


def two_samples(spec, off=None):
    mg = synth.make_metagenome(spec)
    fields = {f.name: getattr(mg, f.name) for f in dataclasses.fields(mg)}
    a, b = Sample(**fields), Sample(**fields)
    b.role, b.off = "b", off
    return a, b


def _upload_samples(eng, a, b, mod_types, low=0.3, high=0.7, min_cov=5, thresholds_b=None, bin_names=None):
    idx = list(range(len(a.names)))
    eng.upload_assembly([a.names[i] for i in idx], [a.contig_ascii(i) for i in idx], [a.bin_names[i] for i in idx], bin_names=bin_names)
    low_b, high_b = thresholds_b or (low, high)
    for mg, suffix, lo, hi in ((a, "", low, high), (b, "@b", low_b, high_b)):
        for mt in mod_types:
            first = True
            for local, i in enumerate(idx):
                p = mg.contig_pileup(i, mt)
                keep = p["nvalid"] > min_cov
                eng.upload_pileup(mt, np.full(int(keep.sum()), local, np.uint32), p["position"][keep], p["strand"][keep],
                                  synth.pct_to_fraction(p["pct_hundredths"][keep]), low=lo, high=hi, append=not first, label=mt + suffix)
                first = False


def _oracle_inputs(a, b, mod_types):
    piles_a, piles_b, seqs = {}, {}, {}
    for mt in mod_types:
        piles_a[mt], seqs = oracle_bin_inputs(a, mt)
        piles_b[mt], _ = oracle_bin_inputs(b, mt)
    return seqs, piles_a, piles_b


def reach_class(s, p):
    sets, mp = Motif(s, p).stripped_sets()
    r = max(mp, len(sets) - 1 - mp)
    return 0 if r <= 31 else 1 if r <= 63 else 2


MOTIFS_A = [("GATC", 1), ("[AG]GATC[CT]", 2), ("GATC", 0), ("GCAC......GTT", 2), ("A" + "." * 40 + "C", 0), ("A" + "." * 70 + "T", 0), ("A", 0)]
MOTIFS_M = [("CC[AT]GG", 1), ("C..GG", 0), ("G" + "." * 50 + "C", 51), ("C" + "." * 94 + "G", 0)]
ZOO_SPEC = synth.SynthSpec(n_contigs=12, total_bp=300_000, n_bins=4, mod_types=("a", "m"), seed=77, min_contig_bp=3_000, n_fraction=0.002,
                           fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m"), ("GCACNNNNNNGTT", 2, "a")))
ZOO_OFF = ("bin_001", "GATC", 1, "a")


def _zoo():
    a, b = two_samples(ZOO_SPEC, off=ZOO_OFF)
    bins = sorted(set(a.bin_names))
    cands = [(bn, mt, m, p) for bn in bins for mt in ("a", "m") for m, p in (MOTIFS_A if mt == "a" else MOTIFS_M)]
    return a, b, cands


def _host_expected(a, b, cands, mod_types=("a", "m")):
    seqs, piles_a, piles_b = _oracle_inputs(a, b, mod_types)
    bin_contigs = {bn: [n for i, n in enumerate(a.names) if a.bin_names[i] == bn] for bn in set(a.bin_names)}
    return Expected(cands, bin_contigs, {n: i for i, n in enumerate(a.names)}, seqs, piles_a, piles_b), seqs, piles_a, piles_b


def test_the_input_is_not_degenerate():
    """(oracle side only, no GPU) Every one of the 18 columns is non-zero for at least one (candidate, contig); candidates run at G = 1, 2
    and 3; the switched-off motif has no methylated site left in B and the oracle's own test value for it is below 1e-6."""
    a, b, cands = _zoo()
    exp, _, _, _ = _host_expected(a, b, cands)
    table = np.concatenate(exp.tables)
    print("columns", table.sum(axis=0).tolist())
    assert (table.max(axis=0) > 0).all(), table.max(axis=0).tolist()
    assert {reach_class(m, p) for _, _, m, p in cands} == {0, 1, 2}
    k = cands.index((ZOO_OFF[0], ZOO_OFF[3], ZOO_OFF[1], ZOO_OFF[2]))
    t = exp.tables[k].sum(axis=0)
    nine = t[:9] + t[9:]
    assert nine[0] == 0 and nine[3] == 0 and nine[6] == 0 and nine[1] + nine[2] > 100
    assert exact_p(int(nine[3]), int(nine[1])) < 1e-6
    other = cands.index(("bin_000", "a", "GATC", 1))
    t = exp.tables[other].sum(axis=0)
    assert (t[:9] + t[9:])[0] > 100                                     # ... and stays methylated elsewhere
    for sel in TRANSITIONS:
        assert len(exp.selected((sel,))) > 0, sel


# ------------------------------------------------------------------------------------------------ 1. a literal case
@gpu
def test_literal_case_by_hand(engine_cls):
    """TACGGACGCCACG: ACG occurs at 1, 5, 10 on '+'; its reverse complement CGT nowhere.  A: 1 mod, 5 mod, 10 nomod; B: 1 nomod, 5 no row, 10 mod."""
    eng = engine_cls()
    eng.upload_assembly(["c"], ["TACGGACGCCACG"], ["b"])
    eng.upload_pileup("a", [0, 0, 0], [1, 5, 10], np.frombuffer(b"+++", np.uint8), [0.9, 0.95, 0.1])
    eng.upload_pileup("a", [0, 0], [1, 10], np.frombuffer(b"++", np.uint8), [0.2, 0.8], label="a@b")
    names, table = eng.motif_compare_counts([(Motif("ACG", 0), "a", "b")], LABELS)[0]
    assert names == ["c"] and table.tolist() == [[0, 1, 1, 1, 0, 0, 0, 0, 0] + [0] * 9]
    assert records_of(eng, [("b", "a", "ACG", 0)], SWITCHED)[0] == [(0, 0, 1, 1), (0, 0, 10, 3)]
    assert records_of(eng, [("b", "a", "ACG", 0)], TRANSITIONS)[0] == [(0, 0, 1, 1), (0, 0, 5, 2), (0, 0, 10, 3)]
    assert records_of(eng, [("b", "a", "ACG", 0)], ("mod>nocall",))[0] == [(0, 0, 5, 2)]
    # CGT@2 is ACG@0 seen from the other strand: the same positions on '-', where neither sample has a row
    names, table = eng.motif_compare_counts([(Motif("CGT", 2), "a", "b")], LABELS)[0]
    assert table.tolist() == [[0] * 9 + [0, 0, 0, 0, 0, 0, 0, 0, 3]]
    assert records_of(eng, [("b", "a", "CGT", 2)], TRANSITIONS)[0] == [(0, 0, 1, 24), (0, 0, 5, 24), (0, 0, 10, 24)]
    assert eng.motif_compare_counts([], LABELS) == [] and list(eng.motif_compare_sites([], LABELS)) == []
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. the synthetic metagenome, identities
@gpu
def test_synthetic_metagenome_two_samples(engine_cls):
    a, b, cands = _zoo()
    seqs, piles_a, piles_b = _oracle_inputs(a, b, ("a", "m"))
    eng = engine_cls()
    _upload_samples(eng, a, b, ("a", "m"))
    before = eng.stats()["launches"]
    got = eng.motif_compare_counts(engine_cands(cands), LABELS)
    assert eng.stats()["launches"] - before == 3                        # one count launch per reach width, whatever the batch
    exp, got = check(eng, cands, seqs, piles_a, piles_b, selections=[(t,) for t in TRANSITIONS] + [SWITCHED, TRANSITIONS])
    table = np.concatenate([t for _, t in got])
    print("columns", table.sum(axis=0).tolist())
    assert (table.max(axis=0) > 0).all()
    # the eighteen sum to the occurrences
    for (bn, mt, m, p), (names, t) in zip(cands, got):
        assert t.sum(axis=1).tolist() == [len(oracle_cover(seqs[n], m, p)) for n in names]
    # compare(A, A) is diagonal, and its diagonal is motif_site_counts
    same = eng.motif_compare_counts(engine_cands(cands), lambda mt: (mt, mt))
    six = eng.motif_site_counts(engine_cands(cands))
    for (_, t), (_, s) in zip(same, six):
        assert np.array_equal(t[:, [0, 4, 8, 9, 13, 17]], s) and t.sum() == s.sum()
    # swapping the slots transposes the 3 x 3 blocks
    swapped = eng.motif_compare_counts(engine_cands(cands), lambda mt: (mt + "@b", mt))
    for (_, t), (_, s) in zip(got, swapped):
        assert np.array_equal(t.reshape(-1, 2, 3, 3).transpose(0, 1, 3, 2).reshape(-1, 18), s)
    rec_ab, _ = records_of(eng, cands[:3], ("mod>nomod",))
    rec_ba, _ = records_of(eng, cands[:3], ("nomod>mod",), labels=lambda mt: (mt + "@b", mt))
    assert len(rec_ab) > 0 and [(k, c, p, (code & 16) | 3) for k, c, p, code in rec_ab] == rec_ba
    # a candidate listed twice gets equal rows and equal records
    twice = eng.motif_compare_counts(engine_cands([cands[0], cands[5], cands[0]]), LABELS)
    assert np.array_equal(twice[0][1], twice[2][1]) and np.array_equal(twice[0][1], got[0][1])
    rec, _ = records_of(eng, [cands[0], cands[5], cands[0]], SWITCHED)
    assert [r[1:] for r in rec if r[0] == 0] == [r[1:] for r in rec if r[0] == 2] and any(r[0] == 2 for r in rec)
    eng.close()


@gpu
def test_two_threshold_pairs_of_one_pileup(engine_cls):
    """Any two present slots: sample A's rows classified at 0.3 / 0.7 against the same rows at 0.1 / 0.9 — nothing switches, calls are lost."""
    a, _, cands = _zoo()
    cands = cands[:11]
    seqs, piles_a, _ = _oracle_inputs(a, a, ("a", "m"))
    eng = engine_cls()
    _upload_samples(eng, a, a, ("a", "m"), thresholds_b=(0.1, 0.9))
    exp, got = check(eng, cands, seqs, piles_a, piles_a, thresholds_b=(0.1, 0.9))
    t = np.concatenate([t for _, t in got]).sum(axis=0)
    t = t[:9] + t[9:]
    assert t[1] == t[3] == t[6] == t[7] == 0 and t[2] > 0 and t[5] > 0 and t[0] > 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. windows
@gpu
def test_windows_do_not_change_the_result(engine_cls):
    spec = synth.SynthSpec(n_contigs=6, total_bp=120_000, n_bins=2, mod_types=("a",), seed=5, min_contig_bp=3_000, fixed_motifs=(("GATC", 1, "a"),))
    a, b = two_samples(spec)
    bins = sorted(set(a.bin_names))
    cands = [(bins[0], "a", "GATC", 1), (bins[1], "a", "CCCCCCCCCCCC", 3), (bins[0], "a", "A" + "." * 70 + "T", 0), (bins[1], "a", "GATC", 1),
             (bins[1], "a", "[AG]GATC[CT]", 2), (bins[0], "a", "AC", 0)]
    seqs, piles_a, piles_b = _oracle_inputs(a, b, ("a",))
    eng = engine_cls()
    _upload_samples(eng, a, b, ("a",))
    exp, _ = check(eng, cands, seqs, piles_a, piles_b)
    want = exp.selected(SWITCHED)
    total = len(want)
    assert total > 300
    whole, n = records_of(eng, cands, SWITCHED)
    assert n == 1 and whole == want
    prime = next(q for q in range(total // 10, total) if all(q % d for d in range(2, int(q ** 0.5) + 1)))
    for budget in (prime, 7, 1):
        rec, n_b = records_of(eng, cands, SWITCHED, max_records=budget)
        assert rec == want, budget
        assert n_b >= total // budget
    everything = exp.selected(TRANSITIONS)
    prime = next(q for q in range(len(everything) // 10, len(everything)) if all(q % d for d in range(2, int(q ** 0.5) + 1)))
    rec, n_b = records_of(eng, cands, TRANSITIONS, max_records=prime)
    assert rec == everything and n_b >= 10
    with pytest.raises(ValueError):
        list(eng.motif_compare_sites(engine_cands(cands), LABELS, max_records=0))
    # the ABI's windows: odd sizes tile the call, nothing beyond what was reported is touched
    from nanomotif_amd import _lib
    from nanomotif_amd.engine import _ptr
    bt, slots_b = eng._compare_batch(engine_cands(cands), LABELS)
    args = eng._compare_args(bt, slots_b)
    per_cand = [sum(1 for r in want if r[0] == k) for k in range(len(cands))]
    at, parts = 0, []
    while at < total:
        cap = 333
        contig, pos, code = (np.full(cap + 8, 0xEE, dtype=t) for t in (np.uint32, np.uint32, np.uint8))
        off = np.zeros(len(cands) + 1, dtype=np.uint64)
        nw = C.c_uint64(99)
        _lib.check(eng.lib.nm_motif_compare_sites(eng.ctx, *args, 10, at, cap, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8),
                                                  _ptr(off, C.c_uint64), C.byref(nw)))
        assert nw.value == min(cap, total - at) and (code[nw.value:] == 0xEE).all() and (pos[nw.value:] == 0xEE).all()
        assert off.tolist() == [sum(per_cand[:k]) for k in range(len(cands) + 1)]
        parts += list(zip(contig[:nw.value].tolist(), pos[:nw.value].tolist(), code[:nw.value].tolist()))
        at += int(nw.value)
    assert parts == [r[1:] for r in want]
    nw = C.c_uint64(99)
    _lib.check(eng.lib.nm_motif_compare_sites(eng.ctx, *args, 10, total + 5, 10, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8),
                                              _ptr(off, C.c_uint64), C.byref(nw)))
    assert nw.value == 0 and int(off[-1]) == total
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. geometry
@gpu
def test_layouts_that_break_naive_chunking(engine_cls):
    """A contig of eight chunks with occurrences across the 8 192-position chunk border, an N run across a border, contigs shorter than the
    motif, a bin without contigs; the one-letter candidate A @ 0 against a direct count of the calls on A / T positions."""
    from oracle.scan import ContigPileup
    rng = np.random.default_rng(12)
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    big = list(rand(60_000))
    big[8185:8200] = "N" * 15                                           # an N run across a chunk border
    big[8170:8185] = "GATCGATCGATCGAT"                                  # ... with occurrences right before it
    big[8200:8204] = "GATC"
    big[16380:16390] = "AAAAAAAAAA"                                     # overlapping occurrences across a chunk border
    big[24574:24578] = "GATC"                                           # a palindrome astride a chunk border
    seqs = {"big": "".join(big), "tiny1": "G", "tiny2": "GA", "tiny3": "ATC", "ends_GA": rand(9000) + "GA", "starts_TC": "TC" + rand(500),
            "pal": "GATC" * 50 + "AATT" * 30, "n_only": "N" * 40, "edge": "GATC" + rand(8192 - 8) + "GATC", "other": "GATC" + rand(3000) + "GA",
            "alone": rand(20_000)}
    bins = {n: ("b3" if n == "alone" else "b2" if n == "other" else "b1") for n in seqs}
    names = list(seqs)
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names], bin_names=["b0_empty", "b1", "b2", "b3"])
    assert eng.bin_contigs("b0_empty") == []
    piles = {"a": {}, "a@b": {}}
    for label in piles:
        cid, pos, st, fr = [], [], [], []
        for i, n in enumerate(names):
            L = len(seqs[n])
            p = np.sort(rng.choice(L, size=max(1, (2 * L) // 3), replace=False)).astype(np.int64)
            strand = rng.choice(np.array([ord("+"), ord("-")], dtype=np.uint8), size=len(p))
            f = rng.choice([0.0, 0.3, 0.30000000000000004, 0.5, 0.7, 0.6999999999999999, 1.0], size=len(p))
            piles[label][n] = ContigPileup(p, strand, f)
            cid += [i] * len(p); pos += p.tolist(); st += strand.tolist(); fr += f.tolist()
        eng.upload_pileup("a", cid, pos, np.array(st, np.uint8), fr, label=label)
    motifs = [("GATC", 1), ("GATC", 0), ("AA", 0), ("AA", 1), ("A", 0), ("AATT", 1), ("GA.C", 1), ("G[AG]TC", 1), ("A.........A", 0), ("ATC", 2), ("GAT[CG]", 3),
              ("G" + "." * 40 + "C", 0), ("A" + "." * 80 + "T", 81), ("T" + "." * 94 + "A", 0)]
    cands = [(b, "a", m, p) for b in ("b1", "b2", "b3") for m, p in motifs]
    exp, got = check(eng, cands, seqs, {"a": piles["a"]}, {"a": piles["a@b"]})
    table = np.concatenate(exp.tables)
    assert (table.sum(axis=0) > 50).all() and len(exp.records) > 100_000
    # occurrences astride the borders are there: GATC @ 1 at 24575 '+' and 24576 '-', AA @ 0 on every position of the run of A
    k = cands.index(("b1", "a", "GATC", 1))
    on_big = {(r[2], r[3] >> 4) for r in exp.records if r[0] == k and r[1] == names.index("big")}
    assert {(24575, 0), (24576, 1), (8171, 0), (8201, 0)} <= on_big and not any(8185 <= p < 8200 for p, _ in on_big)
    k = cands.index(("b1", "a", "AA", 0))
    assert {(p, 0) for p in range(16380, 16389)} <= {(r[2], r[3] >> 4) for r in exp.records if r[0] == k and r[1] == names.index("big")}
    # contigs shorter than the motif and the contig of N hold no occurrence of GATC
    k = cands.index(("b1", "a", "GATC", 1))
    rows = eng.bin_contigs("b1")
    for n in ("tiny1", "tiny2", "tiny3", "n_only"):
        assert got[k][1][rows.index(n)].sum() == 0
    # A @ 0: every A on '+' and every T on '-', by a direct count of the calls
    for b in ("b1", "b2", "b3"):
        k = cands.index((b, "a", "A", 0))
        for r, n in enumerate(eng.bin_contigs(b)):
            ca, cb = oracle_calls(piles["a"][n], 0.3, 0.7), oracle_calls(piles["a@b"][n], 0.3, 0.7)
            direct = np.zeros(18, dtype=np.int64)
            for p, letter in enumerate(seqs[n]):
                if letter in "AT":
                    x = (p, 0 if letter == "A" else 1)
                    direct[9 * x[1] + 3 * state_of(x, ca) + state_of(x, cb)] += 1
            assert got[k][1][r].tolist() == direct.tolist(), (b, n)
    # a bin without contigs: no rows, no records, also next to other candidates; and an empty batch
    res = eng.motif_compare_counts(engine_cands([("b0_empty", "a", "GATC", 1), ("b2", "a", "GATC", 1), ("b0_empty", "a", "A", 0)]), LABELS)
    assert res[0][0] == [] and res[0][1].shape == (0, 18) and res[2][1].shape == (0, 18)
    assert np.array_equal(res[1][1], got[cands.index(("b2", "a", "GATC", 1))][1])
    rec, _ = records_of(eng, [("b0_empty", "a", "GATC", 1), ("b2", "a", "GATC", 1), ("b0_empty", "a", "A", 0)], TRANSITIONS)
    assert {r[0] for r in rec} == {1} and len(rec) == int(res[1][1].sum())
    assert records_of(eng, [("b0_empty", "a", "GATC", 1)], TRANSITIONS)[0] == []
    rows0, tot, tab, nw = np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(18, np.int64), C.c_uint64(5)
    from nanomotif_amd.engine import _ptr
    assert eng.lib.nm_motif_compare_count(eng.ctx, 0, None, None, None, None, None, None, None, 0x1FF, _ptr(rows0, C.c_uint64), None, None) == 0
    assert eng.lib.nm_motif_compare_sites(eng.ctx, 0, None, None, None, None, None, None, None, 0x1FF, 0, 0, None, None, None, _ptr(tot, C.c_uint64),
                                          C.byref(nw)) == 0 and nw.value == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. errors, launches
@gpu
def test_errors_are_loud_and_leave_the_engine_usable(engine_cls):
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.engine import _ptr
    eng = engine_cls()
    bt, slots_b = eng._compare_batch([(Motif("GATC", 1), "a", 0)], (0, 0))
    rows, tot, tab = np.array([0, 1], np.uint64), np.zeros(1, np.uint64), np.zeros((1, 18), np.int64)
    assert eng.lib.nm_motif_compare_count(eng.ctx, *eng._compare_args(bt, slots_b), 0x1FF, _ptr(rows, C.c_uint64), _ptr(tot, C.c_uint64),
                                          _ptr(tab, C.c_int64)) == -3                                # NM_ESTATE: no assembly
    eng.upload_assembly(["c"], ["GATCGATC"], ["b"])
    eng.upload_pileup("a", [0], [1], np.frombuffer(b"+", np.uint8), [1.0])
    eng.upload_pileup("a", [0], [1], np.frombuffer(b"+", np.uint8), [0.0], label="a@b")
    far = Motif("A" + "." * 100 + "T", 0)
    with pytest.raises(NmScanError) as e:
        eng.motif_site_counts([(far, "a", "b")])
    sites_code = e.value.code
    assert sites_code == -5                                             # NM_ERANGE
    for call in (lambda c, l: eng.motif_compare_counts(c, l), lambda c, l: list(eng.motif_compare_sites(c, l))):
        for pair in (("a", 5), (5, "a"), ("a", 8), (200, "a@b")):       # a slot without a pileup, on either side; a slot beyond the eight
            with pytest.raises(NmScanError) as e:
                call([(Motif("GATC", 1), "a", "b")], pair)
            assert e.value.code == -3, pair                             # NM_ESTATE
        with pytest.raises(NmScanError) as e:                           # no such bin
            call([(Motif("GATC", 1), "a", 7)], LABELS)
        assert e.value.code == -1
        with pytest.raises(NmScanError) as e:                           # no such bin and no pileup in a slot: the bin is refused first
            call([(Motif("GATC", 1), "a", 7)], ("a", 5))
        assert e.value.code == -1
        with pytest.raises(NmScanError) as e:                           # beyond the reach limit: nm_motif_sites' code
            call([(Motif("GATC", 1), "a", "b"), (far, "a", "b")], LABELS)
        assert e.value.code == sites_code
    bt, slots_b = eng._compare_batch([(Motif("GATC", 1), "a", "b")], LABELS)
    args = eng._compare_args(bt, slots_b)
    rows, tot, tab = np.array([0, 1], np.uint64), np.zeros(1, np.uint64), np.zeros((1, 18), np.int64)
    contig, pos, code, off, nw = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(8, np.uint8), np.zeros(2, np.uint64), C.c_uint64(0)
    for bad in (0, 512, 513, 0x1FF | 1 << 16, 1 << 31):
        assert eng.lib.nm_motif_compare_count(eng.ctx, *args, bad, _ptr(rows, C.c_uint64), _ptr(tot, C.c_uint64), _ptr(tab, C.c_int64)) == -1, bad
        assert eng.lib.nm_motif_compare_sites(eng.ctx, *args, bad, 0, 8, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32), _ptr(code, C.c_uint8),
                                              _ptr(off, C.c_uint64), C.byref(nw)) == -1, bad
    assert eng.lib.nm_motif_compare_count(eng.ctx, *args, 0x1FF, None, _ptr(tot, C.c_uint64), _ptr(tab, C.c_int64)) == -1
    assert eng.lib.nm_motif_compare_count(eng.ctx, *args, 0x1FF, _ptr(np.array([0, 0], np.uint64), C.c_uint64), _ptr(tot, C.c_uint64), _ptr(tab, C.c_int64)) == -1
    assert eng.lib.nm_motif_compare_count(eng.ctx, 1, None, None, None, None, None, None, None, 0x1FF, _ptr(rows, C.c_uint64), _ptr(tot, C.c_uint64), _ptr(tab, C.c_int64)) == -1
    assert eng.lib.nm_motif_compare_sites(eng.ctx, *args, 0x1FF, 0, 8, None, None, None, _ptr(off, C.c_uint64), C.byref(nw)) == -1
    # the engine is usable afterwards: GATC@1 on GATCGATC occurs at '+' 1, 5 and '-' 2, 6; (1, '+') is mod in A and nomod in B
    assert eng.lib.nm_motif_compare_count(eng.ctx, *args, 2, _ptr(rows, C.c_uint64), _ptr(tot, C.c_uint64), _ptr(tab, C.c_int64)) == 0
    assert tab.tolist() == [[0, 1, 0, 0, 0, 0, 0, 0, 1] + [0] * 8 + [2]] and tot.tolist() == [1]
    assert records_of(eng, [("b", "a", "GATC", 1)], TRANSITIONS)[0] == [(0, 0, 1, 1), (0, 0, 2, 24), (0, 0, 5, 8), (0, 0, 6, 24)]
    eng.close()


@gpu
def test_launches_do_not_grow_with_the_batch(engine_cls):
    a, b, cands = _zoo()
    eng = engine_cls()
    _upload_samples(eng, a, b, ("a", "m"))
    assert {reach_class(m, p) for _, _, m, p in cands} == {0, 1, 2}
    counted = {}
    for reps in (1, 4):
        batch = engine_cands(cands * reps)
        before = eng.stats()["launches"]
        eng.motif_compare_counts(batch, LABELS)
        mid = eng.stats()["launches"]
        parts = list(eng.motif_compare_sites(batch, LABELS, transitions=TRANSITIONS))
        counted[reps] = (mid - before, eng.stats()["launches"] - mid, len(parts))
    # count: one launch per width; the export counts once for its budget, then per delivery count (3) + scan + gather + fill (3)
    assert counted[1] == (3, 3 + (3 + 2 + 3), 1) and counted[4] == counted[1]
    narrow = engine_cands([c for c in cands if reach_class(c[2], c[3]) == 0])
    before = eng.stats()["launches"]
    eng.motif_compare_counts(narrow, LABELS)
    assert eng.stats()["launches"] - before == 1
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. the command
def _run(tmp, command, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "nanomotif_amd", command] + args, cwd=tmp, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _filtered_piles(mg):
    """mod type -> {contig -> ContigPileup} after the three pre-filters of motif_discovery (find_motifs_bin.py:399-414), per bin as
    oracle.pipeline.bin_rows builds them."""
    from oracle import pileup as op
    from oracle import pipeline as opl
    from oracle.scan import ContigPileup
    piles = {mt: {} for mt in opl.MODS}
    for b in sorted(set(mg.bin_names)):
        t, idx = opl.bin_table(mg, b)
        t = op.prefilter(t)
        for mt_id, mt in enumerate(opl.MODS):
            for i in idx:
                s = (t["mod_type"] == mt_id) & (t["contig"] == i)
                if s.any():
                    o = np.argsort(t["position"][s], kind="stable")
                    piles[mt][mg.names[i]] = ContigPileup(t["position"][s][o], t["strand"][s][o], t["fraction_mod"][s][o])
    return piles


def _rows(text):
    lines = text.strip().split("\n")
    head = lines[0].split("\t")
    return head, [dict(zip(head, line.split("\t"))) for line in lines[1:]]


def _derived(n):
    """The derived columns of one 3 x 3 table, the test's own way: integer binomials."""
    n = [int(x) for x in n]
    both = n[0] + n[1] + n[3] + n[4]
    deg = ["%.6f" % ((n[0] + n[1]) / both), "%.6f" % ((n[0] + n[3]) / both), "%.6f" % ((n[3] - n[1]) / both)] if both else ["nan"] * 3
    g, l = n[3], n[1]
    p = "nan" if g + l == 0 else "%.6g" % exact_p(g, l)
    return [str(n[0] + n[1] + n[2]), str(n[3] + n[4] + n[5]), str(n[0] + n[3] + n[6]), str(n[1] + n[4] + n[7])] + deg + [p]


def _expected_files(a, b, bin_motifs_texts, transitions=SWITCHED):
    """The four files the oracle gives for the candidates of several bin-motifs.tsv (complements included, duplicates dropped)."""
    from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL, iupac_to_regex
    from nanomotif_amd.pileup import MOD_TYPES
    piles_a, piles_b = _filtered_piles(a), _filtered_piles(b)
    seqs = {n: a.contig_str(i) for i, n in enumerate(a.names)}
    cands, seen = [], set()
    for text in bin_motifs_texts:
        for row in _rows(text)[1]:
            both = [(row["reference"], row["motif"], row["mod_type"], int(row["mod_position"]))]
            if row["motif_complement"]:
                both.append((row["reference"], row["motif_complement"], row["mod_type"], int(row["mod_position_complement"])))
            for c in both:
                if c not in seen:
                    seen.add(c)
                    cands.append(c)
    bins = sorted(set(a.bin_names))
    bin_contigs = {bn: [n for i, n in enumerate(a.names) if a.bin_names[i] == bn] for bn in bins}      # contig_bin.tsv order
    index = {n: i for i, n in enumerate(a.names)}
    mod_types = [mt for mt in MOD_TYPES if piles_a[mt] or piles_b[mt]]                                  # slot order
    exp = Expected([(bn, mt, iupac_to_regex(m), p) for bn, m, mt, p in cands], bin_contigs, index, seqs, piles_a, piles_b)
    f_main, f_contigs = [], []
    for k, (bn, m, mt, p) in enumerate(cands):
        t = exp.tables[k].sum(axis=0)
        nine = (t[:9] + t[9:]).tolist()
        f_main.append([bn, m, mt, str(p)] + [str(x) for x in nine] + _derived(nine))
        f_contigs += [[bn, name, m, mt, str(p)] + [str(int(x)) for x in exp.tables[k][r]] for r, name in enumerate(bin_contigs[bn])]
    keys = [(bn, mt) for bn in bins for mt in mod_types]
    bg = Expected([(bn, mt, MOD_TYPE_TO_CANONICAL[mt], 0) for bn, mt in keys], bin_contigs, index, seqs, piles_a, piles_b)
    f_bins = []
    for (bn, mt), t in zip(keys, bg.tables):
        t = t.sum(axis=0)
        nine = (t[:9] + t[9:]).tolist()
        f_bins.append([bn, mt] + [str(x) for x in nine] + _derived(nine))
    bed = "".join(f"{a.names[c]}\t{p}\t{p + 1}\t{cands[k][1]}_{cands[k][2]}_{cands[k][3]}\t0\t{'-' if code & 16 else '+'}\t{TRANSITIONS[code & 15]}\t{cands[k][0]}\n"
                  for k, c, p, code in exp.selected(transitions))
    return f_main, f_contigs, f_bins, bed, cands


def _body(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [line.split("\t") for line in lines[1:-1]]


@gpu
def test_command_on_two_pileups(tmp_path):
    """motif_discovery on each sample, then motif_compare --switched_sites on both pileups and both bin-motifs.tsv, each in a child process,
    plain and bgzip + tabix: the four files equal the oracle-derived text; the marginals are the counts of each sample's bin-motifs.tsv; the
    motif switched off in one bin reads as switched off (its 1 020 methylated sites of sample A are nomod or without a call in B:
    mcnemar_p = 2^-1019).  The other motifs move too, by design of the input: the planted sites are 97 % methylated, so flipping the same
    share of every row takes far more sites from mod to nomod than back (GATC in the other bin: 77 against 2)."""
    from helpers import write_bgzf_tabix
    spec = synth.SynthSpec(n_contigs=4, total_bp=400_000, n_bins=2, mod_types=("a", "m"), seed=61, min_contig_bp=60_000,
                           fixed_motifs=(("GATC", 1, "a"), ("ACCCA", 4, "a"), ("CCWGG", 1, "m")))
    off = ("bin_001", "GATC", 1, "a")
    a, b = two_samples(spec, off=off)
    tmp = str(tmp_path)
    a.write_fasta(tmp + "/assembly.fasta")
    a.write_contig_bin(tmp + "/contig_bin.tsv")
    for mg, name in ((a, "a"), (b, "b")):
        mg.write_bed(f"{tmp}/pileup_{name}.bed")
        write_bgzf_tabix(open(f"{tmp}/pileup_{name}.bed", "rb").read(), f"{tmp}/pileup_{name}.bed.gz", block_size=50_000)
        _run(tmp, "motif_discovery", ["assembly.fasta", f"pileup_{name}.bed", "-c", "contig_bin.tsv", "--out", "out_" + name])
    bm_a, bm_b = open(tmp + "/out_a/bin-motifs.tsv").read(), open(tmp + "/out_b/bin-motifs.tsv").read()
    assert ("bin_001", "GATC") in {(r["reference"], r["motif"]) for r in _rows(bm_a)[1]}
    f_main, f_contigs, f_bins, bed, cands = _expected_files(a, b, [bm_a, bm_b])
    assert len(bed) > 0 and len(f_main) >= len(_rows(bm_a)[1])
    for pa, pb, out in (("pileup_a.bed", "pileup_b.bed", "cmp"), ("pileup_a.bed.gz", "pileup_b.bed.gz", "cmp_gz")):
        _run(tmp, "motif_compare", ["assembly.fasta", pa, pb, "-c", "contig_bin.tsv", "--bin_motifs", "out_a/bin-motifs.tsv", "out_b/bin-motifs.tsv",
                                    "--out", out, "--switched_sites"])
        head, body = _body(f"{tmp}/{out}/motif-compare.tsv")
        assert head[:4] == ["bin", "motif", "mod_type", "mod_position"] and head[4:13] == ["n_" + t.replace(">", "_") for t in TRANSITIONS]
        assert head[13:] == ["n_mod_a", "n_nomod_a", "n_mod_b", "n_nomod_b", "degree_a", "degree_b", "degree_delta", "mcnemar_p"]
        for row in body:
            print(out, "\t".join(row))
        assert body == f_main
        main = body
        head, body = _body(f"{tmp}/{out}/motif-compare-contigs.tsv")
        assert len(head) == 23 and body == f_contigs
        head, body = _body(f"{tmp}/{out}/motif-compare-bins.tsv")
        assert head[:2] == ["bin", "mod_type"] and len(head) == 19 and body == f_bins and len(body) == 4
        got_bed = open(f"{tmp}/{out}/switched-sites.bed").read()
        assert len(got_bed) == len(bed) and got_bed == bed
        assert os.path.exists(f"{tmp}/{out}/args.motif_compare.json") and os.path.exists(f"{tmp}/{out}/logs/timings.motif_compare.json")
        # every row of either bin-motifs.tsv finds its n_mod / n_nomod in that sample's marginals
        table = {(r[0], r[1], r[2], int(r[3])): r for r in main}
        assert len(table) == len(main)
        for text, at in ((bm_a, 13), (bm_b, 15)):
            for r in _rows(text)[1]:
                row = table[(r["reference"], r["motif"], r["mod_type"], int(r["mod_position"]))]
                assert (int(row[at]), int(row[at + 1])) == (int(r["n_mod"]), int(r["n_nomod"])), (r, row)
                if r["motif_complement"]:
                    row = table[(r["reference"], r["motif_complement"], r["mod_type"], int(r["mod_position_complement"]))]
                    assert (int(row[at]), int(row[at + 1])) == (int(r["n_mod_complement"]), int(r["n_nomod_complement"])), (r, row)
        # the switched-off motif
        row = table[(off[0], "GATC", "a", 1)]
        n = [int(x) for x in row[4:13]]
        assert n[0] == 0 and n[3] == 0 and n[1] + n[2] == int(row[13]) > 0 and float(row[20]) < 1e-6
    # other transitions: the same tables, other records; without --switched_sites no BED
    _run(tmp, "motif_compare", ["assembly.fasta", "pileup_a.bed", "pileup_b.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out_a/bin-motifs.tsv",
                                "out_b/bin-motifs.tsv", "--out", "cmp_lost", "--switched_sites", "--transitions", "mod>nocall,nocall>mod,mod>nomod"])
    lost = ("mod>nomod", "mod>nocall", "nocall>mod")
    assert open(tmp + "/cmp_lost/switched-sites.bed").read() == _expected_files(a, b, [bm_a, bm_b], transitions=lost)[3]
    _run(tmp, "motif_compare", ["assembly.fasta", "pileup_a.bed", "pileup_b.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out_a/bin-motifs.tsv",
                                "out_b/bin-motifs.tsv", "--out", "cmp_plain"])
    assert not os.path.exists(tmp + "/cmp_plain/switched-sites.bed")
    for name in ("motif-compare.tsv", "motif-compare-contigs.tsv", "motif-compare-bins.tsv"):
        assert open(f"{tmp}/cmp_plain/{name}").read() == open(f"{tmp}/cmp/{name}").read() == open(f"{tmp}/cmp_lost/{name}").read()
