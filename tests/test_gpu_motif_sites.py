"""GPU: the batched per-site export (nm_motif_sites / nm_motif_sites_count, ``ScanEngine.motif_sites``, ``nanomotif motif_sites``)
against the reference's recorded vectors (fixture g2), ``hit_positions`` and the CPU oracle built per contig from
``oracle.scan.motif_model_contig(..., save_motif_positions=True)`` + ``subseq_indices``.  Records, their order and the count
tables must be bit-exact; every comparison runs over ALL candidates and ALL contigs of its input."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import load_golden, motif_zoo, oracle_bin_inputs, sha1, spec_from_json
from nanomotif_amd import synth
from nanomotif_amd.motif import Motif

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ("mod", "nomod", "nocall")
KEYS = ("index_meth_fwd", "index_nonmeth_fwd", "index_meth_rev", "index_nonmeth_rev")


@pytest.fixture(scope="module")
def engine_cls():
    from nanomotif_amd.engine import ScanEngine
    return ScanEngine


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_contig_sites(seq, pile, motif_str, pos, low=0.3, high=0.7):
    """(positions, codes) of one motif on one contig in contract order.  The called states are the four arrays of
    motif_model_contig(save_motif_positions=True); the occurrences are subseq_indices of the stripped motif ('+') and of its reverse
    complement ('-') shifted to the modified base; an occurrence in neither array of its strand carries no call."""
    from oracle.model import BetaBernoulliModel
    from oracle.motif import Motif as OMotif
    from oracle.scan import motif_model_contig, subseq_indices
    m = OMotif(motif_str, pos)
    _, arrays = motif_model_contig(pile, seq, BetaBernoulliModel(), m, low, high, save_motif_positions=True)
    st = m.new_stripped_motif()
    rc = st.reverse_compliment()
    ps, cs = [], []
    for strand, (mm, meth, non) in enumerate(((st, arrays[KEYS[0]], arrays[KEYS[1]]), (rc, arrays[KEYS[2]], arrays[KEYS[3]]))):
        idx = subseq_indices(mm.string, seq) + mm.mod_position
        state = np.full(len(idx), 2, dtype=np.int64)
        is_m, is_n = np.isin(idx, meth), np.isin(idx, non)
        assert is_m.sum() == len(meth) and is_n.sum() == len(non) and not (is_m & is_n).any()     # the called sites ARE occurrences
        state[is_m] = 0
        state[is_n] = 1
        ps.append(idx)
        cs.append(state + 4 * strand)
    p, c = np.concatenate(ps), np.concatenate(cs)
    order = np.lexsort((c >> 2, p))                                     # ascending position, '+' before '-'
    return p[order].astype(np.int64), c[order].astype(np.uint8)


def expected_records(eng, cands, seqs, piles, low=0.3, high=0.7, states=STATES):
    """Structured records (engine.SITE_DTYPE) of ``cands`` = [(motif string, pos, mod type, bin)] in contract order, and the six-count
    table per candidate.  ``seqs``: contig name -> sequence; ``piles``: mod type -> {contig name -> ContigPileup}."""
    from nanomotif_amd.engine import SITE_DTYPE
    from oracle.scan import _EMPTY
    want = [STATES.index(s) for s in states]
    parts, tables = [], []
    for k, (s, p, mt, b) in enumerate(cands):
        names = eng.bin_contigs(b)
        table = np.zeros((len(names), 6), dtype=np.int64)
        for r, name in enumerate(names):
            pos, code = oracle_contig_sites(seqs[name], piles[mt].get(name, _EMPTY), s, p, low, high)
            for j in range(6):
                table[r, j] = int(((code >> 2 == j // 3) & (code & 3 == j % 3)).sum())
            keep = np.isin(code & 3, want)
            rec = np.zeros(int(keep.sum()), dtype=SITE_DTYPE)
            rec["candidate"], rec["contig"], rec["pos"], rec["code"] = k, eng.contig_index[name], pos[keep], code[keep]
            parts.append(rec)
        tables.append(table)
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=SITE_DTYPE)), tables


def collect(eng, cands, states=STATES, max_records=None):
    """All records of ``eng.motif_sites`` concatenated, the count tables per candidate, and the number of deliveries."""
    from nanomotif_amd.engine import SITE_DTYPE
    ecands = [(Motif(s, p), mt, b) for s, p, mt, b in cands]
    parts, tables, n = [], [], 0
    for sb in eng.motif_sites(ecands, states=states, max_records=max_records):
        n += 1
        assert max_records is None or len(sb.records) <= max_records
        parts.append(sb.records)
        if sb.counts is not None:
            tables += [t for _, t in sb.counts]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=SITE_DTYPE)), tables, n


def assert_same_records(got, exp, what=""):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for f in ("candidate", "contig", "pos", "code"):
        bad = np.flatnonzero(got[f] != exp[f])
        assert len(bad) == 0, (what, f, int(bad[0]), got[max(0, int(bad[0]) - 2):int(bad[0]) + 3].tolist(), exp[max(0, int(bad[0]) - 2):int(bad[0]) + 3].tolist())
    assert got.tobytes() == exp.tobytes()


def reach_class(s, p):
    sets, mp = Motif(s, p).stripped_sets()
    r = max(mp, len(sets) - 1 - mp)
    return 0 if r <= 31 else 1 if r <= 63 else 2


def _upload_metagenome(eng, mg, mod_types, low=0.3, high=0.7, min_cov=5):
    idx = list(range(len(mg.names)))
    eng.upload_assembly([mg.names[i] for i in idx], [mg.contig_ascii(i) for i in idx], [mg.bin_names[i] for i in idx])
    for mt in mod_types:
        first = True
        for local, i in enumerate(idx):
            p = mg.contig_pileup(i, mt)
            keep = p["nvalid"] > min_cov
            eng.upload_pileup(mt, np.full(int(keep.sum()), local, np.uint32), p["position"][keep], p["strand"][keep],
                              synth.pct_to_fraction(p["pct_hundredths"][keep]), low=low, high=high, append=not first)
            first = False


# ------------------------------------------------------------------------------------------------ tests
def test_literal_cases_of_the_parity_suite(engine_cls):
    """The two literal cases of tests/test_gpu_parity.py (reference tests/test_motif_find.py:14-39, tests/test_fasta.py:95-109)."""
    eng = engine_cls()
    eng.upload_assembly(["c"], ["TACGGACGCCACG"], ["b"])
    eng.upload_pileup("a", [0, 0, 0], [1, 5, 10], np.frombuffer(b"+++", np.uint8), [0.9, 0.95, 0.1])
    rec, tables, _ = collect(eng, [("ACG", 0, "a", "b")])
    fwd = rec[rec["code"] < 4]
    assert fwd["pos"][fwd["code"] == 0].tolist() == [1, 5] and fwd["pos"][fwd["code"] == 1].tolist() == [10]
    assert fwd["pos"].tolist() == [1, 5, 10] and set(rec["contig"].tolist()) == {0}
    # '-': CGT occurs nowhere in TACGGACGCCACG
    assert len(rec) == 3 and tables[0].tolist() == [[2, 1, 0, 0, 0, 0]]
    assert eng.motif_site_counts([(Motif("ACG", 0), "a", "b")])[0][1].tolist() == [[2, 1, 0, 0, 0, 0]]
    seq = "AATTAAATTAAGTAAAT"
    eng.upload_assembly(["c"], [seq], ["b"])
    eng.upload_pileup("a", np.zeros(len(seq), np.uint32), np.arange(len(seq)), np.full(len(seq), ord("+"), np.uint8), np.ones(len(seq)))
    rec, tables, _ = collect(eng, [("AA.T", 0, "a", "b"), ("AATT", 0, "a", "b")])
    a, b = rec[rec["candidate"] == 0], rec[rec["candidate"] == 1]
    assert a["pos"][a["code"] == 0].tolist() == [0, 4, 5, 9, 13] and b["pos"][b["code"] == 0].tolist() == [0, 5]
    # reverse complements A.TT / AATT shifted to the modified base (their last position) carry no call: no '-' row was uploaded
    assert a["pos"][a["code"] == 6].tolist() == [3, 8] and b["pos"][b["code"] == 6].tolist() == [3, 8]
    assert not np.isin(rec["code"], (1, 2, 4, 5)).any()
    from oracle.scan import ContigPileup
    pile = ContigPileup(np.arange(len(seq)), np.full(len(seq), ord("+"), np.uint8), np.ones(len(seq)))
    exp, _ = expected_records(eng, [("AA.T", 0, "a", "b"), ("AATT", 0, "a", "b")], {"c": seq}, {"a": {"c": pile}})
    assert_same_records(rec, exp)
    eng.close()


def test_g2_records_are_the_references_recorded_arrays(engine_cls):
    """Fixture g2 (recorded from the reference's motif_model_contig(save_motif_positions=True)): for EVERY case the records with state
    mod / nomod on '+' / '-' are the four recorded arrays and what hit_positions returns; all three states per strand are subseq_indices
    of the stripped motif (its reverse complement) shifted to the modified base."""
    from oracle.motif import Motif as OMotif
    from oracle.scan import subseq_indices
    g = load_golden("g2_motif_model_contig.json")
    mg = synth.make_metagenome(spec_from_json(g["spec"]))
    seq = mg.contig_str(0)
    assert hashlib.sha1(seq.encode()).hexdigest() == g["seq_sha1"]
    n_checked = 0
    for (low, high) in ((0.3, 0.7), (0.1, 0.9)):
        eng = engine_cls()
        _upload_metagenome(eng, mg, ("a", "m"), low=low, high=high, min_cov=-1)
        cases = [c for c in g["cases"] if (c["low"], c["high"]) == (low, high)]
        assert len(cases) > 10
        cands = [(c["motif"], c["pos"], c["mod_type"], mg.bin_names[0]) for c in cases]
        rec, tables, _ = collect(eng, cands)
        off = np.searchsorted(rec["candidate"], np.arange(len(cases) + 1))
        for k, c in enumerate(cases):
            r = rec[off[k]:off[k + 1]]
            r = r[r["contig"] == 0]
            for which, key in enumerate(KEYS):
                pos = r["pos"][r["code"] == (which // 2) * 4 + which % 2].astype(np.int64)
                assert len(pos) == c[key]["n"] and sha1(pos) == c[key]["sha1"], (c["motif"], key)
                assert np.array_equal(pos, eng.hit_positions(0, c["mod_type"], Motif(c["motif"], c["pos"]), which)), (c["motif"], key)
            st = OMotif(c["motif"], c["pos"]).new_stripped_motif()
            rc = st.reverse_compliment()
            assert np.array_equal(r["pos"][r["code"] < 4], subseq_indices(st.string, seq) + st.mod_position), c["motif"]
            assert np.array_equal(r["pos"][r["code"] >= 4], subseq_indices(rc.string, seq) + rc.mod_position), c["motif"]
            row = tables[k][eng.bin_contigs(mg.bin_names[0]).index(mg.names[0])]
            assert (row[0] + row[3], row[1] + row[4]) == (c["n_mod"], c["n_nomod"])
            n_checked += 1
        eng.close()
    assert n_checked == len(g["cases"])


WIDE_EXTRAS = [("A" + "." * 70 + "T", 0), ("C" + "." * 94 + "G", 95), ("G" + "." * 94 + "A", 0), ("T" + "." * 40 + "[AC]" + "." * 40 + "C", 41),
               ("A" + "." * 62 + "C", 0), ("G" + "." * 62 + "A", 63)]


def test_zoo_on_a_synthetic_metagenome_in_one_call(engine_cls):
    """>= 8 bins, two mod types, every helpers.motif_zoo() motif (plus far-reaching ones, so that all three kernel widths occur) on every
    bin in ONE call: records == the per-contig oracle in contract order; the count table agrees with score_per_contig and score."""
    spec = synth.SynthSpec(n_contigs=20, total_bp=500_000, n_bins=8, mod_types=("a", "m"), seed=77, min_contig_bp=3_000, n_fraction=0.002,
                           fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m"), ("GCACNNNNNNGTT", 2, "a")))
    mg = synth.make_metagenome(spec)
    bins = sorted(set(mg.bin_names))
    assert len(bins) >= 8 and int(mg.lengths.sum()) <= 1_000_000
    eng = engine_cls()
    _upload_metagenome(eng, mg, ("a", "m"))
    motifs = motif_zoo() + WIDE_EXTRAS
    classes = [reach_class(s, p) for s, p in motifs]
    assert set(classes) == {0, 1, 2}, "all three kernel widths must occur"
    cands = [(s, p, "am"[k % 2], b) for b in bins for k, (s, p) in enumerate(motifs)]
    piles, seqs = {}, {}
    for mt in ("a", "m"):
        piles[mt], seqs = oracle_bin_inputs(mg, mt)
    rec, tables, n_deliveries = collect(eng, cands)
    assert n_deliveries == 1
    exp, exp_tables = expected_records(eng, cands, seqs, piles)
    assert len(exp) > 1_000_000 and set(exp["code"].tolist()) == {0, 1, 2, 4, 5, 6}
    assert_same_records(rec, exp)
    assert len(tables) == len(cands)
    for k in range(len(cands)):
        assert np.array_equal(tables[k], exp_tables[k]), cands[k]
    ecands = [(Motif(s, p), mt, b) for s, p, mt, b in cands]
    per_contig = eng.score_per_contig(ecands)
    total = eng.score(ecands)
    counts = eng.motif_site_counts(ecands)
    for k in range(len(cands)):
        names, two = per_contig[k]
        assert counts[k][0] == names and np.array_equal(counts[k][1], tables[k])
        assert np.array_equal(tables[k][:, 0] + tables[k][:, 3], two[:, 0]) and np.array_equal(tables[k][:, 1] + tables[k][:, 4], two[:, 1]), cands[k]
        assert (tables[k][:, [0, 3]].sum(), tables[k][:, [1, 4]].sum()) == tuple(total[k].tolist()), cands[k]
    # a selection of states is the same records with the others left out
    for states in (("mod",), ("nomod", "nocall"), ("nocall",)):
        sub = cands[::37]
        got, _, _ = collect(eng, sub, states=states)
        exp_sub, _ = expected_records(eng, sub, seqs, piles, states=states)
        assert_same_records(got, exp_sub, states)
    eng.close()


def _layout_case():
    rng = np.random.default_rng(12)
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    big = list(rand(60_000))                                            # spans eight chunks of 8192
    big[8185:8200] = "N" * 15                                           # an N run across a chunk border
    big[8170:8185] = "GATCGATCGATCGAT"                                  # ... with occurrences right before it
    big[8200:8204] = "GATC"
    big[16380:16390] = "AAAAAAAAAA"                                     # overlapping occurrences across a chunk border
    big[24574:24578] = "GATC"                                           # a palindrome astride a chunk border
    seqs = {"big": "".join(big), "tiny1": "G", "tiny2": "GA", "tiny3": "ATC", "ends_GA": rand(9000) + "GA", "starts_TC": "TC" + rand(500),
            "pal": "GATC" * 50 + "AATT" * 30, "n_only": "N" * 40, "edge": "GATC" + rand(8192 - 8) + "GATC", "edge2": rand(8191) + "A",
            "other_bin": "GATC" + rand(3000) + "GA", "other_bin2": "TC" + rand(100)}
    bins = {n: ("b2" if n.startswith("other") else "b1") for n in seqs}
    return seqs, bins, rng


def test_layouts_that_break_naive_chunking(engine_cls):
    """A contig over many chunks, contigs shorter than the motif, an N run across a chunk border, an occurrence that would straddle two
    neighbouring contigs (GA|TC: must not appear), overlapping occurrences, a palindrome (both strands at neighbouring positions)."""
    from oracle.scan import ContigPileup
    seqs, bins, rng = _layout_case()
    names = list(seqs)
    eng = engine_cls()
    eng.upload_assembly(names, [seqs[n] for n in names], [bins[n] for n in names])
    piles = {"a": {}, "m": {}}
    for mt in ("a", "m"):
        cid, pos, st, fr = [], [], [], []
        for i, n in enumerate(names):
            L = len(seqs[n])
            p = np.sort(rng.choice(L, size=max(1, L // 2), replace=False)).astype(np.int64)
            strand = rng.choice(np.array([ord("+"), ord("-")], dtype=np.uint8), size=len(p))
            f = rng.choice([0.0, 0.3, 0.30000000000000004, 0.5, 0.7, 0.6999999999999999, 1.0], size=len(p))
            piles[mt][n] = ContigPileup(p, strand, f)
            cid += [i] * len(p); pos += p.tolist(); st += strand.tolist(); fr += f.tolist()
        eng.upload_pileup(mt, cid, pos, np.array(st, np.uint8), fr)
    motifs = [("GATC", 1), ("GATC", 0), ("AA", 0), ("AA", 1), ("A", 0), ("AATT", 1), ("GA.C", 1), ("G[AG]TC", 1), ("A.........A", 0),
              ("G" + "." * 40 + "C", 0), ("A" + "." * 80 + "T", 81), ("T" + "." * 94 + "A", 0), ("ATC", 2), ("GAT[CG]", 3)]
    cands = [(s, p, mt, b) for b in ("b1", "b2") for mt in ("a", "m") for s, p in motifs]
    rec, tables, _ = collect(eng, cands)
    exp, exp_tables = expected_records(eng, cands, seqs, piles)
    assert_same_records(rec, exp)
    for k in range(len(cands)):
        assert np.array_equal(tables[k], exp_tables[k]), cands[k]
    # spelled out: GATC@1 on ends_GA | starts_TC — nothing at the seam
    k = cands.index(("GATC", 1, "a", "b1"))
    r = rec[rec["candidate"] == k]
    seam = r[(r["contig"] == names.index("ends_GA")) & (r["pos"] >= 9000)]
    assert len(seam) == 0 and not (r[r["contig"] == names.index("starts_TC")]["pos"] < 2).any()
    for n in ("tiny1", "tiny2", "tiny3", "n_only"):
        assert not (r["contig"] == names.index(n)).any()
    pal = r[r["contig"] == names.index("pal")]
    assert pal["pos"][pal["code"] < 4][:3].tolist() == [1, 5, 9] and pal["pos"][pal["code"] >= 4][:3].tolist() == [2, 6, 10]
    big = r[r["contig"] == names.index("big")]
    assert {8171, 8175, 8179, 8201, 24575} <= set(big["pos"][big["code"] < 4].tolist())
    assert not ((big["pos"] >= 8183) & (big["pos"] < 8200)).any()          # GAT|N..: the run of N holds no occurrence
    k = cands.index(("AA", 0, "a", "b1"))
    r = rec[(rec["candidate"] == k) & (rec["contig"] == names.index("big")) & (rec["code"] < 4)]
    assert set(range(16380, 16389)) <= set(r["pos"].tolist())
    eng.close()


def test_budget_and_windows_do_not_change_the_result(engine_cls):
    """max_records of 1 000, of one candidate's size minus one, and unlimited give the same concatenation; at the ABI consecutive windows of
    odd sizes tile the batch exactly and a window past the end writes nothing."""
    from nanomotif_amd import _lib
    from nanomotif_amd.engine import _ptr
    spec = synth.SynthSpec(n_contigs=6, total_bp=120_000, n_bins=2, mod_types=("a",), seed=5, min_contig_bp=3_000, fixed_motifs=(("GATC", 1, "a"),))
    mg = synth.make_metagenome(spec)
    eng = engine_cls()
    _upload_metagenome(eng, mg, ("a",))
    bins = sorted(set(mg.bin_names))
    motifs = [("GATC", 1), ("A", 0), ("AA", 0), ("G[AG].GAAG[CT]", 5), ("A" + "." * 70 + "T", 0), ("CC[AT]GG", 1), ("TTTTTTTTTTTT", 0)]
    cands = [(s, p, "a", b) for b in bins for s, p in motifs]
    piles, seqs = {}, {}
    piles["a"], seqs = oracle_bin_inputs(mg, "a")
    exp, _ = expected_records(eng, cands, seqs, piles)
    whole, tables, n = collect(eng, cands)
    assert n == 1
    assert_same_records(whole, exp)
    sizes = np.bincount(whole["candidate"], minlength=len(cands))
    assert sizes.max() > 20_000 and sizes.min() < 1_000                 # candidates above and below the small budgets
    for budget in (1_000, int(sizes[1]) - 1, int(sizes.max()) - 1, 10 ** 9):
        got, tables_b, n_b = collect(eng, cands, max_records=budget)
        assert_same_records(got, exp, budget)
        assert all(np.array_equal(x, y) for x, y in zip(tables_b, tables)) and len(tables_b) == len(tables)
        assert n_b > 1 or budget >= len(exp)
    # ---- the ABI: windows
    b = eng.make_batch([(Motif(s, p), mt, bn) for s, p, mt, bn in cands])
    total = len(exp)

    def window(first, cap):
        contig, pos, code = (np.full(max(cap, 1) + 8, 0xEE, dtype=t) for t in (np.uint32, np.uint32, np.uint8))
        off = np.zeros(len(b) + 1, dtype=np.uint64)
        nw = C.c_uint64(99)
        _lib.check(eng.lib.nm_motif_sites(eng.ctx, *eng._batch_args(b), 7, first, cap, _ptr(contig, C.c_uint32), _ptr(pos, C.c_uint32),
                                          _ptr(code, C.c_uint8), _ptr(off, C.c_uint64), C.byref(nw)))
        n_w = int(nw.value)
        assert n_w == max(0, min(cap, total - first))
        # nothing beyond what was reported is touched
        assert (code[n_w:] == 0xEE).all() and (pos[n_w:] == 0xEE).all() and (contig[n_w:] == 0xEE).all()
        assert np.array_equal(off.astype(np.int64), np.searchsorted(exp["candidate"], np.arange(len(cands) + 1)))
        return contig[:n_w], pos[:n_w], code[:n_w]
    for size in (1, 63, 65, 1_000):
        # consecutive windows of this size over a stretch that crosses candidate, contig and chunk boundaries
        start = max(0, int(np.searchsorted(exp["candidate"], 1)) - 2 * size - 1)
        at, parts = start, []
        for _ in range(6 if size < 1_000 else 40):
            parts.append(window(at, size))
            at += len(parts[-1][0])
        got = [np.concatenate([p[i] for p in parts]) for i in range(3)]
        assert at == min(total, start + len(got[0]))
        for i, f in enumerate(("contig", "pos", "code")):
            assert np.array_equal(got[i], exp[f][start:at]), (size, f)
    # windows that tile the whole batch
    at, parts = 0, []
    while at < total:
        parts.append(window(at, 65_537))
        at += len(parts[-1][0])
    assert at == total
    for i, f in enumerate(("contig", "pos", "code")):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), exp[f]), f
    # the last, short window; a window past the end; an empty window
    assert len(window(total - 5, 63)[0]) == 5
    assert len(window(total, 63)[0]) == 0 and len(window(total + 10_000, 1_000)[0]) == 0 and len(window(0, 0)[0]) == 0
    eng.close()


def test_errors_are_loud(engine_cls):
    from nanomotif_amd._lib import NmScanError
    eng = engine_cls()
    with pytest.raises(NmScanError) as e:                               # no assembly
        b = eng.make_batch([(Motif("GATC", 1), "a", 0)], slot_of=lambda mt: 0)
        list(eng.motif_sites(b))
    assert e.value.code == -3                                           # NM_ESTATE
    eng.upload_assembly(["c"], ["GATCGATC"], ["b"])
    with pytest.raises(NmScanError) as e:                               # no pileup in the slot
        list(eng.motif_sites(eng.make_batch([(Motif("GATC", 1), "a", "b")], slot_of=lambda mt: 0)))
    assert e.value.code == -3
    eng.upload_pileup("a", [0], [1], np.frombuffer(b"+", np.uint8), [1.0])
    with pytest.raises(NmScanError) as e:                               # reaches further than 95 from the modified base
        list(eng.motif_sites([(Motif("A" + "." * 100 + "T", 0), "a", "b")]))
    assert e.value.code == -5
    with pytest.raises(NmScanError) as e:
        list(eng.motif_sites(eng.make_batch([(Motif("GATC", 1), "a", 7)])))      # no such bin
    assert e.value.code == -1
    with pytest.raises(NmScanError) as e:                               # no such bin and no pileup in the slot: the bin is refused first
        list(eng.motif_sites(eng.make_batch([(Motif("GATC", 1), "a", 7)], slot_of=lambda mt: 5)))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        list(eng.motif_sites([(Motif("GATC", 1), "a", "b")], states=("methylated",)))
    assert eng.lib.nm_motif_sites(eng.ctx, 1, None, None, None, None, None, None, 7, 0, 0, None, None, None, None, None) == -1
    assert eng.lib.nm_motif_sites_count(eng.ctx, 1, None, None, None, None, None, None, 7, None, None, None) == -1
    rec = np.concatenate([sb.records for sb in eng.motif_sites([(Motif("GATC", 1), "a", "b")])])
    assert rec["pos"].tolist() == [1, 2, 5, 6] and rec["code"].tolist() == [0, 6, 2, 6]
    eng.close()


# ------------------------------------------------------------------------------------------------ the command
def _run(tmp, command, args, env_extra=None):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env_extra or {}))
    r = subprocess.run([sys.executable, "-m", "nanomotif_amd", command] + args, cwd=tmp, env=env, capture_output=True, text=True)
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


def _expected_files(mg, bin_motifs_text, low, high, states=STATES):
    """motif-sites.bed and the summary rows the oracle gives for the candidates of a bin-motifs.tsv."""
    from nanomotif_amd.motif import iupac_to_regex
    from oracle.scan import _EMPTY
    piles = _filtered_piles(mg)
    seqs = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    lines = bin_motifs_text.strip().split("\n")
    head = lines[0].split("\t")
    cands, seen = [], set()
    for line in lines[1:]:
        row = dict(zip(head, line.split("\t")))
        both = [(row["reference"], row["motif"], row["mod_type"], int(row["mod_position"]))]
        if row["motif_complement"]:
            both.append((row["reference"], row["motif_complement"], row["mod_type"], int(row["mod_position_complement"])))
        for c in both:
            if c not in seen:
                seen.add(c)
                cands.append(c)
    bed, summary = [], {}
    for b, motif, mt, pos in cands:
        for i, name in enumerate(mg.names):                             # contigs in contig_bin.tsv order
            if mg.bin_names[i] != b:
                continue
            p, code = oracle_contig_sites(seqs[name], piles[mt].get(name, _EMPTY), iupac_to_regex(motif), pos, low, high)
            summary[(b, name, motif, mt, pos)] = [int(((code >> 2 == j // 3) & (code & 3 == j % 3)).sum()) for j in range(6)]
            for q, cd in zip(p.tolist(), code.tolist()):
                if STATES[cd & 3] in states:
                    bed.append(f"{name}\t{q}\t{q + 1}\t{motif}_{mt}_{pos}\t0\t{'-' if cd & 4 else '+'}\t{STATES[cd & 3]}\t{b}\n")
    return "".join(bed), summary, cands


def _read_summary(path):
    lines = open(path).read().strip().split("\n")
    head = lines[0].split("\t")
    assert head == ["bin", "contig", "motif", "mod_type", "mod_position", "n_mod_fwd", "n_nomod_fwd", "n_nocall_fwd", "n_mod_rev", "n_nomod_rev",
                    "n_nocall_rev", "n_mod", "n_nomod", "n_nocall"]
    out = {}
    for line in lines[1:]:
        f = line.split("\t")
        key = (f[0], f[1], f[2], f[3], int(f[4]))
        assert key not in out
        out[key] = [int(x) for x in f[5:]]
        assert out[key][6:] == [out[key][0] + out[key][3], out[key][1] + out[key][4], out[key][2] + out[key][5]]
    return out


def _check_identity_with_bin_motifs(bin_motifs_text, summary):
    """For every row of bin-motifs.tsv: the summary's n_mod / n_nomod summed over the bin's contigs are the row's (and the _complement
    columns for the complement candidate)."""
    lines = bin_motifs_text.strip().split("\n")
    head = lines[0].split("\t")
    assert len(lines) > 3
    for line in lines[1:]:
        row = dict(zip(head, line.split("\t")))
        pairs = [((row["reference"], row["motif"], row["mod_type"], int(row["mod_position"])), (int(row["n_mod"]), int(row["n_nomod"])))]
        if row["motif_complement"]:
            pairs.append(((row["reference"], row["motif_complement"], row["mod_type"], int(row["mod_position_complement"])),
                          (int(row["n_mod_complement"]), int(row["n_nomod_complement"]))))
        for (b, motif, mt, pos), want in pairs:
            rows = [v for k, v in summary.items() if (k[0], k[2], k[3], k[4]) == (b, motif, mt, pos)]
            assert rows, (b, motif)
            got = (sum(v[6] for v in rows), sum(v[7] for v in rows))
            print("identity", b, motif, mt, pos, "bin-motifs", want, "summary", got)
            assert got == want, (b, motif, mt, pos, got, want)


def test_command_after_motif_discovery(tmp_path):
    """motif_discovery then motif_sites on files written the way tests/test_gpu_cli.py writes them, plain and bgzip + tabix:
    motif-sites.bed is byte-equal to the oracle's text and the summary sums to the rows of bin-motifs.tsv."""
    from helpers import write_bgzf_tabix
    spec = synth.SynthSpec(n_contigs=4, total_bp=500_000, n_bins=2, mod_types=("a", "m"), seed=61, min_contig_bp=60_000,
                           fixed_motifs=(("GATC", 1, "a"), ("ACCCA", 4, "a"), ("GRNGAAGY", 5, "a"), ("CCWGG", 1, "m")))
    mg = synth.make_metagenome(spec)
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_bed(tmp + "/pileup.bed")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    write_bgzf_tabix(open(tmp + "/pileup.bed", "rb").read(), tmp + "/pileup.bed.gz", block_size=50_000)
    for pileup, out in (("pileup.bed", "plain"), ("pileup.bed.gz", "gz")):
        _run(tmp, "motif_discovery", ["assembly.fasta", pileup, "-c", "contig_bin.tsv", "--out", out])
        bm = open(f"{tmp}/{out}/bin-motifs.tsv").read()
        motifs = {l.split("\t")[1] for l in bm.strip().split("\n")[1:]}
        assert {"GATC", "ACCCA", "CCWGG"} <= motifs
        assert any(l.split("\t")[7] for l in bm.strip().split("\n")[1:]), "no row with a complement"
        r = _run(tmp, "motif_sites", ["assembly.fasta", pileup, "-c", "contig_bin.tsv", "--bin_motifs", f"{out}/bin-motifs.tsv", "--out", out + "_sites"])
        bed, exp_summary, cands = _expected_files(mg, bm, 0.3, 0.7)
        got_bed = open(f"{tmp}/{out}_sites/motif-sites.bed").read()
        assert len(got_bed) == len(bed) and got_bed == bed, (pileup, len(got_bed), len(bed))
        assert {l.split("\t")[6] for l in bed.split("\n")[:-1]} == set(STATES)
        summary = _read_summary(f"{tmp}/{out}_sites/motif-sites-summary.tsv")
        assert {k: v[:6] for k, v in summary.items()} == exp_summary
        assert list(summary) == [(b, n, m, mt, p) for b, m, mt, p in cands for i, n in enumerate(mg.names) if mg.bin_names[i] == b]
        _check_identity_with_bin_motifs(bm, summary)
        assert os.path.exists(f"{tmp}/{out}_sites/args.motif_sites.json") and os.path.exists(f"{tmp}/{out}_sites/logs/timings.motif_sites.json")
    # --states: the same lines with the other states left out
    _run(tmp, "motif_sites", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "plain/bin-motifs.tsv", "--out", "nomod_sites",
                              "--states", "nomod"])
    bm = open(tmp + "/plain/bin-motifs.tsv").read()
    assert open(tmp + "/nomod_sites/motif-sites.bed").read() == _expected_files(mg, bm, 0.3, 0.7, states=("nomod",))[0]
    assert open(tmp + "/nomod_sites/motif-sites-summary.tsv").read() == open(tmp + "/plain_sites/motif-sites-summary.tsv").read()


def test_command_with_other_thresholds(tmp_path):
    """Non-default thresholds: the sites are classified at the thresholds given (BED and summary equal the oracle at 0.2 / 0.85), and the rows
    of bin-motifs.tsv that motif_discovery scored at those thresholds sum up.  (motif_discovery scores the motifs its merge stage makes on
    a second classification fixed at 0.3 / 0.7, find_motifs_bin.py:569, and a complement's columns are its partner row's: a row must agree
    with this run or with a motif_sites run at 0.3 / 0.7 on the same files, and rows of the first kind must exist.)"""
    spec = synth.SynthSpec(n_contigs=4, total_bp=400_000, n_bins=2, mod_types=("a", "m"), seed=62, min_contig_bp=60_000,
                           fixed_motifs=(("GATC", 1, "a"), ("GRNGAAGY", 5, "a"), ("CCWGG", 1, "m")))
    mg = synth.make_metagenome(spec)
    tmp = str(tmp_path)
    mg.write_fasta(tmp + "/assembly.fasta")
    mg.write_bed(tmp + "/pileup.bed")
    mg.write_contig_bin(tmp + "/contig_bin.tsv")
    thr = ["--methylation_threshold_low", "0.2", "--methylation_threshold_high", "0.85"]
    _run(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"] + thr)
    bm = open(tmp + "/out/bin-motifs.tsv").read()
    assert len(bm.strip().split("\n")) > 3
    _run(tmp, "motif_sites", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "sites"] + thr)
    bed, exp_summary, _ = _expected_files(mg, bm, 0.2, 0.85)
    assert open(tmp + "/sites/motif-sites.bed").read() == bed
    summary = _read_summary(tmp + "/sites/motif-sites-summary.tsv")
    assert {k: v[:6] for k, v in summary.items()} == exp_summary
    _run(tmp, "motif_sites", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "sites_merge"])
    merge = _read_summary(tmp + "/sites_merge/motif-sites-summary.tsv")
    lines = bm.strip().split("\n")
    head = lines[0].split("\t")
    n_own = 0
    for line in lines[1:]:
        row = dict(zip(head, line.split("\t")))
        key = (row["reference"], row["motif"], row["mod_type"], int(row["mod_position"]))
        sums = lambda table: (sum(v[6] for k, v in table.items() if (k[0], k[2], k[3], k[4]) == key),
                              sum(v[7] for k, v in table.items() if (k[0], k[2], k[3], k[4]) == key))
        want = (int(row["n_mod"]), int(row["n_nomod"]))
        print("thresholds", key, "bin-motifs", want, "at 0.2/0.85", sums(summary), "at 0.3/0.7", sums(merge))
        assert want in (sums(summary), sums(merge)), key
        n_own += want == sums(summary)
        if row["motif_complement"]:
            key = (row["reference"], row["motif_complement"], row["mod_type"], int(row["mod_position_complement"]))
            want = (int(row["n_mod_complement"]), int(row["n_nomod_complement"]))          # (the partner row's own counts, postprocess.py:85-109)
            print("thresholds, complement", key, "bin-motifs", want, "at 0.2/0.85", sums(summary), "at 0.3/0.7", sums(merge))
            assert want in (sums(summary), sums(merge)), key
    assert n_own > 0
