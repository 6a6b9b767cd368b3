"""Narrow compact non-literal heavy batches (the headline kernel and its per-contig twin) take every IUPAC set of one, two or
three bases as ONE constraint on the class planes is-A/C/G/T, H, L, X = H ^ L: a positive sense (acc &= plane) or a negative one
(acc &= ~plane), the reverse strand from a compile-time mirror of the forward class words.  An all-valid chunk never looks at V;
a boundary chunk does, and nothing but V keeps an invalid position out of a negative class.  Bit-exact against the oracle: every
class at every narrow offset, invalid positions of every kind around A and C sites, mixed programs, per-contig counters, and the
8-plane path (NM_SCORE_CLASSES=0, read at call time) against the class path."""
import numpy as np
import pytest

from helpers import oracle_bin_inputs
from nanomotif_amd import synth
from nanomotif_amd.motif import Motif

pytestmark = pytest.mark.gpu

LITERALS = ["A", "C", "G", "T"]
TWO_SETS = ["[GT]", "[AC]", "[CG]", "[AT]", "[CT]", "[AG]"]           # H, ~H, L, ~L, X, ~X on the code A=00 C=01 G=11 T=10
THREE_SETS = ["[CGT]", "[AGT]", "[ACT]", "[ACG]"]                     # ~A, ~C, ~G, ~T
ALL_SETS = LITERALS + TWO_SETS + THREE_SETS
NEGATIVE = ["[AC]", "[AT]", "[AG]"] + THREE_SETS                      # the classes an invalid position could slip into
POSITIVE = LITERALS + ["[GT]", "[CG]", "[CT]"]
CANONICAL = {"a": "A", "m": "C"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _motif(mod_set, others):
    """(motif string, mod_position): `mod_set` at the modified position, (offset from it, set) for the rest."""
    lo = min([0] + [d for d, _ in others])
    hi = max([0] + [d for d, _ in others])
    pos = ["."] * (hi - lo + 1)
    pos[-lo] = mod_set
    for d, s in others:
        pos[d - lo] = s
    return "".join(pos), -lo


def _entry(mt, others):
    return _motif(CANONICAL[mt], others) + (mt,)


# ---- the two inputs -----------------------------------------------------------------------------------------------------
class Scene:
    """An engine with an assembly and both pileups resident, the oracle's inputs per (bin, mod type), and the oracle's
    answers, computed once per zoo entry and shared by the tests."""

    def __init__(self, eng, bins, inputs):
        self.eng, self.bins, self.inputs = eng, bins, inputs
        self._want, self._want_pc = {}, {}

    def want(self, b, s, p, mt):
        from oracle.scan import score_candidates
        key = (b, s, p, mt)
        if key not in self._want:
            pile, seqs = self.inputs[(b, mt)]
            self._want[key] = score_candidates(pile, seqs, [(s, p)])[0]
        return self._want[key]

    def want_per_contig(self, b, s, p, mt):
        from oracle.contig_methylation import per_contig_counts
        key = (b, s, p, mt)
        if key not in self._want_pc:
            pile, seqs = self.inputs[(b, mt)]
            self._want_pc[key] = per_contig_counts(pile, seqs, s, p)
        return self._want_pc[key]


@pytest.fixture(scope="module")
def scene():
    """The 64 kbp / 4-contig / 2-bin scene of test_gpu_strand_walk.py."""
    from nanomotif_amd.engine import ScanEngine
    spec = synth.SynthSpec(n_contigs=4, total_bp=64_000, n_bins=2, mod_types=("a", "m"), seed=77, min_contig_bp=10_000,
                           fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m")))
    mg = synth.make_metagenome(spec)
    eng = ScanEngine(0)
    eng.upload_assembly(mg.names, [mg.contig_ascii(i) for i in range(len(mg.names))], mg.bin_names)
    for mt in ("a", "m"):
        cols = mg.pileup_columns(mt)
        keep = cols["nvalid"] > 5
        eng.upload_pileup(mt, cols["contig_id"][keep], cols["position"][keep], cols["strand"][keep], cols["fraction_mod"][keep])
    bins = sorted(set(mg.bin_names))
    inputs = {}
    for b in bins:
        idx = [i for i, x in enumerate(mg.bin_names) if x == b]
        for mt in ("a", "m"):
            inputs[(b, mt)] = oracle_bin_inputs(mg, mt, contigs=idx)
    yield Scene(eng, bins, inputs)
    eng.close()


INVALID_LETTERS = "NRYKMSW"
CHUNK = 8192


def _dirty(seq, lo, hi):
    """Invalid letters around A / C / T / G sites of seq[lo:hi] (a chunk, or a short contig): 1..14 bp either side of a site,
    in the first and the last word, across the lane boundary 127 | 128, runs of N of length 1, 2 and 40."""
    n = hi - lo
    anchors = "ACTG"
    at = 0
    for k in range(1, 15):                              # an invalid letter k bp right of one site and k bp left of the next
        for side in (+1, -1):
            pos = lo + 200 + 61 * at
            if pos + 15 >= hi or pos - 15 < lo:
                break
            seq[pos] = ord(anchors[at % 4])
            seq[pos + side * k] = ord(INVALID_LETTERS[at % len(INVALID_LETTERS)])
            at += 1
    if n >= CHUNK - 1:
        seq[lo + 2] = ord("N")                          # run of 1 in the first word, a site 3 bp to its right
        seq[lo + 5] = ord("A")
        seq[lo + 9] = ord("C")
        seq[lo + 20] = ord("r")                         # (lower case ambiguity code)
        seq[lo + 127:lo + 129] = ord("N")               # run of 2 across the lane boundary 127 | 128
        seq[lo + 120] = ord("A")
        seq[lo + 125] = ord("C")
        seq[lo + 131] = ord("A")
        seq[lo + 137] = ord("G")
        seq[lo + 255] = ord("Y")                        # the letter left of a lane boundary, a site right of it
        seq[lo + 257] = ord("C")
        seq[lo + 384] = ord("K")                        # the letter right of a lane boundary, a site left of it
        seq[lo + 380] = ord("A")
        seq[hi - 48:hi - 8] = ord("N")                  # run of 40 that ends in the last word
        seq[hi - 52] = ord("A")
        seq[hi - 50] = ord("C")
        seq[hi - 6] = ord("A")
        seq[hi - 4] = ord("T")
        seq[hi - 2] = ord("S")                          # last word
    else:
        seq[lo + 30:lo + 32] = ord("N")
        seq[lo + 33] = ord("A")
        seq[lo + 60] = ord("W")
        seq[lo + 58] = ord("C")


@pytest.fixture(scope="module")
def hand():
    """A hand-made assembly, uploaded as strings.  Which contig serves which chunk path of the class kernels:
      full8192, full16384   chunks that are full but whose halo is the gap: boundary path (needs_v != 0) in every chunk
      over8193, under8191   a last chunk of 1 bp / a chunk one short of full: boundary path
      tiny100               boundary path
      long45000             six chunks: 0 and 5 are the contig's first and last and 1 holds invalid letters (boundary path); 2 and
                            4 are valid but have an invalid letter within three words of them (boundary path); chunk 3 takes
                            the ALL-VALID path (needs_v == 0: the chunk and three words either side of it are valid)
    Lower-case bases everywhere (valid once upper-cased, as the reference reads them)."""
    from nanomotif_amd.engine import ScanEngine
    from oracle.scan import ContigPileup
    rng = np.random.default_rng(20)
    lengths = {"full8192": 8192, "full16384": 16384, "over8193": 8193, "under8191": 8191, "tiny100": 100, "long45000": 45000}
    bin_of = {"full8192": "b0", "full16384": "b1", "over8193": "b0", "under8191": "b1", "tiny100": "b0", "long45000": "b1"}
    names = list(lengths)
    seqs = {}
    for name in names:
        n = lengths[name]
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
        if name == "long45000":
            for lo in (0, CHUNK, 5 * CHUNK):
                _dirty(seq, lo, min(lo + CHUNK, n))
        else:
            for lo in range(0, n, CHUNK):
                if n - lo >= 64:
                    _dirty(seq, lo, min(lo + CHUNK, n))
        lower = rng.random(n) < 0.05
        seq[lower] |= 0x20
        seqs[name] = seq.tobytes().decode()
    eng = ScanEngine(0)
    eng.upload_assembly(names, [seqs[n] for n in names], [bin_of[n] for n in names])
    piles = {"a": {}, "m": {}}
    for mt, pair in (("a", "AT"), ("m", "CG")):
        cid, pos, strand, frac = [], [], [], []
        for i, name in enumerate(names):
            up = np.frombuffer(seqs[name].upper().encode(), dtype=np.uint8)
            at = np.flatnonzero((up == ord(pair[0])) | (up == ord(pair[1])))
            p = np.repeat(at, 2)                                             # a row on either strand of every such position
            s = np.tile(np.frombuffer(b"+-", dtype=np.uint8), len(at))
            f = (np.arange(len(p)) // 2 + np.arange(len(p))) % 2 * 1.0       # 0.0 / 1.0: a false site changes a count
            cid.append(np.full(len(p), i, np.uint32)); pos.append(p); strand.append(s); frac.append(f)
            piles[mt][name] = ContigPileup(p.astype(np.int64), s, f.astype(np.float64))
        eng.upload_pileup(mt, np.concatenate(cid), np.concatenate(pos), np.concatenate(strand), np.concatenate(frac))
    bins = sorted(set(bin_of.values()))
    inputs = {}
    for b in bins:
        mine = [n for n in names if bin_of[n] == b]
        for mt in ("a", "m"):
            inputs[(b, mt)] = ({n: piles[mt][n] for n in mine}, {n: seqs[n].upper() for n in mine})
    yield Scene(eng, bins, inputs)
    eng.close()


def _check(sc, zoo, per_contig=False):
    """zoo: (string, mod_position, mod_type); every bin scores the whole zoo in ONE batch (a heavy one: > 6 per group)."""
    per_type = [sum(t == mt for _, _, t in zoo) for mt in ("a", "m")]
    assert all(n == 0 or n > 6 for n in per_type)
    cands = [(Motif(s, p), mt, b) for b in sc.bins for s, p, mt in zoo]
    if per_contig:
        got = sc.eng.score_per_contig(cands)
        k = 0
        total = 0
        for b in sc.bins:
            for s, p, mt in zoo:
                names, table = got[k]
                want = sc.want_per_contig(b, s, p, mt)
                assert table.tolist() == [list(want[n]) for n in names], (b, s, p, mt)
                total += int(table.sum())
                k += 1
        assert total > 0
        return None
    got = sc.eng.score(cands)
    want = np.asarray([sc.want(b, s, p, mt) for b in sc.bins for s, p, mt in zoo])
    bad = [(cands[i][0].string, cands[i][0].mod_position, cands[i][1], cands[i][2], got[i].tolist(), want[i].tolist())
           for i in range(len(cands)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad[:10]
    assert want.sum() > 0
    return got


# ---- test 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt", ["a", "m"])
@pytest.mark.parametrize("s", ALL_SETS)
def test_every_class_at_every_narrow_offset(scene, mt, s):
    """One constraint beside the canonical base: each of the 14 sets at every offset -31..31 — the mirror map and the
    r / 32 - r rule of every class word, both senses.  (One case per set and mod type: the oracle's regex scans are a second
    per case.)"""
    zoo = [_entry(mt, [(d, s)]) for d in range(-31, 32) if d != 0]
    _check(scene, zoo)


# ---- test 2 ---------------------------------------------------------------------------------------------------------------
def _invalid_zoo(mt):
    zoo = []                                               # (entry, [(offset, set), ...], mod type)
    for s in NEGATIVE + POSITIVE:
        for d in (1, -1, 2, -2, 14, -14, 31, -31):
            zoo.append((_entry(mt, [(d, s)]), [(d, s)], mt))
    # negative classes only: nothing but V keeps an invalid position out
    for others in ([(1, "[AC]"), (-1, "[AT]")], [(2, "[AG]"), (3, "[CGT]"), (-2, "[AGT]")], [(-1, "[ACT]"), (1, "[ACG]")],
                   [(d, s) for d, s in zip((1, 2, 3, 4, 5, 6, 7), NEGATIVE)], [(-d, s) for d, s in zip((1, 2, 3, 4, 5, 6, 7), NEGATIVE)],
                   [(14, "[AT]"), (-14, "[AC]"), (13, "[AG]")], [(31, "[ACG]"), (-31, "[CGT]"), (30, "[AC]")]):
        zoo.append((_entry(mt, others), others, mt))
    return zoo


def _forward_sites(seq, mt, others, lenient):
    """numpy re-count of the forward-strand sites of a motif in an upper-cased contig; lenient: an invalid position passes
    for a member of every NEGATIVE class (what a kernel without V would compute)."""
    up = np.frombuffer(seq.encode(), dtype=np.uint8)
    n = len(up)
    valid = np.isin(up, np.frombuffer(b"ACGT", dtype=np.uint8))
    lo = min([0] + [d for d, _ in others]); hi = max([0] + [d for d, _ in others])
    if n < hi - lo + 1:
        return 0
    i = np.arange(-lo, n - hi)                              # modified positions at which the motif fits inside the contig
    ok = up[i] == ord(CANONICAL[mt])
    for d, s in others:
        member = np.isin(up[i + d], np.frombuffer(s.strip("[]").encode(), dtype=np.uint8))
        if lenient and s in NEGATIVE:
            member |= ~valid[i + d]
        ok &= member
    return int(ok.sum())


@pytest.mark.parametrize("mt", ["a", "m"])
def test_invalid_positions(hand, mt):
    """Every class at offsets +-1, +-2, +-14, +-31 and motifs of negative classes only, for one mod type per case.  N runs, ambiguity codes and lower-case bases 1..14 bp either side of A and C sites, in first and last words and across a
    lane boundary, in contigs of exactly one and two chunks, one over, one under, 100 bp and six chunks (both chunk paths)."""
    zoo = _invalid_zoo(mt)
    entries = [e for e, _, _ in zoo]
    # before the GPU run: the input tests what it is there for
    want = np.asarray([hand.want(b, s, p, mt) for b in hand.bins for s, p, mt in entries])
    assert want.sum() > 0
    for cls in NEGATIVE:
        gains = 0
        for (_, others, mt) in zoo:
            if not any(s == cls for _, s in others):
                continue
            for b in hand.bins:
                for seq in hand.inputs[(b, mt)][1].values():
                    gains += _forward_sites(seq, mt, others, True) - _forward_sites(seq, mt, others, False)
        assert gains > 0, cls
    _check(hand, entries)


# ---- tests 3 - 5 -----------------------------------------------------------------------------------------------------------
def _mixed_zoo():
    rng = np.random.default_rng(14)
    offsets = [d for d in range(-31, 32) if d != 0]
    zoo = []
    for n in range(1, 13):                                 # 1..12 constraints per strand from all 14 sets
        for rep in range(3):
            for mt in ("a", "m"):
                ds = rng.choice(offsets, size=n, replace=False)
                sets = [ALL_SETS[int(rng.integers(0, len(ALL_SETS)))] for _ in ds]
                zoo.append(_entry(mt, list(zip(ds.tolist(), sets))))
    for mt in ("a", "m"):
        zoo.append(_entry(mt, [(3, "[AG]"), (7, "[AG]")]))                              # two offsets in one class word
        zoo.append(_entry(mt, [(-3, "[CGT]"), (-7, "[CGT]"), (-20, "[CGT]")]))          # three
        zoo.append(_entry(mt, [(4, "[AG]"), (5, "[CT]")]))                              # X- and X+ at neighbouring offsets
        zoo.append(_entry(mt, [(-4, "[CT]"), (-5, "[AG]")]))
        zoo.append(_entry(mt, [(1, "[GT]"), (2, "[AC]"), (3, "[CG]"), (4, "[AT]"), (5, "[CT]"), (6, "[AG]")]))     # both senses of H, L, X
        zoo.append(_entry(mt, [(-1, "[GT]"), (-2, "[AC]"), (-3, "[CG]"), (-4, "[AT]"), (-5, "[CT]"), (-6, "[AG]")]))
        zoo.append(_entry(mt, [(1, "G"), (-2, "T"), (9, "C")]))                         # literals only, among class candidates: the summary skip
        zoo.append(_entry(mt, [(-1, "A")]))
    return zoo


def _class_only_zoo():
    """A group in which every candidate has class constraints."""
    zoo = []
    for mt in ("a", "m"):
        for i, s in enumerate(TWO_SETS + THREE_SETS):
            zoo.append(_entry(mt, [(i + 1, s), (-(i + 2), (TWO_SETS + THREE_SETS)[(i + 3) % 10])]))
    return zoo


def test_mixed_programs(scene):
    _check(scene, _mixed_zoo())
    _check(scene, _class_only_zoo())


@pytest.mark.parametrize("which", ["scene", "hand"])
def test_per_contig_counters(which, request):
    """The zoo of the mixed programs through the per-contig kernel (the PC twin), on the scene and on the hand-made assembly."""
    sc = request.getfixturevalue(which)
    _check(sc, _mixed_zoo(), per_contig=True)


def test_old_path_against_new(scene, hand, monkeypatch):
    """NM_SCORE_CLASSES=0 sends the same batches down the 8-plane path; it is read at every call."""
    for sc in (scene, hand):
        zoo = _mixed_zoo()
        new = _check(sc, zoo)
        monkeypatch.setenv("NM_SCORE_CLASSES", "0")
        old = _check(sc, zoo)
        monkeypatch.delenv("NM_SCORE_CLASSES")
        again = _check(sc, zoo)
        assert np.array_equal(old, new) and np.array_equal(again, new)
