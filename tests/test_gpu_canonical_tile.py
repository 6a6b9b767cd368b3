"""The class tile of the heavy narrow compact kernels is built canonical-first: a workgroup's mod slot decides a flip of L
(A <-> C, G <-> T on the stored code), so that plane 0 is the slot's canonical base and plane 3 its complement, the walk
starts from those two planes, and the compiler swaps every base set of a C-slot candidate the same way.  Bit for bit against
the oracle: both slot columns in ONE launch, every one of the 14 sets at the far and the near offsets for `m` (every row of
the swap) and for `a` (no swap), a candidate of four classes, invalid letters next to C and G sites in boundary chunks (the
flipped L of an invalid position is 1 before V masks it), an all-valid middle chunk, the per-contig twin, and the 8-plane
path (NM_SCORE_CLASSES=0) against the class path."""
import numpy as np
import pytest

from nanomotif_amd.motif import Motif

pytestmark = pytest.mark.gpu

CHUNK = 8192
LITERALS = ["A", "C", "G", "T"]
TWO_SETS = ["[GT]", "[AC]", "[CG]", "[AT]", "[CT]", "[AG]"]           # H+, H-, L+, L-, X+, X- on the code A=00 C=01 G=11 T=10
THREE_SETS = ["[CGT]", "[AGT]", "[ACT]", "[ACG]"]                     # A-, C-, G-, T-
ALL_SETS = LITERALS + TWO_SETS + THREE_SETS
NEGATIVE = ["[AC]", "[AT]", "[AG]"] + THREE_SETS                      # the classes an invalid position could slip into
CANONICAL = {"a": "A", "m": "C"}
FAR_NEAR = (-31, -1, 1, 31)
AROUND = (-31, -2, -1, 1, 2, 31)                                      # invalid letters this far from C and G sites


def _entry(mt, others):
    """(motif string, mod_position, mod type): the canonical base at the modified position, (offset from it, set) for the rest."""
    lo = min([0] + [d for d, _ in others])
    hi = max([0] + [d for d, _ in others])
    pos = ["."] * (hi - lo + 1)
    pos[-lo] = CANONICAL[mt]
    for d, s in others:
        pos[d - lo] = s
    return "".join(pos), -lo, mt


FOUR_CLASSES = [(-31, "[GT]"), (-1, "[AT]"), (1, "[ACG]"), (31, "G")]   # H+, L-, T- and a literal in one candidate


def _zoo():
    """[(entry, [(offset, set), ...])]: for either mod type each set in a candidate of its own at -31, -1, 1, 31, one candidate of
    four classes, and the negative classes at the offsets of the planted invalid letters."""
    zoo = []
    for mt in ("a", "m"):
        for s in ALL_SETS:
            for d in FAR_NEAR:
                zoo.append((_entry(mt, [(d, s)]), [(d, s)]))
        zoo.append((_entry(mt, FOUR_CLASSES), FOUR_CLASSES))
    for s in NEGATIVE:
        for d in (-2, 2):                                              # (+-1 and +-31 are in the block above)
            zoo.append((_entry("m", [(d, s)]), [(d, s)]))
    return zoo


def _plant(seq, anchor, letter, phase):
    """An invalid letter at `anchor` and C / G sites at every distance of AROUND from it that lies inside the contig."""
    for i, k in enumerate(AROUND):
        if 0 <= anchor + k < len(seq):
            seq[anchor + k] = ord("CG"[(i + phase) % 2])
    seq[anchor] = ord(letter)


class Scene:
    def __init__(self, eng, names, seqs, piles):
        self.eng, self.names, self.seqs, self.piles = eng, names, seqs, piles
        self.zoo = _zoo()
        self.entries = [e for e, _ in self.zoo]
        self._want = self._want_pc = None

    def want(self):
        """int64[n, 2], the oracle's counts of every entry; computed once."""
        from oracle.scan import score_candidates
        if self._want is None:
            out = np.zeros((len(self.entries), 2), dtype=np.int64)
            for mt in ("a", "m"):
                idx = [i for i, e in enumerate(self.entries) if e[2] == mt]
                out[idx] = score_candidates(self.piles[mt], self.seqs, [self.entries[i][:2] for i in idx])
            self._want = out
        return self._want

    def want_per_contig(self):
        from oracle.contig_methylation import per_contig_counts
        if self._want_pc is None:
            self._want_pc = [per_contig_counts(self.piles[mt], self.seqs, s, p) for s, p, mt in self.entries]
        return self._want_pc

    def cands(self):
        return [(Motif(s, p), mt, "bin0") for s, p, mt in self.entries]


@pytest.fixture(scope="module")
def scene():
    """One bin, three contigs, lower-case free.  Which chunk takes which body of the class kernels:
      long     3 x 8192 + 100 bp: chunk 0 (invalid letters in its first word and across the lane border 127 | 128), chunk 2 (in its
               last word) and the 100 bp of chunk 3 are boundary chunks; chunk 1 and three words either side of it are valid: the
               ALL-VALID body
      short    1000 bp, a run of two N across 127 | 128: boundary body
      exact    8192 bp, invalid letters in its first and its last word and right of 127 | 128: boundary body"""
    from nanomotif_amd.engine import ScanEngine
    from oracle.scan import ContigPileup
    rng = np.random.default_rng(16)
    lengths = {"long": 3 * CHUNK + 100, "short": 1000, "exact": CHUNK}
    names = list(lengths)
    raw = {n: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=lengths[n])].copy() for n in names}
    for name, phase in (("long", 0), ("exact", 1)):
        seq, hi = raw[name], (3 * CHUNK if name == "long" else CHUNK)
        for anchor, letter in ((3, "N"), (12, "R"), (21, "W")):                       # first word of the contig's first chunk
            _plant(seq, anchor, letter, phase)
        for anchor, letter in ((hi - 4, "N"), (hi - 13, "R"), (hi - 22, "W")):        # last word of a full chunk
            _plant(seq, anchor, letter, phase)
    _plant(raw["long"], 127, "W", 0)                                                  # left of the lane border, sites across it
    _plant(raw["exact"], 128, "R", 1)                                                 # right of it
    _plant(raw["short"], 127, "N", 0)                                                 # a run of two across it
    _plant(raw["short"], 128, "N", 1)
    raw["short"][127] = ord("N")
    seqs = {n: raw[n].tobytes().decode() for n in names}
    long_ = seqs["long"]
    assert set(long_[CHUNK - 96:2 * CHUNK + 96]) <= set("ACGT")                       # chunk 1 stays on the all-valid body
    eng = ScanEngine(0)
    eng.upload_assembly(names, [seqs[n] for n in names], ["bin0"] * len(names))
    piles = {"a": {}, "m": {}}
    for mt, pair in (("a", "AT"), ("m", "CG")):
        cid, pos, strand, frac = [], [], [], []
        for i, name in enumerate(names):
            up = raw[name]
            at = np.flatnonzero((up == ord(pair[0])) | (up == ord(pair[1])))
            p = np.repeat(at, 2)                                             # a row on either strand of every such position
            s = np.tile(np.frombuffer(b"+-", dtype=np.uint8), len(at))
            f = (np.arange(len(p)) // 2 + np.arange(len(p))) % 2 * 1.0       # 0.0 / 1.0: a false site changes a count
            cid.append(np.full(len(p), i, np.uint32)); pos.append(p); strand.append(s); frac.append(f)
            piles[mt][name] = ContigPileup(p.astype(np.int64), s, f.astype(np.float64))
        eng.upload_pileup(mt, np.concatenate(cid), np.concatenate(pos), np.concatenate(strand), np.concatenate(frac))
    yield Scene(eng, names, seqs, piles)
    eng.close()


def _forward_sites(seq, mt, others, lenient):
    """numpy re-count of the forward-strand sites of a motif; lenient: an invalid position passes for a member of every
    NEGATIVE class (what a tile without V, or with L flipped after V, would compute)."""
    up = np.frombuffer(seq.encode(), dtype=np.uint8)
    n = len(up)
    valid = np.isin(up, np.frombuffer(b"ACGT", dtype=np.uint8))
    lo = min([0] + [d for d, _ in others]); hi = max([0] + [d for d, _ in others])
    i = np.arange(-lo, n - hi)
    ok = up[i] == ord(CANONICAL[mt])
    for d, s in others:
        member = np.isin(up[i + d], np.frombuffer(s.strip("[]").encode(), dtype=np.uint8))
        if lenient and s in NEGATIVE:
            member |= ~valid[i + d]
        ok &= member
    return int(ok.sum())


def test_input_tests_what_it_is_there_for(scene):
    """On the CPU, before any count of the device is believed: no class and sense passes on an all-zero table, and the invalid
    letters sit where a tile that forgets V would count them, for every negative class."""
    want = scene.want()
    for mt in ("a", "m"):
        for s in ALL_SETS:
            rows = [i for i, (e, others) in enumerate(scene.zoo) if e[2] == mt and others != FOUR_CLASSES and others[0][1] == s]
            assert len(rows) >= len(FAR_NEAR)
            assert all(want[i].sum() > 0 for i in rows), (mt, s)
            assert want[rows, 0].sum() > 0 and want[rows, 1].sum() > 0, (mt, s)
        four = [i for i, (e, others) in enumerate(scene.zoo) if e[2] == mt and others == FOUR_CLASSES]
        assert len(four) == 1 and want[four[0]].sum() > 0
    for s in NEGATIVE:
        for d in AROUND:
            gains = sum(_forward_sites(seq, "m", [(d, s)], True) - _forward_sites(seq, "m", [(d, s)], False)
                        for seq in scene.seqs.values())
            assert gains > 0, (s, d)
            assert any(e[2] == "m" and others == [(d, s)] for e, others in scene.zoo), (s, d)


def _score(scene):
    got = np.asarray(scene.eng.score(scene.cands()))
    want = scene.want()
    bad = [(scene.entries[i], got[i].tolist(), want[i].tolist()) for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad[:10]
    return got


def test_both_slots_in_one_launch(scene):
    """`a` and `m` candidates in one batch (a heavy one: more than six per group): one launch, a slot column each."""
    assert sum(e[2] == "a" for e in scene.entries) > 6 and sum(e[2] == "m" for e in scene.entries) > 6
    _score(scene)


def test_per_contig_counters(scene):
    got = scene.eng.score_per_contig(scene.cands())
    want = scene.want_per_contig()
    total = 0
    for k, (names, table) in enumerate(got):
        assert table.tolist() == [list(want[k][n]) for n in names], scene.entries[k]
        total += int(table.sum())
    assert total > 0


def test_eight_plane_path_gives_the_same_tables(scene, monkeypatch):
    """NM_SCORE_CLASSES=0 (read at every call) sends the same batch down the 8-plane path."""
    new = _score(scene)
    monkeypatch.setenv("NM_SCORE_CLASSES", "0")
    old = _score(scene)
    monkeypatch.delenv("NM_SCORE_CLASSES")
    again = _score(scene)
    assert np.array_equal(old, new) and np.array_equal(again, new)
