"""A walk of the class kernels starts from a fused head: the first two literal constraints of a candidate (walk order:
lowest program dword, then lowest bit) leave their words and become ONE operation on the canonical plane, dispatched on a
dense id — 36 pairs of literal words, 8 single literals, none — with the literal words skipped altogether when nothing is
left in them.  Bit for bit against the oracle on the contigs of test_gpu_canonical_tile.py (chunks on both tile bodies),
`a` and `m` candidates in one heavy launch: every pair of (side of the modified base, letter) including one word twice,
shifts of 1 and 31 and adjacent bits, every single head, candidates without a literal, two literals alone and with classes
behind them, three and four literals (the remainder stays in words), a pair with four classes; the per-contig twin; and
the same tables with NM_SCORE_HEAD=0 (no head, every literal in its word) and NM_SCORE_CLASSES=0 (the 8-plane path)."""
import numpy as np
import pytest

from test_gpu_canonical_tile import CANONICAL, CHUNK, Scene, _entry, _plant

gpu = pytest.mark.gpu                                                 # every test but the first, which needs the oracle only

LETTERS = "ACGT"
PLANE = {"A": 0, "C": 1, "G": 2, "T": 3}
SWAP = {"A": "C", "C": "A", "G": "T", "T": "G"}                       # what the tile of a C slot makes of a letter
N_PAIRS, SINGLE, NONE, N_HEADS = 36, 36, 44, 45
ADJACENT = {-1: ((-31, -30), (-2, -1)), 1: ((1, 2), (30, 31))}        # two offsets on one side: neighbouring bits of a word
ACROSS = ((-1, 1), (-31, 31), (-1, 31), (-31, 1))                     # one on either side: the far and the near shifts
CLASS_TAILS = ([(-17, "[GT]")], [(-17, "[ACG]"), (16, "[AT]")])
FOUR_CLASSES = [(-29, "[GT]"), (-17, "[AT]"), (16, "[ACG]"), (29, "[CT]")]
NO_LITERAL = ([(-1, "[GT]")], [(31, "[ACG]")], [(-31, "[AT]"), (1, "[ACG]")], [(-2, "[CT]"), (2, "[AG]"), (31, "[CGT]")])
MORE_LITERALS = ([(-31, "A"), (-1, "C"), (1, "G")],                   # three: one left in a word
                 [(1, "T"), (2, "T"), (3, "T")],                      # three bits of ONE word
                 [(-31, "G"), (-30, "G"), (30, "C"), (31, "A")],      # four: two left
                 [(-1, "A"), (1, "C"), (2, "G"), (31, "T")],
                 [(-2, "C"), (-1, "C"), (1, "C"), (17, "[AG]")],      # a remainder and a class
                 [(-1, "T"), (1, "A"), (2, "C"), (-17, "[CGT]"), (16, "[CG]")])


def head_of(mt, others):
    """(head id, a literal is left in a word) as the compiler forms them: literal word w = 4 g + plane of the letter the
    slot's tile shows, g = 0 left of the modified base and 1 right of it, bit r = offset mod 32; the first two in (w, r) order."""
    lits = sorted((4 * (d > 0) + PLANE[SWAP[s] if CANONICAL[mt] == "C" else s], d & 31) for d, s in others if s in PLANE)
    w = [x[0] for x in lits[:2]]
    if not w:
        return NONE, False
    if len(w) == 1:
        return SINGLE + w[0], False
    return w[0] * 8 - w[0] * (w[0] - 1) // 2 + (w[1] - w[0]), len(lits) > 2


def _pairs():
    """All 36 unordered pairs of (side, letter), offsets dealt out in turn: [(d1, l1), (d2, l2)]."""
    ends = [(side, l) for side in (-1, 1) for l in LETTERS]
    out, n_adj, n_across = [], {-1: 0, 1: 0}, 0
    for i, (s1, l1) in enumerate(ends):
        for s2, l2 in ends[i:]:
            if s1 == s2:
                d1, d2 = ADJACENT[s1][n_adj[s1] % 2]
                n_adj[s1] += 1
            else:
                d1, d2 = ACROSS[n_across % 4]
                n_across += 1
            out.append([(d1, l1), (d2, l2)])
    return out


def _zoo():
    zoo = []
    for mt in ("a", "m"):
        pairs = _pairs()
        singles = sorted({c for p in pairs for c in p})
        for group in ([[c] for c in singles], pairs, [p + t for p in pairs[::5] for t in CLASS_TAILS],
                      [[c] + CLASS_TAILS[1] for c in singles[::7]], NO_LITERAL, MORE_LITERALS,
                      [[(-1, "G"), (1, "A")] + FOUR_CLASSES]):
            zoo += [(_entry(mt, list(o)), list(o)) for o in group]
    return zoo


class HeadScene(Scene):
    """The contigs and pileups of test_gpu_canonical_tile.py's scene, built on the CPU; `eng` stays None until `heads` uploads them."""

    def __init__(self):
        from oracle.scan import ContigPileup
        rng = np.random.default_rng(16)
        lengths = {"long": 3 * CHUNK + 100, "short": 1000, "exact": CHUNK}
        self.names = list(lengths)
        raw = {n: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=lengths[n])].copy() for n in self.names}
        for name, phase in (("long", 0), ("exact", 1)):
            hi = 3 * CHUNK if name == "long" else CHUNK
            for anchor, letter in ((3, "N"), (12, "R"), (21, "W"), (hi - 4, "N"), (hi - 13, "R"), (hi - 22, "W")):
                _plant(raw[name], anchor, letter, phase)               # first word of the first chunk, last word of a full one
        _plant(raw["long"], 127, "W", 0)                               # either side of the lane border 127 | 128
        _plant(raw["exact"], 128, "R", 1)
        _plant(raw["short"], 127, "N", 0)
        _plant(raw["short"], 128, "N", 1)
        raw["short"][127] = ord("N")
        self.seqs = {n: raw[n].tobytes().decode() for n in self.names}
        assert set(self.seqs["long"][CHUNK - 96:2 * CHUNK + 96]) <= set("ACGT")     # chunk 1 stays on the all-valid body
        self.piles, self.rows = {"a": {}, "m": {}}, {}
        for mt, pair in (("a", "AT"), ("m", "CG")):
            cid, pos, strand, frac = [], [], [], []
            for i, name in enumerate(self.names):
                at = np.flatnonzero((raw[name] == ord(pair[0])) | (raw[name] == ord(pair[1])))
                p = np.repeat(at, 2)                                   # a row on either strand of every such position
                s = np.tile(np.frombuffer(b"+-", dtype=np.uint8), len(at))
                f = (np.arange(len(p)) // 2 + np.arange(len(p))) % 2 * 1.0
                cid.append(np.full(len(p), i, np.uint32)); pos.append(p); strand.append(s); frac.append(f)
                self.piles[mt][name] = ContigPileup(p.astype(np.int64), s, f.astype(np.float64))
            self.rows[mt] = tuple(np.concatenate(x) for x in (cid, pos, strand, frac))
        self.eng = None
        self.zoo = _zoo()
        self.entries = [e for e, _ in self.zoo]
        self._want = self._want_pc = None


@pytest.fixture(scope="module")
def inputs():
    return HeadScene()


@pytest.fixture(scope="module")
def heads(inputs):
    from nanomotif_amd.engine import ScanEngine
    inputs.eng = ScanEngine(0)
    inputs.eng.upload_assembly(inputs.names, [inputs.seqs[n] for n in inputs.names], ["bin0"] * len(inputs.names))
    for mt in ("a", "m"):
        inputs.eng.upload_pileup(mt, *inputs.rows[mt])
    yield inputs
    inputs.eng.close()
    inputs.eng = None


def test_zoo_has_every_head_and_would_notice_a_dropped_constraint(inputs):
    """On the CPU: every head id occurs for either mod type, with and without literals left behind it, and a head that
    dropped one of its two constraints would change a count (a pair has fewer sites than either of its single parents)."""
    heads = inputs
    want = heads.want()
    assert (want.sum(axis=1) > 0).all(), [heads.entries[i] for i in np.flatnonzero(want.sum(axis=1) == 0)]
    row = {(e[2], tuple(sorted(o))): i for i, (e, o) in enumerate(heads.zoo)}
    for mt in ("a", "m"):
        mine = [(e, o) for e, o in heads.zoo if e[2] == mt]
        ids = {head_of(mt, o)[0] for _, o in mine}
        assert ids == set(range(N_HEADS)), sorted(set(range(N_HEADS)) - ids)
        alone = {head_of(mt, o)[0] for _, o in mine if len(o) == 2 and head_of(mt, o)[0] < N_PAIRS}
        assert alone == set(range(N_PAIRS))                                         # two literals and nothing else
        assert {head_of(mt, o)[0] for _, o in mine if len(o) == 1} >= set(range(SINGLE, NONE))
        assert any(head_of(mt, o) == (NONE, False) and len(o) > 1 for _, o in mine)
        assert sum(head_of(mt, o)[1] for _, o in mine) >= 4                         # the remainder stays in words
        assert any(h < N_PAIRS and not left and len(o) > 2 for _, o in mine for h, left in [head_of(mt, o)])
        shifts = {d for _, o in mine if len(o) == 2 and head_of(mt, o)[0] < N_PAIRS for d, _ in o}
        assert shifts >= {-31, -1, 1, 31}
        for e, o in mine:
            if len(o) == 2 and head_of(mt, o)[0] < N_PAIRS:
                both = want[row[mt, tuple(sorted(o))]].sum()
                for c in o:
                    assert both < want[row[mt, (c,)]].sum(), (e, c)


def _score(heads):
    got = np.asarray(heads.eng.score(heads.cands()))
    want = heads.want()
    bad = [(heads.entries[i], got[i].tolist(), want[i].tolist()) for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad[:10]
    return got


@gpu
def test_every_head_against_the_oracle(heads):
    """`a` and `m` candidates in one heavy batch (more than six per group): one launch, a slot column each."""
    assert sum(e[2] == "a" for e in heads.entries) > 6 and sum(e[2] == "m" for e in heads.entries) > 6
    _score(heads)


@gpu
def test_per_contig_twin(heads):
    got = heads.eng.score_per_contig(heads.cands())
    want = heads.want_per_contig()
    total = 0
    for k, (names, table) in enumerate(got):
        assert table.tolist() == [list(want[k][n]) for n in names], heads.entries[k]
        total += int(table.sum())
    assert total > 0


@gpu
def test_switches_give_the_same_tables(heads, monkeypatch):
    """NM_SCORE_HEAD=0 (no head: plain moves, every literal walked from its word) and NM_SCORE_CLASSES=0 (the 8-plane path),
    both read at every call."""
    new = _score(heads)
    monkeypatch.setenv("NM_SCORE_HEAD", "0")
    no_head = _score(heads)
    monkeypatch.delenv("NM_SCORE_HEAD")
    monkeypatch.setenv("NM_SCORE_CLASSES", "0")
    eight = _score(heads)
    monkeypatch.delenv("NM_SCORE_CLASSES")
    again = _score(heads)
    assert np.array_equal(no_head, new) and np.array_equal(eight, new) and np.array_equal(again, new)
