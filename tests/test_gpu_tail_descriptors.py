"""What a walk of the class kernels finds behind its head is mostly small.  Exactly one class constraint is flagged in the
summary dword of the program, its word the lowest set bit and its shift beside the flag, and reaches its leaf through a 20-way
switch past the quads; two or more classes stay behind the quads.  Left-over literals stay in their words whatever their number:
descriptors for one or two of them were built and measured in the same round and did not pay (profiles/r25/
tail_descriptors.md); their candidates stay here, since the class leaf runs behind them.  Bit for bit against the oracle on the
contigs of test_gpu_canonical_tile.py (chunks on both tile bodies), `a` and `m` candidates in one heavy launch:
  literals   every literal word as the lone left-over behind a pair head — in the head's own word (right above the head's
             bit and far above it; walk order is (word, bit), so a left-over never lies below a head literal of its word),
             behind a head in other words, behind a head that shares only its second literal's word — at shifts 1 and 31;
             two left-overs in one word (adjacent bits) for every word, and in two words on either side of the modified base;
             three left-overs in three words and in one
  classes    every class word (the 2-sets and 3-sets, either side: 20) at shifts 1 and 31 as the only constraint, and
             behind a single head, behind a pair, with one and with two left-over literals; two class constraints in one
             word, in one quad and in two quads (the quads again)
the per-contig twin, and the same tables with NM_SCORE_TAIL = 0 / 1 / 2 (no descriptor / the literal kind, which is not built:
none either / the class one), each also with NM_SCORE_HEAD=0, and with NM_SCORE_CLASSES=0."""
import numpy as np
import pytest

from test_gpu_canonical_tile import CANONICAL, CHUNK, NEGATIVE, _entry, _forward_sites
from test_gpu_head_pair import LETTERS, PLANE, SWAP, HeadScene, _score

gpu = pytest.mark.gpu                                                 # every test but the first, which needs the oracle only

N_LIT_WORDS, N_CLASS_WORDS = 8, 20
TILE_SETS = ["CGT", "AGT", "ACT", "ACG", "GT", "AC", "CG", "AT", "CT", "AG"]     # class words 4..13 as a tile shows them
CLASS_WORD = {s: 4 + i for i, s in enumerate(TILE_SETS)}
HEAD_BITS = (5, 6)                                                    # the head's two literals, where they only have to be there
SHIFTS = (1, 31)


def _offset(g, r):
    """Word-group 0 is left of the modified base: bit r of it is offset r - 32; word-group 1: offset r."""
    return r - 32 if g == 0 else r


def lit(mt, w, r):
    """(offset, letter) of the literal constraint that the compiler puts at bit r of literal word w of an `mt` candidate."""
    tile = LETTERS[w % 4]
    return _offset(w // 4, r), SWAP[tile] if CANONICAL[mt] == "C" else tile


def cls(mt, c, r):
    """(offset, set) of the class constraint at bit r of class word c (0..19, counted from program dword 9)."""
    tile = TILE_SETS[c % 10]
    letters = sorted(SWAP[x] for x in tile) if CANONICAL[mt] == "C" else sorted(tile)
    return _offset(c // 10, r), "[" + "".join(letters) + "]"


def tail_of(mt, others, use_head=True, tail=3):
    """What the compiler must write behind the head: (literals left in the words: their number, [(w, r) of each], class state,
    (c, r) or None).  Class state: 'none', 'one' (the flag) or 'quads'.  tail: bit 1 asks for the class descriptor (NM_SCORE_TAIL;
    3 when unset; bit 0 asked for literal descriptors, which are not built)."""
    swap = CANONICAL[mt] == "C"
    lits = sorted((4 * (d > 0) + PLANE[SWAP[s] if swap else s], d & 31) for d, s in others if s in PLANE)
    left = lits[2:] if use_head else lits
    state, desc = len(left), left
    classes = []
    for d, s in others:
        if s not in PLANE:
            letters = s.strip("[]")
            tile = "".join(sorted(SWAP[x] for x in letters) if swap else sorted(letters))
            classes.append((10 * (d > 0) + CLASS_WORD[tile] - 4, d & 31))
    if not classes:
        return state, desc, "none", None
    if len(classes) == 1 and tail & 2:
        return state, desc, "one", classes[0]
    return state, desc, "quads", None


def _zoo():
    """[(entry, others, kind, index in others of the constraint under test)]"""
    zoo = []

    def add(mt, kind, others, probe):
        assert len({d for d, _ in others}) == len(others), (kind, others)           # one constraint an offset
        zoo.append((_entry(mt, list(others)), list(others), kind, probe))

    for mt in ("a", "m"):
        head = [lit(mt, 0, HEAD_BITS[0]), lit(mt, 0, HEAD_BITS[1])]
        for w in range(N_LIT_WORDS):
            # in the head's own word: right above the head's second bit, and far above
            add(mt, "lone:own-word", [lit(mt, w, 1), lit(mt, w, 2), lit(mt, w, 3)], 2)
            add(mt, "lone:own-word", [lit(mt, w, 1), lit(mt, w, 2), lit(mt, w, 31)], 2)
            if w:
                for r in SHIFTS:                                                    # the head in another word
                    add(mt, "lone:other-word", head + [lit(mt, w, r)], 2)
                add(mt, "lone:shared-second", [head[0], lit(mt, w, 8), lit(mt, w, 9)], 2)
            # two left-overs in one word, adjacent bits
            add(mt, "two:one-word", head + [lit(mt, w, 10), lit(mt, w, 11)], 3)
        for wa, wb in ((1, 6), (3, 4), (2, 7), (0, 5)):                             # two words, either side of the modified base
            add(mt, "two:two-words", head + [lit(mt, wa, 9), lit(mt, wb, 9)], 3)
            add(mt, "two:two-words", head + [lit(mt, wa, 1 if wa else 9), lit(mt, wb, 31)], 2)
        add(mt, "three", head + [lit(mt, 1, 7), lit(mt, 2, 8), lit(mt, 5, 9)], 3)
        add(mt, "three", head + [lit(mt, 6, 7), lit(mt, 6, 8), lit(mt, 6, 9)], 4)
        add(mt, "three", [lit(mt, 3, 1), lit(mt, 3, 2), lit(mt, 3, 3), lit(mt, 3, 30), lit(mt, 3, 31)], 4)
        for c in range(N_CLASS_WORDS):
            for r in SHIFTS:
                add(mt, "class:alone", [cls(mt, c, r)], 0)
            r = (1, 31, 16)[c % 3]
            w1, w2, w3 = c % 8, (c + 3) % 8, (c + 5) % 8
            add(mt, "class:single", [lit(mt, w1, 5), cls(mt, c, r)], 1)
            add(mt, "class:pair", [lit(mt, w1, 5), lit(mt, w2, 6), cls(mt, c, r)], 2)
            add(mt, "class:one-left", [lit(mt, w1, 5), lit(mt, w2, 6), lit(mt, w3, 7), cls(mt, c, r)], 3)
            add(mt, "class:two-left", [lit(mt, w1, 5), lit(mt, w2, 6), lit(mt, w3, 7), lit(mt, w1, 8), cls(mt, c, r)], 4)
        for c in (0, 4, 8, 13, 19):                                                 # two class constraints: the quads again
            add(mt, "classes:one-word", [cls(mt, c, 1), cls(mt, c, 31)], 1)
        for c, c2 in ((0, 3), (5, 6), (9, 10), (12, 15), (17, 19)):
            assert c // 4 == c2 // 4
            add(mt, "classes:one-quad", [cls(mt, c, 2), cls(mt, c2, 30)], 1)
        for c, c2 in ((0, 19), (3, 4), (7, 8), (2, 13), (11, 16)):
            assert c // 4 != c2 // 4
            add(mt, "classes:two-quads", [lit(mt, 2, 5), cls(mt, c, 3), cls(mt, c2, 29)], 2)
    return zoo


class TailScene(HeadScene):
    """The contigs and pileups of test_gpu_head_pair.py's scene with this file's candidates."""

    def __init__(self):
        super().__init__()
        full = _zoo()
        self.zoo = [(e, o) for e, o, _, _ in full]
        self.kinds = [k for _, _, k, _ in full]
        self.probes = [p for _, _, _, p in full]
        self.entries = [e for e, _ in self.zoo]
        self._want = self._want_pc = None


@pytest.fixture(scope="module")
def inputs():
    return TailScene()


@pytest.fixture(scope="module")
def tails(inputs):
    from nanomotif_amd.engine import ScanEngine
    inputs.eng = ScanEngine(0)
    inputs.eng.upload_assembly(inputs.names, [inputs.seqs[n] for n in inputs.names], ["bin0"] * len(inputs.names))
    for mt in ("a", "m"):
        inputs.eng.upload_pileup(mt, *inputs.rows[mt])
    yield inputs
    inputs.eng.close()
    inputs.eng = None


def test_zoo_reaches_every_leaf_and_would_notice_one_that_does_nothing(inputs):
    """On the CPU, by count: every class word through the flag in every company (alone, behind a single head and a pair, with
    one and two literals left in every literal word), every fallback; and the oracle's counts change when the constraint under
    test is dropped."""
    from oracle.scan import score_candidates
    z = inputs
    want = z.want()
    assert (want.sum(axis=1) > 0).all(), [z.entries[i] for i in np.flatnonzero(want.sum(axis=1) == 0)]
    every_lit, every_cls = set(range(N_LIT_WORDS)), set(range(N_CLASS_WORDS))
    for mt in ("a", "m"):
        mine = [(o, k, tail_of(mt, o)) for (e, o), k in zip(z.zoo, z.kinds) if e[2] == mt]
        for kind in ("lone:own-word", "lone:other-word", "lone:shared-second"):
            words = {t[1][0][0] for o, k, t in mine if k == kind}
            assert words == every_lit - ({0} if kind != "lone:own-word" else set()), (kind, words)
            assert all(t[0] == 1 for o, k, t in mine if k == kind)
        assert {t[1][0][1] for o, k, t in mine if t[0] == 1} >= {1, 31}                        # the left-over's shifts
        two = [t for o, k, t in mine if t[0] == 2]
        assert {t[1][0][0] for t in two} == every_lit and {t[1][1][0] for t in two} == every_lit
        assert all(t[0] == 2 for o, k, t in mine if k.startswith("two:"))
        assert any(t[1][0][0] == t[1][1][0] and t[1][0][1] + 1 == t[1][1][1] for t in two)       # one word, adjacent bits
        assert any(t[1][0][0] < 4 <= t[1][1][0] for t in two)                                    # either side
        assert {t[1][k][1] for t in two for k in (0, 1)} >= {1, 31}
        assert sum(t[0] >= 3 for o, k, t in mine) >= 3 and all(t[0] == 3 for o, k, t in mine if k == "three")
        for kind, lit_state in (("class:alone", 0), ("class:single", 0), ("class:pair", 0), ("class:one-left", 1), ("class:two-left", 2)):
            got = [t for o, k, t in mine if k == kind]
            assert all(t[0] == lit_state and t[2] == "one" for t in got), kind
            assert {t[3][0] for t in got} == every_cls, kind
        alone = {t[3] for o, k, t in mine if k == "class:alone"}
        assert alone == {(c, r) for c in every_cls for r in SHIFTS}                              # every sense at shifts 1 and 31
        for kind in ("classes:one-word", "classes:one-quad", "classes:two-quads"):
            assert sum(k == kind for o, k, t in mine) >= 3 and all(t[2] == "quads" for o, k, t in mine if k == kind), kind
        # the switch settings, restated: no flag where the class descriptor is off; without a head every literal is a left-over
        assert all(tail_of(mt, o, tail=0)[2] != "one" and tail_of(mt, o, tail=1)[2] != "one" and tail_of(mt, o, tail=2)[2] == t[2]
                   for o, k, t in mine)
        assert {tail_of(mt, o, use_head=False)[0] for o, k, t in mine if t[2] == "one"} >= {0, 1, 2, 3, 4}
    # the constraint under test dropped: other counts (dropping it can only add sites)
    for mt in ("a", "m"):
        idx = [i for i, e in enumerate(z.entries) if e[2] == mt]
        less = [_entry(mt, [c for k, c in enumerate(z.zoo[i][1]) if k != z.probes[i]])[:2] for i in idx]
        loose = score_candidates(z.piles[mt], z.seqs, less)
        same = [z.entries[i] for i, row in zip(idx, loose) if np.array_equal(row, want[i])]
        assert not same, same
        assert all((row >= want[i]).all() for i, row in zip(idx, loose))
    # the negative senses, and X: matches in a boundary chunk and in an interior one, and invalid letters where a leaf that
    # forgot V would count them (`m`: the scene plants them around C and G sites at these offsets)
    long_ = z.seqs["long"]
    for (e, o), kind in zip(z.zoo, z.kinds):
        if kind != "class:alone":
            continue
        mt = e[2]
        assert _forward_sites(long_[CHUNK:2 * CHUNK], mt, o, False) > 0, e                     # chunk 1: the all-valid body
        assert _forward_sites(z.seqs["exact"], mt, o, False) + _forward_sites(z.seqs["short"], mt, o, False) > 0, e
        if mt == "m" and o[0][1] in NEGATIVE:
            assert sum(_forward_sites(s, mt, o, True) - _forward_sites(s, mt, o, False) for s in z.seqs.values()) > 0, e


@gpu
def test_every_tail_against_the_oracle(tails):
    """`a` and `m` candidates in one heavy batch (more than six per group): one launch, a slot column each."""
    assert sum(e[2] == "a" for e in tails.entries) > 6 and sum(e[2] == "m" for e in tails.entries) > 6
    _score(tails)


@gpu
def test_per_contig_twin(tails):
    got = tails.eng.score_per_contig(tails.cands())
    want = tails.want_per_contig()
    total = 0
    for k, (names, table) in enumerate(got):
        assert table.tolist() == [list(want[k][n]) for n in names], tails.entries[k]
        total += int(table.sum())
    assert total > 0


@gpu
@pytest.mark.parametrize("tail", ["0", "1", "2"])
def test_switches_give_the_same_tables(tails, monkeypatch, tail):
    """NM_SCORE_TAIL (whether the compiler writes the class descriptor), alone and with NM_SCORE_HEAD=0; all read at every call."""
    new = _score(tails)
    monkeypatch.setenv("NM_SCORE_TAIL", tail)
    switched = _score(tails)
    monkeypatch.setenv("NM_SCORE_HEAD", "0")
    no_head = _score(tails)
    monkeypatch.delenv("NM_SCORE_TAIL")
    monkeypatch.delenv("NM_SCORE_HEAD")
    again = _score(tails)
    assert np.array_equal(switched, new) and np.array_equal(no_head, new) and np.array_equal(again, new)


@gpu
def test_no_head_and_eight_plane_path_give_the_same_tables(tails, monkeypatch):
    """The descriptor without a head (NM_SCORE_HEAD=0), and the 8-plane path (NM_SCORE_CLASSES=0)."""
    new = _score(tails)
    monkeypatch.setenv("NM_SCORE_HEAD", "0")
    no_head = _score(tails)
    monkeypatch.delenv("NM_SCORE_HEAD")
    monkeypatch.setenv("NM_SCORE_CLASSES", "0")
    eight = _score(tails)
    monkeypatch.delenv("NM_SCORE_CLASSES")
    assert np.array_equal(no_head, new) and np.array_equal(eight, new)
