"""The order in which a walk of the class kernels looks at its program, and the order in which a pass fetches the programs of
its candidates: whichever way the 28 word tests are laid out (skip by branch or by falling through), whichever half of the
32 dwords a word lies in, and whether a program is fetched at the top of its walk or a walk ahead, the counts are the
oracle's, bit for bit.  On the contigs of test_gpu_canonical_tile.py (chunks on both tile bodies) plus four small bins, `a`
and `m` candidates in one heavy launch and in the per-contig twin:
  * a constraint in each of the 20 class words, one word per candidate, at shifts 1 and 31;
  * classes in the first four class words only (the ones that share a 16-dword half with the literals), in the other sixteen
    only, and in both;
  * two and three bits in one word, class and literal (a word's loop goes round more than once);
  * all eight literal words non-empty behind a pair head (planted: the motif has ten literals), and every parent of it
    that lacks one of the ten, so that a skipped word changes a count;
  * nothing after the head; no literal at all;
  * (bin, slot) groups of 1, 2, 32 and 33 candidates (a pass of one candidate, a full pass, a second pass with a shifted
    first program), each ending in a candidate with classes in the last sixteen class words - so does the group that holds
    the last program of the table;
  * the same tables under NM_SCORE_HEAD=0 and NM_SCORE_CLASSES=0."""
import numpy as np
import pytest

from test_gpu_canonical_tile import CANONICAL, CHUNK, Scene, _entry, _plant

gpu = pytest.mark.gpu                                                 # every test but the first, which needs the oracle only

PLANE = {"A": 0, "C": 1, "G": 2, "T": 3}
SWAP = {"A": "C", "C": "A", "G": "T", "T": "G"}                       # what the tile of a C slot makes of a letter
# class word 4..13 of a set (csrc/nmscan_device.h: A- C- G- T-, H+ H-, L+ L-, X+ X- on the code A=00 C=01 G=11 T=10)
CLASS_WORD = {"CGT": 4, "AGT": 5, "ACT": 6, "ACG": 7, "GT": 8, "AC": 9, "CG": 10, "AT": 11, "CT": 12, "AG": 13}
CLASS_SETS = ["[" + s + "]" for s in CLASS_WORD]
EDGE = (-31, -1, 1, 31)                                               # shifts 1, 31 left of the modified base and 1, 31 right of it
SECOND_HALF = [(-2, "[GT]")]                                        # class word 4 of 20: not among the first four
# ten literals: three in literal word 0 (two of them become the head), one in each of the other seven
EIGHT = {"a": [(-8, "A"), (-7, "A"), (-6, "A"), (-5, "C"), (-4, "G"), (-3, "T"), (1, "A"), (2, "C"), (3, "G"), (4, "T")],
         "m": [(-8, "C"), (-7, "C"), (-6, "C"), (-5, "A"), (-4, "G"), (-3, "T"), (1, "A"), (2, "C"), (3, "G"), (4, "T")]}
GROUPS = {"grp01": 1, "grp02": 2, "grp32": 32, "grp33": 33}           # bin -> candidates per mod type (bin ids follow the sorted names)
SMALL_CONTIGS = {"grp01": ("one", 1500), "grp02": ("two", CHUNK + 300), "grp32": ("full", 2 * CHUNK + 77), "grp33": ("over", 1000)}


def words_of(mt, others):
    """(literal words, class words) of a candidate as its program holds them before the head is taken: {word: [bits]}; literal
    word 4 g + plane, class word 10 g + (p - 4), g = 0 left of the modified base and 1 right of it, bit = offset mod 32."""
    lit, cls = {}, {}
    for d, s in others:
        letters = s.strip("[]")
        if CANONICAL[mt] == "C":
            letters = "".join(sorted(SWAP[c] for c in letters))
        if len(letters) == 1:
            lit.setdefault(4 * (d > 0) + PLANE[letters], []).append(d & 31)
        else:
            cls.setdefault(10 * (d > 0) + CLASS_WORD[letters] - 4, []).append(d & 31)
    return lit, cls


def left_after_head(mt, others):
    """The literal words once the first two literals in (word, bit) order have left them."""
    lit, _ = words_of(mt, others)
    flat = sorted((w, r) for w, bits in lit.items() for r in bits)[2:]
    out = {}
    for w, r in flat:
        out.setdefault(w, []).append(r)
    return out


def _bin0_zoo(mt):
    pair = [(-1, "G"), (1, "T")]
    zoo = [[(d, s)] for s in CLASS_SETS for d in EDGE]                                  # one class word each, no literal
    first4 = ([(-5, "[CGT]")], [(-9, "[ACG]"), (-17, "[AGT]")])
    rest = ([(5, "[GT]"), (-7, "[AT]")], [(9, "[ACT]")])
    both = ([(-5, "[CGT]"), (7, "[ACT]"), (-11, "[CT]")],)
    for group in (first4, rest, both):
        zoo += [list(o) for o in group] + [pair + list(o) for o in group[:1]]
    zoo += [[(1, "[GT]"), (2, "[GT]")], [(-3, "[AT]"), (-2, "[AT]"), (-1, "[AT]")], [(-31, "[CGT]"), (-16, "[CGT]"), (-1, "[CGT]")],
            [(-31, "A"), (-30, "A"), (1, "T"), (2, "T")], [(-2, "G"), (-1, "G"), (1, "T"), (2, "T"), (3, "T")]]
    zoo += [EIGHT[mt]] + [EIGHT[mt][:i] + EIGHT[mt][i + 1:] for i in range(len(EIGHT[mt]))]
    zoo += [pair, [(31, "C")]]                                                          # nothing after the head
    zoo += [pair + SECOND_HALF]                                                         # the group ends in the last sixteen
    return zoo


class OrderScene(Scene):
    """The contigs of test_gpu_canonical_tile.py's scene in bin0 and one contig in each bin of GROUPS, built on the CPU; `eng` stays
    None until the `order` fixture uploads them."""

    def __init__(self):
        from oracle.scan import ContigPileup
        rng = np.random.default_rng(18)
        lengths = {"long": 3 * CHUNK + 100, "short": 1000, "exact": CHUNK}
        lengths.update({name: n for name, n in SMALL_CONTIGS.values()})
        self.names = list(lengths)
        self.bin_of = {"long": "bin0", "short": "bin0", "exact": "bin0"}
        self.bin_of.update({name: b for b, (name, _) in SMALL_CONTIGS.items()})
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
        # the ten-literal motif and each of its parents: whole in every kind of chunk, and once with each literal spoiled
        self.n_planted = {}
        for mt, shift in (("a", 0), ("m", 2000)):
            whole = [("long", 600), ("long", CHUNK + 500), ("long", 2 * CHUNK + 1000), ("exact", 4000)]
            whole = [(n, at + shift) for n, at in whole] + [("long", 3 * CHUNK + (50 if mt == "a" else 80)), ("short", 500 if mt == "a" else 800)]
            for name, at in whole:
                self._write(raw[name], at, mt, None)
            for i in range(len(EIGHT[mt])):
                self._write(raw["long"], CHUNK + 1000 + shift + 40 * i, mt, i)
            self.n_planted[mt] = len(whole)
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
        # (entry, offsets and sets, bin): bin0 takes the zoo, the small bins deal it out again and end in the last sixteen words
        self.zoo, self.bins = [], []
        for mt in ("a", "m"):
            mine = _bin0_zoo(mt)
            for o in mine:
                self.zoo.append((_entry(mt, o), o)); self.bins.append("bin0")
            at = 0
            for b, n in GROUPS.items():
                for k in range(n):
                    o = SECOND_HALF if k == n - 1 else mine[(7 * at + 3) % len(mine)]
                    at += 1
                    self.zoo.append((_entry(mt, o), o)); self.bins.append(b)
        self.entries = [e for e, _ in self.zoo]
        self._want = self._want_pc = None

    @staticmethod
    def _write(seq, at, mt, spoiled):
        """EIGHT[mt] around `at`; spoiled: the index of the one literal that gets another letter."""
        seq[at] = ord(CANONICAL[mt])
        for i, (d, s) in enumerate(EIGHT[mt]):
            seq[at + d] = ord(s if i != spoiled else "ACGT"[(PLANE[s] + 2) % 4])

    def contigs_of(self, b):
        return [n for n in self.names if self.bin_of[n] == b]

    def want(self):
        from oracle.scan import score_candidates
        if self._want is None:
            out = np.zeros((len(self.entries), 2), dtype=np.int64)
            for mt in ("a", "m"):
                for b in ["bin0"] + list(GROUPS):
                    idx = [i for i, e in enumerate(self.entries) if e[2] == mt and self.bins[i] == b]
                    names = self.contigs_of(b)
                    out[idx] = score_candidates({n: self.piles[mt][n] for n in names}, {n: self.seqs[n] for n in names},
                                                [self.entries[i][:2] for i in idx])
            self._want = out
        return self._want

    def want_per_contig(self):
        from oracle.contig_methylation import per_contig_counts
        if self._want_pc is None:
            self._want_pc = []
            for (s, p, mt), b in zip(self.entries, self.bins):
                names = self.contigs_of(b)
                self._want_pc.append(per_contig_counts({n: self.piles[mt][n] for n in names}, {n: self.seqs[n] for n in names}, s, p))
        return self._want_pc

    def cands(self):
        from nanomotif_amd.motif import Motif
        return [(Motif(s, p), mt, b) for (s, p, mt), b in zip(self.entries, self.bins)]


@pytest.fixture(scope="module")
def inputs():
    return OrderScene()


@pytest.fixture(scope="module")
def order(inputs):
    from nanomotif_amd.engine import ScanEngine
    inputs.eng = ScanEngine(0)
    inputs.eng.upload_assembly(inputs.names, [inputs.seqs[n] for n in inputs.names], [inputs.bin_of[n] for n in inputs.names])
    for mt in ("a", "m"):
        inputs.eng.upload_pileup(mt, *inputs.rows[mt])
    yield inputs
    inputs.eng.close()
    inputs.eng = None


def test_zoo_holds_what_the_walk_order_can_get_wrong(inputs):
    """On the CPU: the cases of the module docstring are there for either mod type, and a skipped word would change a count."""
    want = inputs.want()
    groups = {}
    for i, ((_, _, mt), b) in enumerate(zip(inputs.entries, inputs.bins)):
        groups.setdefault((mt, b), []).append(i)
    # every candidate has sites where the whole zoo is, in bin0 (the ten-literal motif is planted there only); every group has some
    assert all(want[i].sum() > 0 for (_, b), idx in groups.items() if b == "bin0" for i in idx)
    assert all(want[idx].sum() > 0 for idx in groups.values())
    assert len(inputs.entries) > 6 * len(groups)                                        # a heavy launch
    assert sorted(inputs.bin_of.values())[-1] == "grp33" and sorted(set(inputs.bin_of.values()))[0] == "bin0"
    for mt in ("a", "m"):
        mine = [o for (e, o), b in zip(inputs.zoo, inputs.bins) if e[2] == mt and b == "bin0"]
        alone = {(w, r) for o in mine if len(o) == 1 for w, bits in words_of(mt, o)[1].items() for r in bits}
        assert alone >= {(w, r) for w in range(20) for r in (1, 31)}                  # every class word, both shifts
        quads = [{w // 4 for w in words_of(mt, o)[1]} for o in mine]
        assert any(q == {0} for q in quads) and any(q and 0 not in q for q in quads) and any(0 in q and len(q) > 1 for q in quads)
        for n in (2, 3):
            assert any(len(bits) == n for o in mine for bits in words_of(mt, o)[1].values()), n
            assert any(len(bits) == n for o in mine for bits in left_after_head(mt, o).values()), n
        assert sorted(left_after_head(mt, EIGHT[mt])) == list(range(8)) and len(words_of(mt, EIGHT[mt])[0][0]) == 3
        assert any(len(o) == 2 and not words_of(mt, o)[1] and not left_after_head(mt, o) for o in mine)      # a pair and nothing else
        assert any(not words_of(mt, o)[0] for o in mine)                                                     # no literal
        assert sorted(len(groups[mt, b]) for b in GROUPS) == [1, 2, 32, 33]
        for b in ["bin0"] + list(GROUPS):
            last = inputs.zoo[groups[mt, b][-1]][1]
            assert any(w >= 4 for w in words_of(mt, last)[1]), (mt, b)                  # ends in the last sixteen class words
        row = {tuple(o): i for i, ((e, o), b) in enumerate(zip(inputs.zoo, inputs.bins)) if e[2] == mt and b == "bin0"}
        whole = want[row[tuple(EIGHT[mt])]].sum()
        assert whole >= inputs.n_planted[mt]
        for i in range(len(EIGHT[mt])):
            assert want[row[tuple(EIGHT[mt][:i] + EIGHT[mt][i + 1:])]].sum() > whole, (mt, i)


def _score(order):
    got = np.asarray(order.eng.score(order.cands()))
    want = order.want()
    bad = [(order.entries[i], order.bins[i], got[i].tolist(), want[i].tolist()) for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad[:10]
    return got


@gpu
def test_one_heavy_launch_against_the_oracle(order):
    _score(order)


@gpu
def test_per_contig_twin(order):
    got = order.eng.score_per_contig(order.cands())
    want = order.want_per_contig()
    total = 0
    for k, (names, table) in enumerate(got):
        assert sorted(names) == sorted(want[k]), (order.entries[k], order.bins[k])
        assert table.tolist() == [list(want[k][n]) for n in names], (order.entries[k], order.bins[k])
        total += int(table.sum())
    assert total > 0


@gpu
def test_switches_give_the_same_tables(order, monkeypatch):
    """NM_SCORE_HEAD=0 (id 44, every literal in its word) and NM_SCORE_CLASSES=0 (the 8-plane path), both read at every call."""
    new = _score(order)
    monkeypatch.setenv("NM_SCORE_HEAD", "0")
    no_head = _score(order)
    monkeypatch.delenv("NM_SCORE_HEAD")
    monkeypatch.setenv("NM_SCORE_CLASSES", "0")
    eight = _score(order)
    monkeypatch.delenv("NM_SCORE_CLASSES")
    again = _score(order)
    assert np.array_equal(no_head, new) and np.array_equal(eight, new) and np.array_equal(again, new)
