"""Heavy batches on the work list with packed contig tails (csrc/nmscore_worklist.h, score_kernel's load_entry): a metagenome of
0.19 Mbp whose contigs end on every border of a lane strip, scored through every heavy kernel that walks the list, every way a batch
reaches it.  Counts are compared by equality with a brute force written here — a regex over each contig string and a dict of the
uploaded calls — with the same call on the plain list (NM_SCORE_PACK_TAILS=0) and on the 8-plane kernel (NM_SCORE_CLASSES=0)."""
import os
import re

import numpy as np
import pytest

from nanomotif_amd.motif import Motif

pytestmark = pytest.mark.gpu

CANONICAL = {"a": "A", "m": "C"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
CHUNK, STRIP = 8192, 128
ANY = "ACGT "
# (sets per position, modified position); * = the canonical base of the mod type.  Padding reads as base code 00 = A with V = 0: the
# shapes that begin or end with a set holding A are the ones a walk over padding would count
LITERALS = [("G * T C", 1), ("* C G", 0), ("C C * G G", 2), ("* A", 0), ("A *", 1), ("T * A", 1), ("A A *", 2), ("* T", 0), ("*", 0)]
SETS = [("T AT * A", 2), ("AG * T", 1), ("CG * CG", 1), ("ACT * G", 1), ("G ACG * ACGT T", 2), ("* ACG", 0), ("ACG *", 1), ("* AC", 0),
        ("AG *", 1), ("AT * ACGT AG", 1), ("* ACGT ACT", 0)]
REACH_31 = [("A " + ANY * 30 + "* " + ANY * 30 + "ACG", 31), ("ACG " + ANY * 30 + "*", 31), ("* " + ANY * 30 + "AC", 0)]
MIXED = LITERALS[:6] + SETS + REACH_31
REACH_40 = [("AG " + ANY * 39 + "*", 40), ("* " + ANY * 39 + "A", 0)] + LITERALS[:6]     # a wide batch: two halo words either side


def _token(s):
    return s if len(s) == 1 else "." if len(s) == 4 else "[" + s + "]"


def motif_of(shape, mt):
    sets = [CANONICAL[mt] if t == "*" else t for t in shape[0].split()]
    return Motif("".join(_token(s) for s in sets), shape[1]), sets, shape[1]


def contig_lengths():
    """Four bins.  0: the border lengths of a chunk and a strip.  1: a hundred short contigs (their tails share a few rows; 100 chunks
    become 8 rows, across a multiple of 16 entries).  2: tails that fill one row exactly next to a long contig, and last bp on bit 0 /
    bit 31 of a strip's first and last word.  3: one contig (as many entries packed as plain)."""
    rng = np.random.default_rng(11)
    return [[1, 127, 128, 129, 8191, 8192, 8193, 16384, 16385],
            [int(x) for x in rng.integers(200, 901, size=100)],
            [CHUNK + 20 * STRIP, 44 * STRIP - 5, 4 * CHUNK + 3 * STRIP + 32, 5 * STRIP + 32, 7 * STRIP + 97, 2 * STRIP + 1, 9 * STRIP],
            [3 * CHUNK + 1000]]


class Data:
    def __init__(self, seed=3):
        rng = np.random.default_rng(seed)
        self.names, self.bins, self.seqs = [], [], []
        per_bin = contig_lengths()
        for k in range(max(len(c) for c in per_bin)):          # upload order mixes the bins
            for b, contigs in enumerate(per_bin):
                if k < len(contigs):
                    self.names.append("contig_%d_%03d" % (b, k))
                    self.bins.append("bin_%d" % b)
                    self.seqs.append(rng.choice(list("ACGT"), size=contigs[k]))
        # planted: a shape's first letters at a contig's end with the window ending on the last bp / one past it, at its start with
        # the window starting on bp 0 / one before it
        plant = [s for s in LITERALS + SETS if len(s[0].split()) > 1]
        for i, seq in enumerate(self.seqs):
            shape = plant[i % len(plant)]
            letters = [motif_of(shape, "am"[i // len(plant) % 2])[1][j][0] for j in range(len(shape[0].split()))]
            if len(seq) < 2 * len(letters) + 2:
                continue
            head, tail = (letters, letters) if i % 4 == 0 else (letters[1:], letters) if i % 4 == 1 else (letters, letters[:-1]) if i % 4 == 2 else (letters[1:], letters[:-1])
            seq[:len(head)] = head
            seq[len(seq) - len(tail):] = tail
        self.seqs = ["".join(s) for s in self.seqs]
        assert sum(len(s) for s in self.seqs) <= 300_000
        self.bin_names = sorted(set(self.bins))
        self.calls, self.columns = {}, {}
        for mt, base in CANONICAL.items():
            cid, pos, strand, frac = [], [], [], []
            for i, s in enumerate(self.seqs):
                a = np.frombuffer(s.encode(), dtype=np.uint8)
                for st, letter in (("+", base), ("-", COMPLEMENT[base])):
                    p = np.flatnonzero(a == ord(letter))
                    f = rng.choice([0.95, 0.05, 0.5], size=len(p), p=[0.45, 0.45, 0.1])
                    cid.append(np.full(len(p), i, np.uint32)); pos.append(p.astype(np.uint32)); strand.append(np.full(len(p), ord(st), np.uint8)); frac.append(f)
                    for q, v in zip(p.tolist(), f.tolist()):
                        if v != 0.5:
                            self.calls[(mt, i, q, st)] = v > 0.5
            self.columns[mt] = tuple(np.concatenate(x) for x in (cid, pos, strand, frac))
        self._brute = {}

    def engine(self, keep=None):
        """An engine with all contigs, or with the contigs whose index is in ``keep`` (the bins keep their numbers)."""
        from nanomotif_amd.engine import ScanEngine
        keep = list(range(len(self.names))) if keep is None else sorted(keep)
        new_id = np.full(len(self.names), -1, np.int64)
        new_id[keep] = np.arange(len(keep))
        eng = ScanEngine(0)
        eng.upload_assembly([self.names[i] for i in keep], [self.seqs[i] for i in keep], [self.bins[i] for i in keep], bin_names=self.bin_names)
        for mt in ("a", "m"):
            cid, pos, strand, frac = self.columns[mt]
            rows = new_id[cid] >= 0
            eng.upload_pileup(mt, new_id[cid][rows].astype(np.uint32), pos[rows], strand[rows], frac[rows])
        return eng

    def brute(self, shape, mt):
        """int64[n_contigs, 2]: (n_mod, n_nomod) of a shape on every contig — every (overlapping) regex match of the motif on the '+'
        strand and of its reverse complement on the '-' strand that lies inside the contig, looked up in the calls."""
        key = (shape, mt)
        if key not in self._brute:
            _, sets, mp = motif_of(shape, mt)
            rc = ["".join(COMPLEMENT[x] for x in s) for s in reversed(sets)]
            out = np.zeros((len(self.seqs), 2), dtype=np.int64)
            for strand, ss, at in (("+", sets, mp), ("-", rc, len(sets) - 1 - mp)):
                pattern = re.compile("(?=" + "".join("[%s]" % s for s in ss) + ")")
                for i, seq in enumerate(self.seqs):
                    for m in pattern.finditer(seq):
                        call = self.calls.get((mt, i, m.start() + at, strand))
                        if call is not None:
                            out[i, 0 if call else 1] += 1
            self._brute[key] = out
        return self._brute[key]

    def batch(self, shapes, bins, contigs=None):
        """Every shape for both mod types on each of ``bins``: ([(Motif, mod type, bin name)], their brute-force table over ``contigs``)."""
        contigs = range(len(self.names)) if contigs is None else contigs
        cands, want = [], []
        for b in bins:
            mine = [i for i in contigs if self.bins[i] == self.bin_names[b]]
            for mt in ("a", "m"):
                for shape in shapes:
                    cands.append((motif_of(shape, mt)[0], mt, self.bin_names[b]))
                    want.append(self.brute(shape, mt)[mine].sum(axis=0))
        return cands, np.array(want, dtype=np.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def engine(data):
    eng = data.engine()
    yield eng
    eng.close()


def _with_env(name, value, fn):
    assert name not in os.environ
    os.environ[name] = value
    try:
        return fn()
    finally:
        del os.environ[name]


def three_ways(run):
    """The call as it is, on the plain list, and (packed list) on the 8-plane kernel."""
    return run(), _with_env("NM_SCORE_PACK_TAILS", "0", run), _with_env("NM_SCORE_CLASSES", "0", run)


def assert_three_ways(run, want):
    for what, got in zip(("packed", "plain list", "8-plane kernel"), three_ways(run)):
        bad = np.flatnonzero((np.asarray(got) != want).any(axis=1))
        assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5].tolist()}: got {np.asarray(got)[bad[:5]].tolist()}, brute force {want[bad[:5]].tolist()}"


def test_planted_sites_decide(data):
    """The brute force sees the planted sites: windows that end on a contig's last bp or start on bp 0 count, and there are windows
    one past the end / one before the start that only padding read as A would complete."""
    ends_a = [s for s in LITERALS + SETS if "A" in s[0].split()[-1] and s[0].split()[-1] != "*"]
    assert len(ends_a) >= 4
    n_last = n_first = 0
    for shape in LITERALS + SETS:
        for mt in ("a", "m"):
            _, sets, mp = motif_of(shape, mt)
            pattern = re.compile("(?=" + "".join("[%s]" % s for s in sets) + ")")
            for seq in data.seqs:
                starts = [m.start() for m in pattern.finditer(seq)]
                n_last += len(seq) - len(sets) in starts
                n_first += 0 in starts
    assert n_last >= 20 and n_first >= 20


@pytest.mark.parametrize("shapes", [LITERALS, MIXED, REACH_40], ids=["literals", "classes", "wide"])
def test_every_bin(data, engine, shapes):
    """All four bins (the static table over the list): the literal-only 4-plane kernel, the class kernel and its 8-plane twin, and a
    wide batch (two halo words a side)."""
    cands, want = data.batch(shapes, range(4))
    assert want.sum() > 0 and (want.sum(axis=1) > 0).sum() > len(want) // 2
    assert_three_ways(lambda: engine.score(cands), want)


def test_one_bin_of_four_brings_its_own_table(data, engine):
    """Candidates in one bin: the batch's own segment table, cut over list positions.  Bin 1 (100 chunks, 8 packed rows) crosses a
    multiple of 16 entries between the lists, bin 3 (one contig: 4 chunks, or 3 and a row) does not."""
    wgs = {}
    for b in (1, 3):
        cands, want = data.batch(MIXED, [b])
        assert want.sum() > 0
        got = []
        for env in (None, "0"):
            run = lambda: engine.score(cands)
            got.append(run() if env is None else _with_env("NM_SCORE_PACK_TAILS", env, run))
            wgs[(b, env)] = engine.stats()["last_workgroups"]
        assert got[0].tolist() == want.tolist() and got[1].tolist() == want.tolist()
        assert _with_env("NM_SCORE_CLASSES", "0", lambda: engine.score(cands)).tolist() == want.tolist()
    print("last_workgroups", wgs)
    assert wgs[(1, None)] < wgs[(1, "0")]
    assert wgs[(3, None)] == wgs[(3, "0")]


def test_device_counts_on_two_lanes(data, engine):
    import torch
    batches = [data.batch(MIXED, [b]) for b in range(4)] + [data.batch(LITERALS, range(4))]

    def run():
        tables = [torch.full((len(c), 2), -1, dtype=torch.int64, device="cuda:0") for c, _ in batches]
        made = [engine.make_batch(c) for c, _ in batches]
        engine.set_score_lanes(2)
        try:
            for b, t in zip(made, tables):
                engine.score_into_device(b, t.data_ptr())
            engine.sync()
        finally:
            engine.set_score_lanes(1)
        return np.concatenate([t.cpu().numpy() for t in tables])
    assert_three_ways(run, np.concatenate([w for _, w in batches]))


def test_subset_of_the_contigs(data):
    """An engine that holds two contigs in three of bins 0, 1 and 3 and nothing of bin 2: other tails share the rows."""
    keep = [i for i in range(len(data.names)) if data.bins[i] != "bin_2" and i % 3 != 1]
    eng = data.engine(keep)
    try:
        cands, want = data.batch(MIXED, range(4), contigs=keep)
        assert want.sum() > 0 and want[len(want) // 2: 3 * len(want) // 4].sum() == 0          # (bin 2 is not resident)
        assert_three_ways(lambda: eng.score(cands), want)
    finally:
        eng.close()


def test_per_contig_rows_are_what_they_were(data, engine):
    """score_per_contig does not walk the list: the same rows whatever the switch says, and the brute force's."""
    cands, _ = data.batch(MIXED[:12], range(4))
    shapes = [(shape, mt) for _ in range(4) for mt in ("a", "m") for shape in MIXED[:12]]

    def run():
        return engine.score_per_contig(cands)
    for got in three_ways(run):
        for (names, table), (shape, mt) in zip(got, shapes):
            rows = [data.names.index(n) for n in names]
            assert table.tolist() == data.brute(shape, mt)[rows].tolist()
