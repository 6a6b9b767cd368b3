"""The parked class kernel (csrc/nmscan_device.h: Variant::PARK — a chunk's state words M and U wait in LDS through the walks, 28
candidates a pass, 7 waves per SIMD) against the unparked instantiation (NM_SCORE_PARK=0), the 8-plane kernel (NM_SCORE_CLASSES=0)
and a brute force, by equality.  0.22 Mbp in four bins whose work lists are 17, 5, 3 and 4 entries long (segments of 16, 1, 5, 3
and 4): all-valid chunks, boundary chunks and packed tail rows, waves with no, one, two and four entries.  The park slot of a
thread is rewritten once per entry: on the engine that hands a workgroup a whole segment (NM_SPLIT=0, NM_FINE=0) every wave of
bin 0 walks four entries whose state words differ pairwise in every lane (asserted on the host from the uploaded calls, as is the
number of workgroups that grid launches), and a slot left stale would count another chunk's calls.
Which instantiation a call launched is read from the engine (stats()["last_parked"]), never inferred."""
import os

import numpy as np
import pytest

from test_gpu_score_tail_pack import CANONICAL, CHUNK, COMPLEMENT, STRIP, Data, _with_env, motif_of

pytestmark = pytest.mark.gpu

# contigs per bin -> list entries (chunks whose 64 strips hold sequence, then rows of 64 strips of the partly filled ones)
CONTIGS = [[14 * CHUNK + 3000, CHUNK + 50 * STRIP, 40 * STRIP],        # 15 chunks (13 all-valid) + 114 strips = 2 rows: 17
           [4 * CHUNK + 2000, 40 * STRIP],                            # 4 chunks + 56 strips = 1 row: 5
           [2 * CHUNK + 1000],                                        # 2 chunks + 8 strips: 3
           [3 * CHUNK + 64]]                                          # 3 chunks + 1 strip: 4
ENTRIES = [17, 5, 3, 4]
# candidates per (bin, mod type) group; PARKED: one pass (1 .. 28) and two (33, 56) at 28 rows as at 32
PARKED = {(0, "a"): 56, (0, "m"): 33, (1, "a"): 28, (1, "m"): 27, (2, "a"): 10, (2, "m"): 1, (3, "a"): 28, (3, "m"): 10}
UNPARKED_SIZES = [29, 32, 57]                                          # one pass more at 28 rows than at 32
BASES = "ACGT"


def list_entries(lengths):
    """(entries, all-valid chunks, boundary chunks, rows) of a bin's packed list (csrc/nmscore_worklist.h)."""
    full = valid = strips = 0
    for n in lengths:
        for q in range((n + 96 + CHUNK - 1) // CHUNK):
            s = min(64, max(0, -(-(n - q * CHUNK) // STRIP)))
            if s == 64:
                full += 1
                valid += q >= 1 and (q + 1) * CHUNK + 96 <= n
            else:
                strips += s
    rows = -(-strips // 64)
    return full + rows, valid, full - valid, rows


def make_shapes(n, seed):
    """n distinct shapes in the neighbour suite's notation, in turn literals only, a lone class, several classes."""
    rng = np.random.default_rng(seed)
    two, three = ["AC", "AG", "AT", "CG", "CT", "GT"], ["ACG", "ACT", "AGT", "CGT"]
    out, seen = [], set()
    while len(out) < n:
        kind, length = len(out) % 3, int(rng.integers(3, 8))
        mp = int(rng.integers(0, length))
        sets = [BASES[rng.integers(0, 4)] if j in (0, length - 1) or rng.random() < 0.35 else "ACGT" for j in range(length)]
        free = [j for j in range(length) if j != mp]
        for j in rng.permutation(free)[:(0, 1, min(3, len(free)))[kind]]:
            pool = two if rng.random() < 0.6 else three
            sets[j] = pool[rng.integers(0, len(pool))]
        sets[mp] = "*"
        shape = (" ".join(sets), mp)
        if shape not in seen and any(len(s) < 4 for s in sets if s != "*") and (kind == 0 or any(1 < len(s) < 4 for s in sets)):
            seen.add(shape)
            out.append(shape)
    return out


class ParkData(Data):
    """The neighbour suite's Data (its engine(), its regex brute()) over the contigs above, and a numpy brute force for the many shapes."""

    def __init__(self, seed=5):
        rng = np.random.default_rng(seed)
        self.names, self.bins, self.seqs = [], [], []
        for k in range(max(len(c) for c in CONTIGS)):               # upload order mixes the bins
            for b, contigs in enumerate(CONTIGS):
                if k < len(contigs):
                    self.names.append("contig_%d_%d" % (b, k))
                    self.bins.append("bin_%d" % b)
                    self.seqs.append("".join(rng.choice(list(BASES), size=contigs[k])))
        assert sum(len(s) for s in self.seqs) <= 300_000
        self.bin_names = sorted(set(self.bins))
        self.calls, self.columns, self.state, self._brute, self._fast, self._member = {}, {}, {}, {}, {}, {}
        self.codes = [np.frombuffer(s.encode(), dtype=np.uint8) for s in self.seqs]
        for mt, base in CANONICAL.items():
            cid, pos, strand, frac = [], [], [], []
            for i, a in enumerate(self.codes):
                for st, letter in (("+", base), ("-", COMPLEMENT[base])):
                    p = np.flatnonzero(a == ord(letter))
                    f = rng.choice([0.95, 0.05, 0.5], size=len(p), p=[0.45, 0.45, 0.1])
                    cid.append(np.full(len(p), i, np.uint32)); pos.append(p.astype(np.uint32)); strand.append(np.full(len(p), ord(st), np.uint8)); frac.append(f)
                    state = np.zeros(len(a), np.uint8)                  # 1 methylated, 2 not, 0 no call
                    state[p[f > 0.5]] = 1
                    state[p[f < 0.5]] = 2
                    self.state[(mt, i, st)] = state
            self.columns[mt] = tuple(np.concatenate(x) for x in (cid, pos, strand, frac))

    def fill_calls(self):
        """The dict the neighbour's regex brute force looks calls up in."""
        for (mt, i, st), state in self.state.items():
            for q in np.flatnonzero(state).tolist():
                self.calls[(mt, i, q, st)] = state[q] == 1

    def member(self, i, letters):
        """bool[len]: contig i holds one of ``letters`` there."""
        key = (i, letters)
        if key not in self._member:
            self._member[key] = np.isin(self.codes[i], np.frombuffer(letters.encode(), dtype=np.uint8))
        return self._member[key]

    def fast(self, shape, mt):
        """int64[n_contigs, 2] like Data.brute: windows by shifted comparisons instead of a regex."""
        key = (shape, mt)
        if key not in self._fast:
            _, sets, mp = motif_of(shape, mt)
            rc = ["".join(COMPLEMENT[x] for x in s) for s in reversed(sets)]
            out = np.zeros((len(self.seqs), 2), dtype=np.int64)
            for st, ss, at in (("+", sets, mp), ("-", rc, len(sets) - 1 - mp)):
                for i, a in enumerate(self.codes):
                    n = len(a) - len(ss) + 1
                    if n <= 0:
                        continue
                    hit = np.ones(n, dtype=bool)
                    for j, s in enumerate(ss):
                        if len(s) < 4:
                            hit &= self.member(i, s)[j:j + n]
                    state = self.state[(mt, i, st)][at:at + n][hit]
                    out[i, 0] += int((state == 1).sum())
                    out[i, 1] += int((state == 2).sum())
            self._fast[key] = out
        return self._fast[key]

    def entry_words(self, b, mt):
        """uint8[entries, 64, 2, 128]: what lane l of entry e of bin b's packed list holds in its state words — bit (plane, bp) of its
        128 bp strip: plane 0 = M (a methylated call, either strand), 1 = U — in list order (csrc/nmscore_worklist.h): the bin's chunks
        whose 64 strips hold sequence, contig by contig, then rows of 64 strips taken from the partly filled chunks."""
        chunks, strips = [], []
        for i in (i for i in range(len(self.names)) if self.bins[i] == self.bin_names[b]):          # upload order inside the bin
            state = self.state[(mt, i, "+")] | self.state[(mt, i, "-")]                                # (the strands' calls sit on different bases)
            n = len(state)
            padded = np.zeros((n + 96 + CHUNK - 1) // CHUNK * CHUNK, np.uint8)
            padded[:n] = state
            for q in range(len(padded) // CHUNK):
                held = min(64, max(0, -(-(n - q * CHUNK) // STRIP)))
                rows = padded[q * CHUNK:(q + 1) * CHUNK].reshape(64, STRIP)
                if held == 64:
                    chunks.append(rows)
                else:
                    strips.extend(rows[:held])
        while len(strips) % 64:
            strips.append(np.zeros(STRIP, np.uint8))
        entries = np.array(chunks + [np.array(strips[r:r + 64]) for r in range(0, len(strips), 64)])
        return np.stack([entries == 1, entries == 2], axis=2).astype(np.uint8)

    def groups(self, sizes, shapes):
        """[(Motif, mod type, bin name)] with sizes[(bin, mt)] candidates a group, and their brute-force table."""
        cands, want, at = [], [], 0
        for (b, mt), n in sizes.items():
            mine = [i for i in range(len(self.names)) if self.bins[i] == self.bin_names[b]]
            for k in range(n):
                shape = shapes[(at + k) % len(shapes)]
                cands.append((motif_of(shape, mt)[0], mt, self.bin_names[b]))
                want.append(self.fast(shape, mt)[mine].sum(axis=0))
            at += 7
        return cands, np.array(want, dtype=np.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def data():
    return ParkData()


@pytest.fixture(scope="module")
def shapes():
    return make_shapes(57, seed=23)


WHOLE_SEGMENTS = {}            # id(engine) -> it was made with NM_SPLIT=0 NM_FINE=0


@pytest.fixture(scope="module", params=["whole segments", "default grid"])
def engine(request, data):
    """'whole segments': a workgroup walks a whole segment (16 entries: four a wave); default: a small assembly is cut into quarters."""
    env = {"NM_SPLIT": "0", "NM_FINE": "0"} if request.param == "whole segments" else {}
    assert not any(k in os.environ for k in ("NM_SPLIT", "NM_FINE", "NM_SCORE_PARK", "NM_SCORE_CLASSES"))
    os.environ.update(env)
    try:
        eng = data.engine()
    finally:
        for k in env:
            del os.environ[k]
    WHOLE_SEGMENTS[id(eng)] = request.param == "whole segments"
    yield eng
    eng.close()


def ways(engine, run, parked):
    """The call as it is, on the unparked instantiation and on the 8-plane kernel: [(what, counts)], the launched instantiation asserted."""
    out = []
    for what, env, want_parked in (("default", None, parked), ("NM_SCORE_PARK=0", ("NM_SCORE_PARK", "0"), 0), ("NM_SCORE_CLASSES=0", ("NM_SCORE_CLASSES", "0"), 0)):
        got = run() if env is None else _with_env(env[0], env[1], run)
        assert engine.stats()["last_parked"] == want_parked, f"{what}: last_parked {engine.stats()['last_parked']}"
        out.append((what, np.asarray(got)))
    return out


def assert_ways(engine, run, want, parked):
    for what, got in ways(engine, run, parked):
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5].tolist()}: got {got[bad[:5]].tolist()}, brute force {want[bad[:5]].tolist()}"


def test_lists_are_what_the_cases_need():
    got = [list_entries(c) for c in CONTIGS]
    assert [g[0] for g in got] == ENTRIES
    assert got[0] == (17, 13, 2, 2) and all(g[1] >= 1 and g[2] >= 1 and g[3] >= 1 for g in got)   # all-valid, boundary, packed: in every bin


@pytest.mark.parametrize("mt", ["a", "m"])
def test_a_wave_of_the_long_segment_walks_four_entries_of_different_state_words(data, mt):
    """What the stale-slot coverage rests on, asserted: bin 0's first segment has 16 entries, a workgroup that holds it whole gives wave
    w the entries w, w + 4, w + 8, w + 12 (score_piece: ``for ck = wave; ck < sg.y; ck += 4``), and in EVERY lane the four M words and
    the four U words a wave parks one after the other differ pairwise — a slot that kept an earlier entry's words counts other calls.
    Wave 3 ends on a packed row (entry 15)."""
    words = data.entry_words(0, mt)
    assert words.shape[:2] == (ENTRIES[0], 64)
    for wave in range(4):
        mine = words[[wave, wave + 4, wave + 8, wave + 12]]
        for x in range(4):
            for y in range(x + 1, 4):
                differ = (mine[x] != mine[y]).any(axis=2)                  # [lane, plane]
                assert differ.all(), f"wave {wave}: entries {wave + 4 * x} and {wave + 4 * y} park equal words in lanes {np.flatnonzero(~differ.all(axis=1))[:5].tolist()}"
    assert list_entries(CONTIGS[0])[0] - list_entries(CONTIGS[0])[3] == 15                         # entries 15 and 16 are the rows


def test_shapes_mix_the_kinds(shapes):
    kinds = [sum(1 < len(s) < 4 for s in shape[0].split()) for shape in shapes]
    assert len(set(shapes)) == 57 and kinds.count(0) >= 15 and kinds.count(1) >= 15 and sum(k >= 2 for k in kinds) >= 10


def test_brute_force_is_the_neighbours(data, shapes):
    """The shifted-comparison brute force against the regex one of tests/test_gpu_score_tail_pack.py, on shapes of every kind."""
    data.fill_calls()
    for shape in shapes[:6]:
        for mt in ("a", "m"):
            assert data.fast(shape, mt).tolist() == data.brute(shape, mt).tolist()
            assert data.fast(shape, mt).sum() > 0


def test_parked_groups(data, engine, shapes):
    """Groups of 1, 10, 27, 28 (one pass) and 33, 56 (two) in one batch over all four bins and both mod types."""
    cands, want = data.groups(PARKED, shapes)
    assert (want.sum(axis=1) > 0).sum() > len(want) * 3 // 4
    assert_ways(engine, lambda: engine.score(cands), want, parked=1)
    # five segments (16 + 1, 5, 3, 4) in runs of eight workgroups, two mod types; whole segments: no piece is cut, so the 16-entry
    # segment is one workgroup's and each of its waves walks four entries
    if WHOLE_SEGMENTS[id(engine)]:
        assert engine.stats()["last_workgroups"] == 16
    else:
        assert engine.stats()["last_workgroups"] > 16


@pytest.mark.parametrize("size", UNPARKED_SIZES)
def test_a_group_with_one_more_pass_unparks_the_batch(data, engine, shapes, size):
    sizes = dict(PARKED)
    sizes[(1, "m")] = size
    cands, want = data.groups(sizes, shapes)
    assert_ways(engine, lambda: engine.score(cands), want, parked=0)


@pytest.mark.parametrize("b", [0, 1, 2, 3])
def test_one_bin_brings_its_own_table(data, engine, shapes, b):
    """Candidates of one bin: the batch's own segments — 16 + 1, 5, 3 and 4 entries."""
    cands, want = data.groups({(b, "a"): 28, (b, "m"): 33}, shapes)
    assert want.sum() > 0
    assert_ways(engine, lambda: engine.score(cands), want, parked=1)


def test_device_counts_on_two_lanes(data, engine, shapes):
    import torch
    batches = [data.groups({(b, "a"): 27, (b, "m"): 10}, shapes) for b in range(4)] + [data.groups(PARKED, shapes)]

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
    assert_ways(engine, run, np.concatenate([w for _, w in batches]), parked=1)
