"""Paths of the scoring call (csrc/nmscan.hip: score_impl, planned in csrc/nmscore_plan.h) that no other test reaches: the batch's
own segment table at its crossover, growth of the program buffer between calls, the copy-engine ways in and out of a batch above
4 MiB, and the two compile paths either side of 2048 light candidates.  Counts are compared by equality with a brute force written
here — a regex over the contig strings and a dict of the uploaded calls — and, where named, with the same engine under its A/B switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nanomotif_amd.motif import Motif

pytestmark = pytest.mark.gpu

CANONICAL = {"a": "A", "m": "C"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
# (sets per position, modified position) — the canonical base of the mod type goes where the * stands
SHAPES = [("G * T C", 1), ("* C G", 0), ("C C * G G", 2), ("T AT * A", 2), ("G ACG * ACGT T", 2), ("* ACGT G CT", 0), ("AG * T", 1),
          ("A ACGT ACGT * C", 3), ("T * ACGT ACGT G", 1), ("CG * CG", 1), ("* A", 0), ("ACT * G", 1), ("G G * ACGT ACGT ACGT C", 2), ("*", 0)]


def _token(s):
    return s if len(s) == 1 else "." if len(s) == 4 else "[" + s + "]"


def motif_of(shape, mt):
    """(Motif for the engine, sets per position, modified position) of a shape for a mod type."""
    sets = [CANONICAL[mt] if t == "*" else t for t in shape[0].split()]
    return Motif("".join(_token(s) for s in sets), shape[1]), sets, shape[1]


class Data:
    """n_bins bins of one contig each, calls of two mod types on every canonical base of both strands."""

    def __init__(self, n_bins, contig_bp, seed):
        rng = np.random.default_rng(seed)
        self.names = ["contig_%03d" % i for i in range(n_bins)]
        self.bins = ["bin_%03d" % i for i in range(n_bins)]
        self.seqs = ["".join(rng.choice(list("ACGT"), size=contig_bp)) for _ in range(n_bins)]
        self.calls = {}            # (mod type, contig, position, strand) -> "mod" / "nomod"; the rows in between are uploaded too
        self.columns = {}
        for mt, base in CANONICAL.items():
            cid, pos, strand, frac = [], [], [], []
            for i, s in enumerate(self.seqs):
                a = np.frombuffer(s.encode(), dtype=np.uint8)
                for st, letter in (("+", base), ("-", COMPLEMENT[base])):
                    p = np.flatnonzero(a == ord(letter))
                    f = rng.choice([0.95, 0.05, 0.5], size=len(p), p=[0.4, 0.4, 0.2])
                    cid.append(np.full(len(p), i, np.uint32)); pos.append(p.astype(np.uint32)); strand.append(np.full(len(p), ord(st), np.uint8)); frac.append(f)
                    for q, v in zip(p.tolist(), f.tolist()):
                        if v != 0.5:
                            self.calls[(mt, i, q, st)] = "mod" if v > 0.5 else "nomod"
            self.columns[mt] = tuple(np.concatenate(x) for x in (cid, pos, strand, frac))
        self._brute = {}

    def engine(self):
        from nanomotif_amd.engine import ScanEngine
        eng = ScanEngine(0)
        eng.upload_assembly(self.names, self.seqs, self.bins)
        for mt in ("a", "m"):
            eng.upload_pileup(mt, *self.columns[mt])
        return eng

    def brute(self, shape, mt, b):
        """(n_mod, n_nomod) of a shape on the contig of bin b: every (overlapping) regex match of the motif on the '+' strand and of
        its reverse complement on the '-' strand, looked up in the calls."""
        key = (shape, mt, b)
        if key not in self._brute:
            _, sets, mp = motif_of(shape, mt)
            rc = ["".join(COMPLEMENT[x] for x in s) for s in reversed(sets)]
            n = {"mod": 0, "nomod": 0, None: 0}
            for strand, ss, at in (("+", sets, mp), ("-", rc, len(sets) - 1 - mp)):
                pattern = re.compile("(?=" + "".join("[%s]" % s for s in ss) + ")")
                for m in pattern.finditer(self.seqs[b]):
                    n[self.calls.get((mt, b, m.start() + at, strand))] += 1
            self._brute[key] = (n["mod"], n["nomod"])
        return self._brute[key]

    def batch(self, groups, per_group, first_shape=0):
        """per_group candidates for every (mod type, bin) of groups: ([(Motif, mod type, bin name)], their brute-force table)."""
        cands, want = [], []
        for g, (mt, b) in enumerate(groups):
            for k in range(per_group):
                shape = SHAPES[(first_shape + g + k) % len(SHAPES)]
                cands.append((motif_of(shape, mt)[0], mt, self.bins[b]))
                want.append(self.brute(shape, mt, b))
        return cands, np.array(want, dtype=np.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def eight():
    return Data(8, 20_000, seed=5)


@pytest.fixture(scope="module")
def eight_engine(eight):
    eng = eight.engine()
    yield eng
    eng.close()


def _with_all_segments(fn):
    os.environ["NM_ALL_SEGMENTS"] = "1"
    try:
        return fn()
    finally:
        del os.environ["NM_ALL_SEGMENTS"]


@pytest.mark.parametrize("n_bins_used", [1, 6, 7])
@pytest.mark.parametrize("style", ["light", "heavy", "per_contig"])
def test_own_segment_table_against_all_segments(eight, eight_engine, n_bins_used, style):
    """8 bins of one segment each: a batch with candidates in 6 of them brings its own segment table (4 * 6 <= 3 * 8), one with 7
    walks the static table; NM_ALL_SEGMENTS=1 keeps every batch on the static one."""
    eng = eight_engine
    assert "NM_ALL_SEGMENTS" not in os.environ
    bins = [1, 7, 4, 0, 6, 2, 5][:n_bins_used]
    groups = [(mt, b) for b in bins for mt in ("a", "m")]
    cands, want = eight.batch(groups, 6 if style == "light" else 7, first_shape=n_bins_used)
    if style == "per_contig":
        run = lambda: np.concatenate([t for _, t in eng.score_per_contig(cands)])       # one contig per bin: one row per candidate
    else:
        run = lambda: eng.score(cands)
    own = run()
    own_wgs = eng.stats()["last_workgroups"]
    ref = _with_all_segments(run)
    ref_wgs = eng.stats()["last_workgroups"]
    print("bins", n_bins_used, style, "workgroups", own_wgs, "with every segment", ref_wgs, "nonzero rows", int((want.sum(axis=1) > 0).sum()))
    assert own.tolist() == want.tolist()
    assert ref.tolist() == want.tolist()
    assert want.sum() > 0
    assert (own_wgs < ref_wgs) if n_bins_used <= 6 else (own_wgs == ref_wgs)


def test_program_buffer_growth_between_calls(eight):
    """1 candidate, then 600 (the program buffer grows), then 1 again: the same counts as each call on a fresh engine."""
    groups = [(mt, b) for b in range(8) for mt in ("a", "m")]
    one, want_one = eight.batch(groups[:1], 1)
    many, want_many = eight.batch(groups * 38, 1)
    many, want_many = many[:600], want_many[:600]
    eng = eight.engine()
    got = [eng.score(one), eng.score(many), eng.score(one)]
    eng.close()
    fresh = []
    for batch in (one, many, one):
        e = eight.engine()
        fresh.append(e.score(batch))
        e.close()
    for g, f, w in zip(got, fresh, (want_one, want_many, want_one)):
        assert g.tolist() == w.tolist()
        assert f.tolist() == w.tolist()


def test_copy_engine_paths_above_4_mib():
    """262 145 candidates on one bin of one chunk: the staged tables and the count table both exceed 4 MiB, so the tables go in and
    the counts come out through the copy engines — by nm_score_batch, nm_score_batch_device and nm_score_batch_begin / _end."""
    import torch
    from nanomotif_amd import _lib
    from nanomotif_amd.engine import CandidateBatch
    data = Data(1, 8_000, seed=6)
    eng = data.engine()
    ten = [(mt, shape) for mt in ("a", "m") for shape in SHAPES[:5]]
    base = eng.make_batch([(motif_of(shape, mt)[0], mt, data.bins[0]) for mt, shape in ten])
    want_ten = np.array([data.brute(shape, mt, 0) for mt, shape in ten], dtype=np.int64)
    n = 262_145
    idx = np.arange(n) % 10
    big = CandidateBatch(np.zeros(n, np.uint32), np.ascontiguousarray(base.slots[idx]), np.ascontiguousarray(base.lens[idx]),
                         np.ascontiguousarray(base.modpos[idx]), np.ascontiguousarray(base.offsets[idx]), base.masks)
    want = want_ten[idx]
    assert n * 16 > (4 << 20) and want_ten.sum() > 0    # 16 bytes a candidate of records + orig_index staged, 16 of counts
    host = eng.score(big)
    dev = torch.full((n, 2), -1, dtype=torch.int64, device="cuda:0")
    eng.score_into_device(big, dev.data_ptr())
    eng.sync()
    later = np.full((n, 2), -1, dtype=np.int64)
    _lib.check(eng.lib.nm_score_batch_begin(eng.ctx, *eng._batch_args(big)))
    _lib.check(eng.lib.nm_score_batch_end(eng.ctx, later.ctypes.data_as(C.POINTER(C.c_int64))))
    eng.close()
    assert np.array_equal(host, want)
    assert np.array_equal(dev.cpu().numpy(), want)
    assert np.array_equal(later, want)


def test_compile_paths_either_side_of_2048_light_candidates():
    """2 x 171 groups of one-chunk bins: 2048 light candidates are compiled and factored by one launch, 2049 by two."""
    data = Data(171, 3_000, seed=7)
    eng = data.engine()
    groups = [(mt, b) for b in range(171) for mt in ("a", "m")]
    cands, want = data.batch(groups, 6)                 # 2052 candidates, six per group
    for n in (2048, 2049):
        got = eng.score(cands[:n])
        assert eng.stats()["last_compact"] == n
        assert got.tolist() == want[:n].tolist()
    assert want[:2048].sum() > 0
    eng.close()
