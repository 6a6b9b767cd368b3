"""nm_ingest_pileup (csrc/nmingest.hip: the counting pass, the classification pass with its key cache, memo, LDS window and queue, the pack and
judge kernels of the list path) against oracle.pileup.prefilter on the geometry input of tests/ingest_geometry.py, by equality only: n_kept,
the kept table, the confident rows and the state of every position of every contig per scored code and strand (motif_sites on the one-letter
motifs: the unmethylated planes position by position).

A call of up to 2 097 152 rows gives every wave 64 rows, one trip of every loop; NM_INGEST_WALK_BLOCKS=1 / 3 makes 4 / 12 waves walk the table,
thousands of rows each, as the waves of a 1e9-row call do.  Every cell reads the NM_INGEST_TIMING line and asserts the path that ran and the
rows per wave the restated split predicts: a cell that silently ran 64 rows a wave, or the other path, fails.  All cells of one table are
compared with one expectation, so they equal each other.  tests/test_ingest_geometry_host.py shows on the CPU that every border is in the input."""
import re

import numpy as np
import pytest

import ingest_geometry as ig
from nanomotif_amd.motif import Motif

pytestmark = pytest.mark.gpu

LABELS = {code: lb for code, lb in ig.SCORED.items()}
LINE = re.compile(r"\[nm_ingest\] (\d+) rows: waiting for earlier work .* freeing scratch [0-9.]+ ms, path (no rows|list|dense stores|dense atomics), "
                  r"walk (\d+) waves x (\d+) rows(?:, list (\d+) waves x (\d+) entries)?$")
MODES = {"as it is": (None, "list"), "dense": ("NM_INGEST_DENSE", "dense stores"), "atomic": ("NM_INGEST_ATOMIC", "dense atomics")}
SWITCHES = ("NM_INGEST_WALK_BLOCKS", "NM_INGEST_DENSE", "NM_INGEST_ATOMIC")


@pytest.fixture(scope="module")
def eng():
    from nanomotif_amd.engine import ScanEngine
    g = ig.build_input()
    e = ScanEngine(0)
    e.upload_assembly(g.names, g.seqs, ["b"] * len(g.names))
    yield e
    e.close()


def _ingest(eng, table, capfd, monkeypatch, k=None, switch=None, rows=slice(None), **kw):
    """one ingest of ``table`` on the engine as it stands -> (result, [(rows, path, waves, rows per wave, list waves, entries per wave)] per call)"""
    g = ig.build_input()
    monkeypatch.setenv("NM_INGEST_TIMING", "1")
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if k:
        monkeypatch.setenv("NM_INGEST_WALK_BLOCKS", str(k))
    if switch:
        monkeypatch.setenv(switch, "1")
    frac = table["fraction_mod"][rows]
    capfd.readouterr()
    res = eng.ingest_pileup(g.lut[table["contig"][rows]].astype(np.uint32), table["position"][rows], table["mod_type"][rows], table["strand"][rows],
                            np.where(np.isnan(frac), -1.0, frac), table["Nvalid_cov"][rows], LABELS, **kw)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "[nm_ingest]" in ln]
    found = [LINE.search(ln) for ln in lines]
    assert all(found), lines
    return res, [(int(m[1]), m[2], int(m[3]), int(m[4]), m[5] and int(m[5]), m[6] and int(m[6])) for m in found]


def _sites(eng):
    """{code: int64[n, 3] (contig, position, site code) of every occurrence of the code's one-letter motif, sorted}"""
    cands = [(Motif(base, 0), label, "b") for _, (label, base) in sorted(ig.SCORED.items())]
    rec = np.concatenate([b.records for b in eng.motif_sites(cands)])
    out = {}
    for j, code in enumerate(sorted(ig.SCORED)):
        r = rec[rec["candidate"] == j]
        a = np.stack([r["contig"].astype(np.int64), r["pos"].astype(np.int64), r["code"].astype(np.int64)], axis=1)
        out[code] = a[np.lexsort((a[:, 1], a[:, 0]))]
    return out


def _assert_equals_oracle(eng, res, e, cell):
    assert res["n_kept"] == e.n_kept, cell
    assert np.array_equal(res["kept"].astype(np.int64), e.kept), (cell, np.argwhere(res["kept"] != e.kept)[:8].tolist())
    assert res["n_confident"] == len(e.confident), cell
    assert sorted(zip(*[x.tolist() for x in res["confident"]])) == e.confident, cell
    got = _sites(eng)
    for code, want in e.sites.items():
        want = np.array(want, dtype=np.int64).reshape(-1, 3)
        assert got[code].shape == want.shape, (cell, code)
        wrong = np.flatnonzero((got[code] != want).any(axis=1))
        assert len(wrong) == 0, (cell, code, len(wrong), got[code][wrong[:8]].tolist(), want[wrong[:8]].tolist())


def _assert_line(line, n, k, path, cell, e=None):
    waves, per = ig.wave_split(n, k)
    assert line[:4] == (n, path, waves, per), (cell, line)
    if path == "list" and e is not None:
        blocks = max(1, min((e.cap + 255) // 256, 8192))
        list_waves = 4 * (min(blocks, k) if k else blocks)
        assert line[4:] == (list_waves, ig.round_up_64(-(-e.n_candidates // list_waves))), (cell, line)
    else:
        assert (line[4] is None) == (path != "list"), (cell, line)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("k", ig.GRIDS, ids=["unset", "k1", "k3"])
def test_table_in_modkit_order(eng, capfd, monkeypatch, k, mode):
    """the table as modkit writes it: the list path, and the dense path with plain stores and with atomics, 64 / 15 040 / 5 056 rows a wave"""
    g = ig.build_input()
    switch, path = MODES[mode]
    res, lines = _ingest(eng, g.table, capfd, monkeypatch, k, switch)
    assert len(lines) == 1
    _assert_line(lines[0], ig.N_ROWS, k, path, (k, mode), ig.expected_of())
    if k == 1 and path == "list":
        assert lines[0][5] > 64 * 50                                    # the judge kernel makes many trips per wave
    _assert_equals_oracle(eng, res, ig.expected_of(), (k, mode))


@pytest.mark.parametrize("k", (None, 1), ids=["unset", "k1"])
def test_table_shuffled(eng, capfd, monkeypatch, k):
    """rows in no order: the window is flushed with atomics in every iteration, on a long walk at k = 1"""
    g = ig.build_input()
    order = np.random.default_rng(11).permutation(ig.N_ROWS)
    res, lines = _ingest(eng, {c: v[order] for c, v in g.table.items()}, capfd, monkeypatch, k)
    assert len(lines) == 1
    _assert_line(lines[0], ig.N_ROWS, k, "dense atomics", ("shuffled", k))
    _assert_equals_oracle(eng, res, ig.expected_of(), ("shuffled", k))


@pytest.mark.parametrize("k", (None, 1), ids=["unset", "k1"])
def test_table_in_parts(eng, capfd, monkeypatch, k):
    """nm_ingest_pileup_part, a call per contig of 65 rows or more: the planes and tables accumulate; the contig of 65 rows is a call of its own
    (65 rows, four waves: 64 rows and 1)"""
    from nanomotif_amd.engine import ScanEngine
    g = ig.build_input()
    parts = ScanEngine._pileup_parts(g.lut[g.table["contig"]].astype(np.uint32), 65)
    assert len(parts) > 20 and any(b - a == 65 and g.table["contig"][a] in g.marks["contig_65"] for a, b in parts)
    res, lines = _ingest(eng, g.table, capfd, monkeypatch, k, max_part_rows=65)
    assert len(lines) == len(parts)
    for line, (a, b) in zip(lines, parts):
        _assert_line(line, b - a, k, "list", ("parts", k, a, b))
    _assert_equals_oracle(eng, res, ig.expected_of(), ("parts", k))


@pytest.mark.parametrize("name", ig.variant_names())
def test_variant_breaks_the_order(eng, capfd, monkeypatch, name):
    """one position going down / a contig in two runs, at a wave's first row, at offsets 64 and 256 and in mid-piece: the counting pass has to see
    it on every grid (the line says `dense atomics`), and the result is the oracle's"""
    for k in ig.GRIDS:
        res, lines = _ingest(eng, ig.variant(name), capfd, monkeypatch, k)
        assert len(lines) == 1
        _assert_line(lines[0], ig.N_ROWS, k, "dense atomics", (name, k))
        _assert_equals_oracle(eng, res, ig.expected_of(name), (name, k))


def test_short_calls_return_zeros_and_leave_the_engine_usable(eng, capfd, monkeypatch):
    """calls of 1 .. 257 rows (prefixes of the table: nothing survives the frequency filter) report nothing and set no bit; the full table
    afterwards, on the same engine, is as correct as before"""
    g = ig.build_input()
    want = {code: np.array([(c, p, (s & 4) | 2) for c, p, s in rec], dtype=np.int64) for code, rec in ig.expected_of().sites.items()}
    for n in ig.PREFIXES:
        res, lines = _ingest(eng, g.table, capfd, monkeypatch, rows=slice(0, n))
        assert len(lines) == 1
        _assert_line(lines[0], n, None, "list", n)
        assert res["n_kept"] == 0 and res["n_confident"] == 0 and not res["kept"].any() and len(res["confident"][0]) == 0, n
        got = _sites(eng)
        assert all(np.array_equal(got[code], want[code]) for code in want), n            # every occurrence: nocall
    res, lines = _ingest(eng, g.table, capfd, monkeypatch)
    _assert_line(lines[0], ig.N_ROWS, None, "list", "after the short calls", ig.expected_of())
    _assert_equals_oracle(eng, res, ig.expected_of(), "after the short calls")
