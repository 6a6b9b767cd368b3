"""nm_motif_pileup_count / nm_motif_pileup_sites (csrc/nmpileup.hip), ``ScanEngine.motif_pileup_counts`` / ``motif_pileup`` and the
``motif_pileup`` command against the brute force of tests/test_motif_pileup_host.py on the geometry input of
tests/test_read_methylation_host.py: every comparison is equality and no record is left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_motif_fractions_host as F
import test_motif_pileup_host as P
import test_read_methylation_host as H
from nanomotif_amd.motif import Motif
from test_gpu_motif_fractions import _engine_candidates, _upload

pytestmark = pytest.mark.gpu
NM_EINVAL, NM_ESTATE, NM_ERANGE = -1, -3, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_NAMES = list(F.BINS_OF)
FIELDS = ["candidate", "contig", "pos", "code", "n_valid", "n_mod"]


def _engine(names, seqs, records, perm_seed=None):
    from nanomotif_amd.engine import ScanEngine
    eng = ScanEngine(0)
    eng.upload_assembly(names, [seqs[n] for n in names], [b for b in BIN_NAMES for _ in F.BINS_OF[b]], bin_names=BIN_NAMES)
    _upload(eng, names, records, perm_seed=perm_seed)
    return eng


@pytest.fixture(scope="module")
def geo():
    """The geometry input resident in three bins with the read statistics of codes a and m uploaded in ascending order, and the brute
    force's records of the candidate list (computed once per process, shared with the host suite)."""
    names, seqs, records, cands, rec = P.geometry()
    assert [n for b in BIN_NAMES for n in F.BINS_OF[b]] == names
    eng = _engine(names, seqs, records)
    yield dict(eng=eng, names=names, seqs=seqs, records=records, cands=cands, rec=rec)
    eng.close()


def _records(eng, cands, select, max_records=None, first_counts=None):
    """The concatenated records of ``ScanEngine.motif_pileup``, with the batches' bookkeeping checked."""
    parts, next_cand = [], 0
    for sb in eng.motif_pileup(_engine_candidates(cands), select=select, max_records=max_records):
        assert max_records is None or len(sb.records) <= max_records
        assert sb.records.dtype == P.RECORD and (sb.first_record == 0) == (sb.counts is not None)
        if sb.first_record == 0:
            assert sb.first_candidate == next_cand and len(sb.counts) == sb.n_candidates
            next_cand += sb.n_candidates
            if first_counts is not None:
                first_counts += sb.counts
        parts.append(sb.records)
    assert next_cand == len(cands)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=P.RECORD)


def _assert_records(got, want, cands, names, what):
    assert got.dtype == want.dtype == P.RECORD
    if len(got) != len(want) or not np.array_equal(got, want):
        n = min(len(got), len(want))
        differ = np.flatnonzero(got[:n] != want[:n])
        i = int(differ[0]) if len(differ) else n
        raise AssertionError((what, "records", len(got), "expected", len(want), "first difference at", i, "got", got[i:i + 3].tolist(), "expected",
                              want[i:i + 3].tolist(), cands[int(want[min(i, len(want) - 1)]["candidate"])]))


@pytest.mark.parametrize("select", P.SELECTS, ids="+".join)
def test_the_records_equal_the_brute_force(geo, select):
    counts = []
    got = _records(geo["eng"], geo["cands"], select, first_counts=counts)
    _assert_records(got, P.selected(geo["rec"], select), geo["cands"], geo["names"], select)
    assert len(got) > 50_000
    want = P.count_table(geo["rec"], geo["names"], F.BINS_OF, geo["cands"])          # the batches carry all four columns whatever the selection
    assert [n for n, _ in counts] == [F.BINS_OF[c[3]] for c in geo["cands"]] and all(np.array_equal(t, w) for (_, t), w in zip(counts, want))


def test_the_row_order_of_the_upload_plays_no_part(geo):
    eng = _engine(geo["names"], geo["seqs"], geo["records"], perm_seed=5)
    try:
        for select in P.SELECTS:
            _assert_records(_records(eng, geo["cands"], select), P.selected(geo["rec"], select), geo["cands"], geo["names"], ("permuted", select))
    finally:
        eng.close()


def test_the_concatenation_does_not_depend_on_the_window(geo):
    """A sub-list whose records number a few hundred (a window of ONE record is one library call each): GATC_a_1 in b0 in front, the
    candidate without a record in the middle.  Windows of 1 and 7 records, one that ends inside a lane's records, one that ends between two
    candidates, and the default."""
    cands, rec = geo["cands"], geo["rec"]
    per_cand = np.bincount(rec["candidate"], minlength=len(cands))
    small = [k for k in range(len(cands)) if per_cand[k] < 130]
    front = cands.index(("GATC", "a", 1, "b0"))
    order = [front] + [k for k in small if k != front]
    assert P.EMPTY_AT in order[1:-1] and 300 < int(per_cand[order].sum()) < 2_000 and len(order) >= 10
    sub = [cands[k] for k in order]
    want = np.concatenate([rec[rec["candidate"] == k] for k in order])
    want["candidate"] = np.repeat(np.arange(len(order), dtype=np.uint32), per_cand[order])
    first = want[want["candidate"] == 0]
    same_lane = np.flatnonzero((first["contig"][1:] == first["contig"][:-1]) & (first["pos"][1:] // P.LANE == first["pos"][:-1] // P.LANE)) + 1
    inside_a_lane, between_candidates = int(same_lane[same_lane > 7][0]), len(first)
    assert 7 < inside_a_lane < between_candidates == per_cand[front] and per_cand[order[1]] > 0
    for select in (("site", "bare"), ("site",)):
        w = P.selected(want, select)
        limits = (1, 7, inside_a_lane, between_candidates, None) if len(select) == 2 else (1, 5, None)
        for limit in limits:
            _assert_records(_records(geo["eng"], sub, select, max_records=limit), w, sub, geo["names"], (select, limit))
    with pytest.raises(ValueError, match="max_records"):
        list(geo["eng"].motif_pileup(_engine_candidates(sub), max_records=0))
    with pytest.raises(ValueError, match="selection"):
        list(geo["eng"].motif_pileup(_engine_candidates(sub), select=()))


def test_the_count_table_and_the_sums_are_those_of_motif_fractions(geo):
    """``motif_pileup_counts`` equals the brute force; its site columns are the histogram sums of ``motif_fractions`` and site + bare its
    occurrences; per (candidate, contig) the records' n_valid and n_mod sum to its sum_valid and sum_mod."""
    eng, cands, names = geo["eng"], geo["cands"], geo["names"]
    got = eng.motif_pileup_counts(_engine_candidates(cands))
    want = P.count_table(geo["rec"], names, F.BINS_OF, cands)
    assert len(got) == len(want) == len(cands)
    fractions = [(n, t.astype(np.int64)) for _, n, t in eng.motif_fractions(_engine_candidates(cands), bins=20)]
    rec = _records(eng, cands, ("site",))
    key = rec["candidate"].astype(np.int64) * len(names) + rec["contig"]
    sums = [np.bincount(key, weights=rec[f].astype(np.float64), minlength=len(cands) * len(names)).astype(np.int64).reshape(len(cands), len(names))
            for f in ("n_valid", "n_mod")]
    rows = 0
    for k, ((cn, table), w, (fn, ft), c) in enumerate(zip(got, want, fractions, cands)):
        assert cn == fn == F.BINS_OF[c[3]] and table.dtype == np.int64 and np.array_equal(table, w), (c, table.tolist(), w.tolist())
        assert np.array_equal(table[:, [0, 2]], ft[:, :, :20].sum(axis=2)) and np.array_equal(table[:, [0, 2]] + table[:, [1, 3]], ft[:, :, 20]), c
        at = [names.index(n) for n in cn]
        assert np.array_equal(sums[0][k, at], ft[:, :, 21].sum(axis=1)) and np.array_equal(sums[1][k, at], ft[:, :, 22].sum(axis=1)), c
        rows += len(cn)
    assert rows > 150 and eng.motif_pileup_counts([]) == [] and list(eng.motif_pileup([])) == []


def test_refusals_come_in_the_order_of_motif_fractions_and_leave_the_engine_usable(geo):
    from nanomotif_amd._lib import NmScanError, check
    from nanomotif_amd.engine import CandidateBatch, ScanEngine
    eng = geo["eng"]
    k0 = geo["cands"].index(("GATC", "a", 1, "b0"))
    cands = geo["cands"][k0:k0 + 6]
    want = np.concatenate([geo["rec"][geo["rec"]["candidate"] == k0 + j] for j in range(6)])
    want["candidate"] -= k0
    b = eng.make_batch(_engine_candidates(cands), slot_of=lambda mt: ["m", "a", "21839"].index(mt))
    rows = np.zeros(len(cands) + 1, dtype=np.uint64)
    np.cumsum([len(F.BINS_OF[c[3]]) for c in cands], out=rows[1:])
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))

    def count(batch=b, select=3, null=None, n=None, ctx=None, row_offset=rows):
        table, totals = np.full((int(rows[-1]), 4), -7, dtype=np.int64), np.zeros(len(cands), dtype=np.uint64)
        args = list(eng._batch_args(batch))
        if n is not None:
            args[0] = n
        tail = [p(row_offset, C.c_uint64), p(totals, C.c_uint64), p(table, C.c_int64)]
        if isinstance(null, int):
            args[null] = None
        elif null is not None:
            tail[("row_offset", "cand_total", "contig_counts").index(null)] = None
        check(eng.lib.nm_motif_pileup_count(eng.ctx if ctx is None else ctx, *args, select, *tail))
        return totals, table

    def sites(batch=b, select=3, null=None, n=None, ctx=None, first=0, capacity=len(want)):
        cols = [np.zeros(max(capacity, 1), dtype=t) for t in (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32)]
        off, written = np.full(len(cands) + 1, 99, dtype=np.uint64), C.c_uint64(99)
        args = list(eng._batch_args(batch))
        if n is not None:
            args[0] = n
        tail = [p(c, t) for c, t in zip(cols, (C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint32, C.c_uint32))] + [p(off, C.c_uint64), C.byref(written)]
        if isinstance(null, int):
            args[null] = None
        elif null is not None:
            tail[null[0]] = None
        check(eng.lib.nm_motif_pileup_sites(eng.ctx if ctx is None else ctx, *args, select, first, capacity, *tail))
        return cols, off, written.value

    def still_fine():
        _assert_records(_records(eng, cands, ("site", "bare")), want, cands, geo["names"], "after a refusal")

    def fractions_refusal(batch):
        with pytest.raises(NmScanError) as e:
            check(eng.lib.nm_motif_fractions_count(eng.ctx, *eng._batch_args(batch), 20, p(np.zeros((int(rows[-1]), 2, 23), np.uint64), C.c_uint64)))
        return e.value.code, str(e.value)

    def refused(code, match, call, **kw):
        with pytest.raises(NmScanError, match=match) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value)
        still_fine()
        return str(e.value)

    for call in (count, sites):
        for select in (0, 4, 5, 8, 1 << 31):
            refused(NM_EINVAL, "select", call, select=select)
        for null in (1, 2, 3, 4, 5, 6):
            refused(NM_EINVAL, "NULL", call, null=null)
    for null in ("row_offset", "cand_total", "contig_counts"):
        refused(NM_EINVAL, "NULL", count, null=null)
    for null in range(7):                                                                   # the five columns, cand_offset, n_written
        refused(NM_EINVAL, "NULL", sites, null=(null,))
    bad_rows = rows.copy()
    bad_rows[0] = 1
    refused(NM_EINVAL, r"row_offset\[0\]", count, row_offset=bad_rows)
    short = rows.copy()
    short[3:] -= 1
    refused(NM_EINVAL, "row_offset gives", count, row_offset=short)
    # one candidate wrong in two ways: the refusal is the one nm_motif_fractions_count gives, by both entry points
    k = np.arange(len(b))
    wide = eng.make_batch(_engine_candidates(cands[:2]) + [(Motif("A" + "." * 96 + "T", 0), "a", "b0")] + _engine_candidates(cands[3:]), slot_of=lambda mt: 1)
    wrong = {
        "bin and slot": (NM_EINVAL, CandidateBatch(np.where(k == 2, 3, b.bins).astype(np.uint32), np.where(k == 2, 2, b.slots).astype(np.uint8), b.lens, b.modpos, b.offsets, b.masks)),
        "slot and reach": (NM_ESTATE, CandidateBatch(wide.bins, np.where(k == 2, 7, wide.slots).astype(np.uint8), wide.lens, wide.modpos, wide.offsets, wide.masks)),
        "bin and reach": (NM_EINVAL, CandidateBatch(np.where(k == 2, 9, wide.bins).astype(np.uint32), wide.slots, wide.lens, wide.modpos, wide.offsets, wide.masks)),
        "reach": (NM_ERANGE, wide),
        "an earlier slot, a later bin": (NM_ESTATE, CandidateBatch(np.where(k == 4, 3, b.bins).astype(np.uint32), np.where(k == 1, 255, b.slots).astype(np.uint8), b.lens, b.modpos, b.offsets, b.masks)),
    }
    for what, (code, batch) in wrong.items():
        f_code, f_text = fractions_refusal(batch)
        assert f_code == code, (what, f_text)
        for call in (count, sites):
            assert refused(code, None, call, batch=batch) == f_text, what
    assert "candidate 2: cand_bin 3 >= n_bins 3" in fractions_refusal(wrong["bin and slot"][1])[1]
    assert "candidate 2: read-statistics slot 7 holds no pileup" in fractions_refusal(wrong["slot and reach"][1])[1]
    # n_cand = 0 is NM_OK and writes nothing but the empty prefix
    totals, table = count(n=0)
    assert (table == -7).all() and not totals.any()
    _, off, written = sites(n=0)
    assert off[0] == 0 and written == 0
    zero = np.zeros(1, dtype=np.uint64)
    assert eng.lib.nm_motif_pileup_count(eng.ctx, 0, None, None, None, None, None, None, 1, p(zero, C.c_uint64), None, None) == 0
    # the plain calls: the table need not be zeroed, the totals follow the selection, windows past the end and of no capacity
    full = P.count_table(geo["rec"], geo["names"], F.BINS_OF, geo["cands"])[k0:k0 + 6]
    for select in (1, 2, 3):
        totals, table = count(select=select)
        assert np.array_equal(table, np.concatenate(full))
        assert totals.tolist() == [int(t[:, [j for j in range(4) if select >> (j & 1) & 1]].sum()) for t in full]
    cols, off, written = sites()
    assert written == len(want) == off[-1] and off.tolist() == [0] + np.cumsum(np.bincount(want["candidate"], minlength=6)).tolist()
    for col, f in zip(cols, FIELDS[1:]):
        assert np.array_equal(col[:written], want[f]), f
    assert sites(first=len(want) + 5)[2] == 0 and sites(capacity=0)[2] == 0 and sites(first=len(want) - 3)[2] == 3
    # the engine's own refusal: a mod code without statistics, before the library is called
    with pytest.raises(ValueError, match="no read statistics are resident for mod type.s. 21839"):
        eng.motif_pileup([(Motif("GATC", 1), "21839", "b0")])
    with pytest.raises(ValueError, match="no read statistics are resident for mod type.s. 21839"):
        eng.motif_pileup_counts([(Motif("GATC", 1), "21839", "b0")])
    fresh = ScanEngine(0)                                                                   # no assembly
    with pytest.raises(NmScanError) as e:
        check(fresh.lib.nm_motif_pileup_count(fresh.ctx, *eng._batch_args(b), 3, p(rows, C.c_uint64), p(np.zeros(6, np.uint64), C.c_uint64),
                                              p(np.zeros((int(rows[-1]), 4), np.int64), C.c_int64)))
    assert e.value.code == NM_ESTATE and "nm_upload_contigs" in str(e.value)
    fresh.close()
    still_fine()


# ------------------------------------------------------------------------------------------------ the command
HEAD = "reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement\n"


def _write_input(tmp, names, seqs, records, cands):
    """The geometry input as an assembly, a bedMethyl pileup (rows in contig, position, strand, code order), a contig-bin table and a
    bin-motifs.tsv of ``cands``."""
    with open(tmp / "a.fasta", "w") as f:
        f.write("".join(f">{n}\n{seqs[n]}\n" for n in names))
    with open(tmp / "cb.tsv", "w") as f:
        f.write("".join(f"{n}\t{b}\n" for b in BIN_NAMES for n in F.BINS_OF[b]))
    with open(tmp / "p.bed", "w") as f:
        for n in names:
            rows = []
            for code in H.CODES:
                r = records.get((n, code))
                if r is not None:
                    rows += [(pos, chr(st), code, nv, nm, nd) for pos, st, nv, nm, nd in
                             zip(r["position"].tolist(), r["strand"].tolist(), r["n_valid"].tolist(), r["n_mod"].tolist(), r["n_diff"].tolist())]
            rows.sort()
            f.write("".join(f"{n}\t{pos}\t{pos + 1}\t{code}\t{nv}\t{st}\t{pos}\t{pos + 1}\t255,0,0\t{nv}\t{100.0 * nm / nv if nv else 0.0:.2f}\t{nm}\t{nv - nm}\t0\t0\t0\t{nd}\t0\n"
                            for pos, st, code, nv, nm, nd in rows))
    with open(tmp / "bin-motifs.tsv", "w") as f:
        f.write(HEAD + "".join(f"{b}\t{m}\t{pos}\t{code}\t1\t1\tx\t\t\t\t\n" for m, code, pos, b in cands))


def _command(tmp, out, more=()):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "nanomotif_amd", "motif_pileup", "a.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "bin-motifs.tsv", "--out", out,
           "--min_valid_read_coverage", str(H.MIN_COV), "--min_valid_cov_to_diff_fraction", str(H.MIN_FRAC)]
    return subprocess.run(cmd + list(more), cwd=tmp, env=env, capture_output=True, text=True, timeout=600)


def test_the_command_writes_the_brute_force(geo, tmp_path):
    """A fresh process on the geometry input as files, the candidate list once each (a bin-motifs.tsv names a candidate once) plus one of a
    mod type the pileup lacks and one of a bin the assembly lacks."""
    from nanomotif_amd import motif_pileup as mp
    from nanomotif_amd.motif_sites import SiteCandidate
    names, seqs, records = geo["names"], geo["seqs"], geo["records"]
    cands = list(dict.fromkeys(geo["cands"]))
    assert len(cands) < len(geo["cands"]) and P.EMPTY in cands
    _write_input(tmp_path, names, seqs, records, cands[:5] + [("GATC", "21839", 3, "b0"), ("GATC", "a", 1, "nowhere")] + cands[5:])
    rec = P.brute_records(names, seqs, records, F.BINS_OF, cands)
    tables = P.count_table(rec, names, F.BINS_OF, cands)
    summary = []
    for k, (c, t) in enumerate(zip(cands, tables)):
        mine = rec[rec["candidate"] == k]
        for i, n in enumerate(F.BINS_OF[c[3]]):
            here = mine[mine["contig"] == names.index(n)]
            summary.append((SiteCandidate(c[3], c[0], c[1], c[2]), n, t[i], int(here["n_valid"].sum()), int(here["n_mod"].sum())))
    want_summary = mp.format_summary(summary)
    assert len(want_summary.splitlines()) > 100                          # a row per (candidate, contig that holds an occurrence)
    for out, more, select in (("all", ["--all_occurrences"], ("site", "bare")), ("sites", [], ("site",))):
        r = _command(tmp_path, out, more)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "the pileup holds no rows of mod type 21839" in r.stdout and "the bin has no contig in the assembly" in r.stdout
        assert open(tmp_path / out / mp.BED_NAME).read() == P.bed_text(P.selected(rec, select), cands, names), out
        assert open(tmp_path / out / mp.SUMMARY_NAME).read() == want_summary, out
        assert os.path.exists(tmp_path / out / "logs" / "timings.motif_pileup.json")
