"""nm_motif_fractions_count (csrc/nmfractions.hip), ``ScanEngine.motif_fractions`` and the ``motif_fractions`` command against the brute
force of tests/test_motif_fractions_host.py on the geometry input of tests/test_read_methylation_host.py: every comparison is equality and
no row is left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_motif_fractions_host as F
import test_read_methylation_host as H
from nanomotif_amd import synth
from nanomotif_amd.motif import Motif, iupac_to_regex
from test_gpu_motif_compare import reach_class

pytestmark = pytest.mark.gpu
NM_EINVAL, NM_ESTATE, NM_ERANGE = -1, -3, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_NAMES = list(F.BINS_OF)
ALL_B = (2, 3, 20, 64)


def candidates():
    """[(IUPAC motif, code, mod position, bin)] from ``H.request()``: the two one-letter backgrounds and the first motif of every (code,
    reach class 1 or 2) in every bin; the other motifs of those classes, GATC, CCWGG and every fifth of the reach-0 motifs (the family around
    GATC, the geometry motifs) dealt round the bins; one candidate twice, GATC_a_1 in all three bins.  Both codes and the three reach
    classes meet in every bin."""
    out, k, first = [], 0, set()
    for i, (m, code, pos) in enumerate(H.request()):
        cls = reach_class(iupac_to_regex(m), pos)
        if (m, code, pos) in F.ONE_LETTER or (cls and (code, cls) not in first):
            out += [(m, code, pos, b) for b in BIN_NAMES]
            first.add((code, cls))
        elif cls or m in ("GATC", "CCWGG") or i % 5 == 0:
            out.append((m, code, pos, BIN_NAMES[k % 3]))
            k += 1
    out.insert(7, out[2])                                                # one candidate twice
    out.append(("GATC", "a", 1, "b0")); out.append(("GATC", "a", 1, "b2"))
    return out


def _columns(order, records, code, perm_seed=None):
    cols = {k: [] for k in ("contig", "position", "strand", "n_valid", "n_mod", "n_diff")}
    for i, name in enumerate(order):
        r = records.get((name, code))
        if r is None:
            continue
        cols["contig"].append(np.full(len(r["position"]), i, np.uint32))
        for k in ("position", "strand", "n_valid", "n_mod", "n_diff"):
            cols[k].append(r[k])
    cat = {k: np.concatenate(v) for k, v in cols.items()}
    if perm_seed is not None:
        perm = np.random.default_rng(perm_seed).permutation(len(cat["contig"]))
        cat = {k: v[perm] for k, v in cat.items()}
    return cat


def _upload(eng, order, records, min_cov=H.MIN_COV, min_frac=H.MIN_FRAC, perm_seed=None, codes=H.CODES):
    from nanomotif_amd.contig_methylation import upload_read_statistics
    for code in codes:
        c = _columns(order, records, code, perm_seed)
        upload_read_statistics(eng, code, c["contig"], c["position"], c["strand"], c["n_valid"], c["n_mod"], c["n_diff"], min_cov, min_frac)


def _engine_candidates(cands):
    return [(Motif(iupac_to_regex(m), pos), code, b) for m, code, pos, b in cands]


def _tables(eng, cands, B, **kw):
    """[(contig names, uint64[n_contigs, 2, B + 3])] of ``ScanEngine.motif_fractions``, with the yielded candidates checked."""
    batch = _engine_candidates(cands)
    got = list(eng.motif_fractions(batch, bins=B, **kw))
    assert len(got) == len(batch) and all(g[0] is c for g, c in zip(got, batch))
    return [(names, table.copy()) for _, names, table in got]


def _assert_tables(got, want, cands, what):
    assert len(got) == len(want) == len(cands)
    for (names, table), w, c in zip(got, want, cands):
        assert names == F.BINS_OF[c[3]], (what, c)
        assert table.dtype == np.uint64 and table.shape == w.shape, (what, c, table.shape, w.shape)
        if not np.array_equal(table, w):
            i = int(np.flatnonzero((table != w).reshape(len(names), -1).any(axis=1))[0])
            raise AssertionError((what, c, names[i], "got", table[i].tolist(), "expected", w[i].tolist()))


@pytest.fixture(scope="module")
def geo():
    """The geometry input resident in three bins with the read statistics of codes a and m uploaded in ascending order; the brute force's
    site values of the candidate list, computed once."""
    from nanomotif_amd.engine import ScanEngine
    names, seqs, records = H.meth_input()
    assert [n for b in BIN_NAMES for n in F.BINS_OF[b]] == names
    eng = ScanEngine(0)
    eng.upload_assembly(names, [seqs[n] for n in names], [b for b in BIN_NAMES for _ in F.BINS_OF[b]], bin_names=BIN_NAMES)
    _upload(eng, names, records)
    cands = candidates()
    values = F.site_values(seqs, records, F.BINS_OF, cands)
    yield dict(eng=eng, names=names, seqs=seqs, records=records, cands=cands, values=values)
    eng.close()


def test_the_candidate_list_covers_what_it_should(geo):
    cands = geo["cands"]
    cls = {(code, reach_class(iupac_to_regex(m), pos), b) for m, code, pos, b in cands}
    assert cls >= {(code, r, b) for code in H.CODES for r in (0, 1, 2) for b in BIN_NAMES}
    assert all((m, code, pos, b) in cands for m, code, pos in F.ONE_LETTER for b in BIN_NAMES)
    assert len(cands) != len(set(cands)) and 35 <= len(cands) <= 70
    assert [c[1] for c in cands[:12]].count("m") not in (0, 12)                              # the codes are interleaved
    assert eng_bin_order(geo) == F.BINS_OF


def eng_bin_order(geo):
    return {b: geo["eng"].bin_contigs(b) for b in BIN_NAMES}


@pytest.mark.parametrize("B", ALL_B)
def test_the_table_equals_the_brute_force(geo, B):
    want = F.table_of(geo["values"], B)
    got = _tables(geo["eng"], geo["cands"], B)
    _assert_tables(got, want, geo["cands"], f"B = {B}")
    assert sum(int(t[:, :, :B].sum()) for _, t in got) > 50_000
    assert any(((t[:, :, B].sum(axis=1) > 0) & (t[:, :, :B].sum(axis=(1, 2)) == 0)).any() for _, t in got)       # occurrences, no site
    if B == 20:                                                                             # groups of one call each, of a few, and one for all
        for limit in (1, 5 * 2 * 23 * 8 * 4, 1 << 30):
            _assert_tables(_tables(geo["eng"], geo["cands"], B, max_bytes=limit), want, geo["cands"], f"max_bytes = {limit}")


def test_the_sums_are_those_of_the_read_methylation_table(geo):
    """Per (candidate, contig): the histogram sums to ``n_motif_obs``, sum_valid / n is ``mean_read_cov`` and sum_mod / sum_valid the
    weighted mean of nm_contig_methylation, bit for bit; a row the table lacks has no site."""
    from nanomotif_amd.contig_methylation import read_methylation_table
    motifs = list(dict.fromkeys(c[:3] for c in geo["cands"]))
    rows = {(r["motif"], r["mod_type"], r["mod_position"], r["contig"]): r for r in read_methylation_table(geo["eng"], motifs, "weighted-mean")}
    seen = 0
    with_sites = sum(int((t[:, :, :20].sum(axis=(1, 2)) > 0).sum()) for t in F.table_of(geo["values"], 20))
    for c, (names, table) in zip(geo["cands"], _tables(geo["eng"], geo["cands"], 20)):
        t = table.astype(np.int64).sum(axis=1)
        for i, name in enumerate(names):
            n, sum_valid, sum_mod = int(t[i, :20].sum()), int(t[i, 21]), int(t[i, 22])
            r = rows.get(c[:3] + (name,))
            if r is None:
                assert n == 0 and sum_valid == 0 and sum_mod == 0, (c, name)
                continue
            seen += 1
            assert n == r["n_motif_obs"] and float(sum_valid) / float(n) == r["mean_read_cov"] and float(sum_mod) / float(sum_valid) == r["methylation_value"], (c, name)
    assert seen == with_sites > 100                                                        # every row of the brute force that holds a site


def test_saturated_histograms_across_a_chunk_border():
    """Two 9 000 bp poly-A contigs (two work items a contig, one row): a kept '+' record on every position, all modified on the first and
    none on the second — every lane adds its 128 sites to one counter, both waves of a contig to one row.  The '-' strand has no T."""
    from nanomotif_amd.engine import ScanEngine
    L = 9_000
    eng = ScanEngine(0)
    eng.upload_assembly(["full", "none"], ["A" * L, "A" * L], ["b", "b"])
    pos = np.arange(L)
    records = {(n, "a"): dict(position=pos, strand=np.full(L, H.PLUS, np.uint8), n_valid=np.full(L, 10), n_mod=np.full(L, m), n_diff=np.zeros(L, np.int64))
               for n, m in (("full", 10), ("none", 0))}
    _upload(eng, ["full", "none"], records, codes=("a",))
    for B in ALL_B:
        ((names, table),) = _tables(eng, [("A", "a", 0, "b")], B)
        want = np.zeros((2, 2, B + 3), dtype=np.uint64)
        want[0, 0, B - 1] = want[1, 0, 0] = L
        want[:, 0, B] = L
        want[:, 0, B + 1] = 10 * L
        want[0, 0, B + 2] = 10 * L
        assert names == ["full", "none"] and np.array_equal(table, want), (B, table.tolist())
    eng.close()


def test_a_reupload_replaces_the_statistics_and_row_order_plays_no_part(geo):
    from nanomotif_amd.engine import ScanEngine
    names, seqs, records = geo["names"], geo["seqs"], geo["records"]
    cands = geo["cands"][::3] + [c for c in geo["cands"] if c[:3] in F.ONE_LETTER]
    eng = ScanEngine(0)
    eng.upload_assembly(names, [seqs[n] for n in names], [b for b in BIN_NAMES for _ in F.BINS_OF[b]], bin_names=BIN_NAMES)
    _upload(eng, names, records, perm_seed=5)
    sub = [geo["values"][geo["cands"].index(c)] for c in cands]
    _assert_tables(_tables(eng, cands, 20), F.table_of(sub, 20), cands, "permuted rows")
    _upload(eng, names, records, min_cov=12, min_frac=0.95, perm_seed=6)
    want = F.expected_table(seqs, records, F.BINS_OF, cands, 20, 12, 0.95)
    assert any(not np.array_equal(a, b) for a, b in zip(want, F.table_of(sub, 20)))
    _assert_tables(_tables(eng, cands, 20), want, cands, "min_cov = 12, min_frac = 0.95")
    eng.close()


def test_every_refusal_returns_its_code_and_leaves_the_engine_usable(geo):
    from nanomotif_amd._lib import NmScanError, check
    from nanomotif_amd.engine import ScanEngine
    eng = geo["eng"]
    cands = geo["cands"][:6]
    want = F.table_of(geo["values"][:6], 20)
    b = eng.make_batch(_engine_candidates(cands), slot_of=lambda mt: ["m", "a", "21839"].index(mt))
    rows = sum(len(F.BINS_OF[c[3]]) for c in cands)

    def call(batch=b, n_bins=20, null=None, ctx=None, n=None):
        out = np.zeros((rows, 2, n_bins + 3 if 2 <= n_bins <= 64 else 70), dtype=np.uint64)
        args = list(eng._batch_args(batch))
        if n is not None:
            args[0] = n
        if null is not None and null != "counts":
            args[null] = None
        check(eng.lib.nm_motif_fractions_count(eng.ctx if ctx is None else ctx, *args, n_bins, None if null == "counts" else out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def still_fine():
        _assert_tables(_tables(eng, cands, 20), want, cands, "after a refusal")

    def refused(code, match, **kw):
        with pytest.raises(NmScanError, match=match) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value)
        still_fine()

    from nanomotif_amd.engine import CandidateBatch
    for n_bins in (0, 1, 65, 1 << 20):
        refused(NM_EINVAL, "n_bins", n_bins=n_bins)
    for null in (1, 2, 3, 4, 5, 6, "counts"):
        refused(NM_EINVAL, "NULL", null=null)
    bad_bin = CandidateBatch(np.where(np.arange(len(b)) == 3, len(BIN_NAMES), b.bins).astype(np.uint32), b.slots, b.lens, b.modpos, b.offsets, b.masks)
    refused(NM_EINVAL, "candidate 3: cand_bin 3 >= n_bins 3", batch=bad_bin)
    for slot in (2, 7, 8, 255):                                                             # 21839 has no statistics; 8 and 255 are no slots
        no_stats = CandidateBatch(b.bins, np.where(np.arange(len(b)) == 1, slot, b.slots).astype(np.uint8), b.lens, b.modpos, b.offsets, b.masks)
        refused(NM_ESTATE, f"candidate 1: read-statistics slot {slot} holds no pileup", batch=no_stats)
    wide = eng.make_batch([(Motif("A" + "." * 96 + "T", 0), "a", "b0")], slot_of=lambda mt: 1)
    with pytest.raises(NmScanError) as e:                                                  # a reach of 97: compile_program's refusal
        check(eng.lib.nm_motif_fractions_count(eng.ctx, *eng._batch_args(wide), 20, np.zeros((1, 2, 23), np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))))
    assert e.value.code == NM_ERANGE
    still_fine()
    assert np.array_equal(call(n=0), np.zeros((rows, 2, 23), np.uint64))                   # n_cand = 0: NM_OK, nothing written
    assert eng.lib.nm_motif_fractions_count(eng.ctx, 0, None, None, None, None, None, None, 20, None) == 0
    got = call().reshape(-1, 2, 23)                                                         # the plain call: the rows back to back
    assert np.array_equal(got, np.concatenate(want))
    # the engine's own refusals: a mod code without statistics and a number of bins out of range, before the library is called
    with pytest.raises(ValueError, match="no read statistics are resident for mod type.s. 21839"):
        eng.motif_fractions([(Motif("GATC", 1), "21839", "b0")])
    for bins in (1, 65):
        with pytest.raises(ValueError, match="bins"):
            eng.motif_fractions(_engine_candidates(cands), bins=bins)
    still_fine()
    # no assembly, and an assembly without statistics
    fresh = ScanEngine(0)
    with pytest.raises(NmScanError) as e:
        check(fresh.lib.nm_motif_fractions_count(fresh.ctx, *eng._batch_args(b), 20, np.zeros((rows, 2, 23), np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))))
    assert e.value.code == NM_ESTATE and "nm_upload_contigs" in str(e.value)
    fresh.upload_assembly(["c"], ["GATC" * 10], ["b0"], bin_names=BIN_NAMES)
    assert fresh.readstats_mods == set()
    with pytest.raises(ValueError, match="resident: none"):
        fresh.motif_fractions([(Motif("GATC", 1), "a", "b0")])
    fresh.close()
    still_fine()


# ------------------------------------------------------------------------------------------------ the command
HEAD = "reference\tmotif\tmod_position\tmod_type\tn_mod\tn_nomod\tmotif_type\tmotif_complement\tmod_position_complement\tn_mod_complement\tn_nomod_complement\n"
COMMAND_CANDS = [("GATC", "a", 1), ("CCWGG", "m", 1), ("GATC", "21839", 3), ("A" + "N" * 40 + "C", "a", 0), ("GATC", "m", 3)]
FILES = ("motif-fractions.tsv", "motif-fractions-contigs.tsv", "motif-fractions-hist.tsv")


def _command(tmp, extra_env=None, out="fr", more=()):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **(extra_env or {}))
    cmd = [sys.executable, "-m", "nanomotif_amd", "motif_fractions", "a.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "bin-motifs.tsv", "--out", out]
    return subprocess.run(cmd + list(more), cwd=tmp, env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def command_files(tmp_path_factory):
    """Two contigs of 160 kbp in one bin as files, and the text the brute force expects of the command at its defaults (20 bins,
    coverage 5, ratio 0.8, edges 6 / 14)."""
    from nanomotif_amd import motif_fractions as mf
    from nanomotif_amd.motif_sites import SiteCandidate
    tmp = tmp_path_factory.mktemp("fractions")
    spec = synth.SynthSpec(n_contigs=2, total_bp=160_000, n_bins=1, mod_types=("a", "m"), seed=43, min_contig_bp=60_000, fixed_motifs=(("GATC", 1, "a"),))
    mg = synth.make_metagenome(spec)
    mg.write_fasta(str(tmp / "a.fasta"))
    mg.write_bed(str(tmp / "p.bed"))
    mg.write_contig_bin(str(tmp / "cb.tsv"))
    with open(tmp / "p.bed", "a") as f:                                  # a contig the bins do not hold: ignored
        f.write("stranger\t7\t8\ta\t9\t+\t7\t8\t255,0,0\t9\t50.00\t4\t5\t0\t0\t0\t0\t0\n")
    bin_name = mg.bin_names[0]
    with open(tmp / "bin-motifs.tsv", "w") as f:
        f.write(HEAD + "".join(f"{bin_name}\t{m}\t{pos}\t{code}\t1\t1\tx\t\t\t\t\n" for m, code, pos in COMMAND_CANDS))
    seqs, rec = {}, {}
    for i, name in enumerate(mg.names):
        seqs[name] = mg.contig_str(i)
        for mt in ("a", "m"):
            p = mg.contig_pileup(i, mt)
            cov = p["nvalid"].astype(np.int64)
            rec[(name, mt)] = dict(position=p["position"].astype(np.int64), strand=p["strand"], n_valid=cov,
                                   n_mod=np.array([int(round(c * h / 10000)) for c, h in zip(cov.tolist(), p["pct_hundredths"].tolist())], np.int64),
                                   n_diff=np.zeros(len(cov), np.int64))
    known = [c for c in COMMAND_CANDS if c[1] != "21839"]
    bins_of = {bin_name: list(mg.names)}
    bg = [("A", "a", 0, bin_name), ("C", "m", 0, bin_name)]
    tables = F.expected_table(seqs, rec, bins_of, bg + [c + (bin_name,) for c in known], 20, 5, 0.8)
    names = list(mg.names)
    texts = mf.format_files([SiteCandidate(bin_name, m, code, pos) for m, code, pos in known], [(names, t) for t in tables[2:]],
                            [((bin_name, "a"), tables[0]), ((bin_name, "m"), tables[1])], 20, 6, 14, 20, 0.1)
    assert len(texts[0].splitlines()) == 1 + len(known) and int(tables[2][:, :, :20].sum()) > 200
    return tmp, texts


def test_the_command_writes_the_brute_force_on_either_parser(command_files):
    tmp, texts = command_files
    r = _command(tmp)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "the pileup holds no rows of mod type 21839" in r.stdout and "skipped" in r.stdout
    assert "read statistics from the device parser's columns" in r.stdout
    for name, text in zip(FILES, texts):
        assert open(tmp / "fr" / name).read() == text, name
    assert os.path.exists(tmp / "fr" / "logs" / "timings.motif_fractions.json")
    r = _command(tmp, {"NANOMOTIF_HOST_PARSER": "1"}, out="fr_host")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "read statistics from the host parser's rows" in r.stdout
    for name in FILES:
        assert open(tmp / "fr_host" / name, "rb").read() == open(tmp / "fr" / name, "rb").read(), name


def test_the_command_refuses_a_multi_rank_launch_and_bad_edges(command_files):
    tmp, _ = command_files
    r = _command(tmp, {"WORLD_SIZE": "2", "RANK": "0"}, out="fr_ranks")
    assert r.returncode == 2 and "one GPU" in r.stdout + r.stderr and not os.path.exists(tmp / "fr_ranks" / FILES[0])
    r = _command(tmp, out="fr_edges", more=["--bins", "2", "--methylation_threshold_low", "0.2"])
    assert r.returncode == 2 and "bin edges 0 / 1 of 2" in r.stdout + r.stderr and not os.path.exists(tmp / "fr_edges" / FILES[0])
