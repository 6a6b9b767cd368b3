"""nm_readstats_upload / nm_contig_methylation (csrc/nmmeth.hip) and nanomotif_amd.contig_methylation: the per-contig READ
methylation table binnary starts from (nanomotif/main.py:142-193) against oracle/contig_methylation.read_methylation
(restated from epimetheus' published behaviour — parity unpinned there; the product is pinned to the restatement)."""
import numpy as np
import pytest

import test_read_methylation_host as H                                  # the brute force and the geometry input of the border tests
from nanomotif_amd import synth
from nanomotif_amd.motif import iupac_to_regex

pytestmark = pytest.mark.gpu

ZOO = ["GATC_a_1", "CCWGG_m_1", "A_a_0", "C_m_0", "GAAGNNNNNTAC_a_2", "GATC_m_3", "AA_a_0", "AA_a_1", "GCGC_m_1", "TTAA_a_2", "RGATCY_a_2",
       "G" + "N" * 35 + "AT_a_36", "CNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNG_m_0", "ACCCA_a_4", "GGCC_m_3", "VCB_m_1",
       "T" + "N" * 70 + "A_a_71", "C" + "N" * 90 + "G_m_0"]       # more than 63 positions from the modified base: the three-halo-word kernels


def _records(mg, rng):
    """{(contig, mod_type): columns} with N_mod consistent with the synthetic percentages and an N_diff column that makes
    the valid-to-diff filter bite on ~10 % of the records."""
    rec = {}
    for i, name in enumerate(mg.names):
        for mt in mg.spec.mod_types:
            p = mg.contig_pileup(i, mt)
            cov = p["nvalid"].astype(np.int64)
            nmod = np.rint(cov * p["pct_hundredths"] / 10000).astype(np.int64)
            ndiff = np.where(rng.random(len(cov)) < 0.1, rng.integers(0, 12, len(cov)), 0).astype(np.int64)
            ndiff[cov == 4] = 1                                     # 4 / 5 = 0.8 exactly: kept
            rec[(name, mt)] = dict(position=p["position"].astype(np.int64), strand=p["strand"], n_valid=cov, n_mod=nmod, n_diff=ndiff)
    return rec


def _upload(eng, mg, rec, min_cov=3, min_frac=0.8, shard=None):
    from nanomotif_amd.contig_methylation import upload_read_statistics
    kept = {}
    for mt in mg.spec.mod_types:
        cols = {k: [] for k in ("contig", "position", "strand", "n_valid", "n_mod", "n_diff")}
        for i, name in enumerate(mg.names):
            r = rec[(name, mt)]
            local = i if shard is None else shard.get(i, 0xFFFFFFFF)
            cols["contig"].append(np.full(len(r["position"]), local, np.uint32))
            for k in ("position", "strand", "n_valid", "n_mod", "n_diff"):
                cols[k].append(r[k])
        cat = {k: np.concatenate(v) for k, v in cols.items()}
        kept[mt] = upload_read_statistics(eng, mt, cat["contig"], cat["position"], cat["strand"], cat["n_valid"], cat["n_mod"], cat["n_diff"],
                                          min_cov, min_frac)
    return kept


def _oracle_rows(mg, rec, motifs, output_type, min_cov=3, min_frac=0.8, contigs=None):
    from nanomotif_amd.contig_methylation import parse_motif_mod
    from oracle.contig_methylation import read_methylation
    triples = [parse_motif_mod(m) for m in motifs]
    idx = range(len(mg.names)) if contigs is None else contigs
    seqs = {mg.names[i]: mg.contig_str(i) for i in idx}
    rows = read_methylation(rec, seqs, [(iupac_to_regex(m), mt, pos) for m, mt, pos in triples], min_cov, min_frac, output_type)
    return [(r["contig"], triples[r["motif"]][0], triples[r["motif"]][1], triples[r["motif"]][2], r["methylation_value"], r["mean_read_cov"],
             r["n_motif_obs"]) for r in rows]


def test_read_methylation_table_equals_the_oracle():
    from nanomotif_amd.contig_methylation import COLUMNS, read_methylation_table
    from nanomotif_amd.engine import ScanEngine
    spec = synth.SynthSpec(n_contigs=9, total_bp=700_000, n_bins=3, mod_types=("a", "m"), seed=41, min_contig_bp=9_000,
                           fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m"), ("GAAGNNNNNTAC", 2, "a")))
    mg = synth.make_metagenome(spec)
    rec = _records(mg, np.random.default_rng(3))
    eng = ScanEngine(0)
    eng.upload_assembly(mg.names, [mg.contig_ascii(i) for i in range(len(mg.names))], mg.bin_names)
    kept = _upload(eng, mg, rec)
    for mt in ("a", "m"):
        want = sum(int(((r["n_valid"] >= 3) & (r["n_valid"] / (r["n_valid"] + r["n_diff"]) >= 0.8)).sum()) for (n, m), r in rec.items() if m == mt)
        assert kept[mt] == want and 0 < want < sum(len(r["position"]) for (n, m), r in rec.items() if m == mt)
    for output_type in ("median", "weighted-mean"):
        rows = read_methylation_table(eng, ZOO, output_type)
        assert rows and list(rows[0]) == COLUMNS
        got = [tuple(r[c] for c in COLUMNS) for r in rows]
        want = _oracle_rows(mg, rec, ZOO, output_type)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g == w, (output_type, g, w)                      # counts, means, medians: bit-exact doubles
    planted = {(r["contig"], r["motif"]): r for r in read_methylation_table(eng, ["GATC_a_1", "CCWGG_m_1"], "median")}
    hit = [planted[(n, "GATC")]["methylation_value"] for n, b in zip(mg.names, mg.bin_names) if ("GATC", 1, "a") in mg.bin_motifs[b] and (n, "GATC") in planted]
    assert hit and min(hit) > 0.8
    # main.py:193: n_motif_obs * mean_read_cov >= --methylation_threshold (default 24)
    kept_rows = read_methylation_table(eng, ZOO, "median", methylation_threshold=24)
    assert [r for r in read_methylation_table(eng, ZOO, "median") if r["n_motif_obs"] * r["mean_read_cov"] >= 24] == kept_rows
    # other read filters: a re-upload replaces the slot
    _upload(eng, mg, rec, min_cov=12, min_frac=0.95)
    got = [tuple(r[c] for c in COLUMNS) for r in read_methylation_table(eng, ZOO[:6], "median")]
    assert got == _oracle_rows(mg, rec, ZOO[:6], "median", 12, 0.95)
    # a shard (multi-GPU: contigs of other ranks carry 0xFFFFFFFF) reports its own contigs only
    eng2 = ScanEngine(0)
    mine = [1, 4, 6]
    eng2.upload_assembly([mg.names[i] for i in mine], [mg.contig_ascii(i) for i in mine], [mg.bin_names[i] for i in mine])
    _upload(eng2, mg, rec, shard={g: k for k, g in enumerate(mine)})
    got = [tuple(r[c] for c in COLUMNS) for r in read_methylation_table(eng2, ZOO, "weighted-mean")]
    assert got == _oracle_rows(mg, rec, ZOO, "weighted-mean", contigs=mine)
    eng.close(); eng2.close()


def test_methylation_pattern_from_files_and_error_paths(tmp_path):
    """The drop-in for main.py:167-178: FASTA + bedMethyl text in, motifs-scored-read-methylation_<type>.tsv out; the shape
    of the reference's own check (tests/binnary/test_utils.py:38-59: GATC_m_3 and GATC_a_1 on two contigs -> 4 rows, 7 columns)."""
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.contig_methylation import COLUMNS, methylation_pattern, upload_read_statistics
    from nanomotif_amd.engine import ScanEngine
    spec = synth.SynthSpec(n_contigs=2, total_bp=160_000, n_bins=1, mod_types=("a", "m"), seed=43, min_contig_bp=60_000,
                           fixed_motifs=(("GATC", 1, "a"),))
    mg = synth.make_metagenome(spec)
    mg.write_fasta(str(tmp_path / "a.fasta"))
    mg.write_bed(str(tmp_path / "p.bed"))
    with open(tmp_path / "p.bed", "a") as f:                      # a contig the assembly does not have: ignored (allow_assembly_pileup_mismatch)
        f.write("stranger\t7\t8\ta\t9\t+\t7\t8\t255,0,0\t9\t50.00\t4\t5\t0\t0\t0\t0\t0\n")
    rec = {}
    for i, name in enumerate(mg.names):
        for mt in ("a", "m"):
            p = mg.contig_pileup(i, mt)
            cov = p["nvalid"].astype(np.int64)
            rec[(name, mt)] = dict(position=p["position"].astype(np.int64), strand=p["strand"], n_valid=cov,
                                   n_mod=np.array([int(round(c * h / 10000)) for c, h in zip(cov.tolist(), p["pct_hundredths"].tolist())], np.int64),
                                   n_diff=np.zeros(len(cov), np.int64))
    motifs = ["GATC_m_3", "GATC_a_1"]
    for output_type in ("median", "weighted-mean"):
        out = tmp_path / f"motifs-scored-read-methylation_{output_type}.tsv"
        rows = methylation_pattern(str(tmp_path / "p.bed"), str(tmp_path / "a.fasta"), motifs, threads=2, min_valid_read_coverage=3,
                                   min_valid_cov_to_diff_fraction=0.8, output=str(out), output_type=output_type)
        want = _oracle_rows(mg, rec, motifs, output_type)
        assert [tuple(r[c] for c in COLUMNS) for r in rows] == want and len(rows) == 4
        text = out.read_text().splitlines()
        assert text[0].split("\t") == ['contig', 'motif', 'mod_type', 'mod_position', 'methylation_value', 'mean_read_cov', 'n_motif_obs']
        assert len(text) == 5
        back = [ln.split("\t") for ln in text[1:]]
        assert [(b[0], b[1], b[2], int(b[3]), float(b[4]), float(b[5]), int(b[6])) for b in back] == want      # repr round-trips doubles
    with pytest.raises(ValueError, match="not in the assembly"):
        methylation_pattern(str(tmp_path / "p.bed"), str(tmp_path / "a.fasta"), motifs, allow_assembly_pileup_mismatch=False)
    with pytest.raises(ValueError, match="median or weighted-mean"):
        methylation_pattern(str(tmp_path / "p.bed"), str(tmp_path / "a.fasta"), motifs, output_type="mean")
    eng = ScanEngine(0)
    eng.upload_assembly(["c"], ["ACGATCGATCGGATCCA" * 10], ["b"])
    from nanomotif_amd.contig_methylation import read_methylation_table
    with pytest.raises(NmScanError, match="holds no pileup"):
        read_methylation_table(eng, ["GATC_a_1"])
    one = dict(contig_local=[0, 0], position=[3, 3], strand=np.frombuffer(b"++", np.uint8), n_valid_cov=[9, 9], n_modified=[4, 5])
    with pytest.raises(NmScanError, match="duplicate"):
        upload_read_statistics(eng, "a", **one)
    with pytest.raises(NmScanError, match="holds no pileup"):          # the failed upload left no half-built slot behind
        read_methylation_table(eng, ["GATC_a_1"])
    with pytest.raises(NmScanError, match="n_modified outside"):
        upload_read_statistics(eng, "a", [0], [3], np.frombuffer(b"+", np.uint8), [9], [10])
    assert upload_read_statistics(eng, "a", [0, 0], [3, 7], np.frombuffer(b"++", np.uint8), [9, 2], [4, 1]) == 1     # coverage 2 < 3
    rows = read_methylation_table(eng, ["GATC_a_1", "GATC_a_1"])      # duplicates collapse (.unique(), main.py:133)
    assert rows == [dict(contig="c", motif="GATC", mod_type="a", mod_position=1, methylation_value=4 / 9, mean_read_cov=9.0, n_motif_obs=1)]
    assert upload_read_statistics(eng, "a", [], [], np.zeros(0, np.uint8), [], []) == 0
    assert read_methylation_table(eng, ["GATC_a_1"]) == []
    eng.close()


# ------------------------------------------------------------------------------------------------ rank, lane and batch borders
# The brute force, the geometry input and the request are tests/test_read_methylation_host.py's; every comparison is equality.
def _columns(order, records, code, perm_seed=None, swap=False):
    """The flat upload of one code: contigs numbered by their place in ``order``, rows ascending per contig or under a fixed permutation."""
    cols = {k: [] for k in ("contig", "position", "strand", "n_valid", "n_mod", "n_diff")}
    for i, name in enumerate(order):
        r = records.get((name, code))
        if r is None:
            continue
        cols["contig"].append(np.full(len(r["position"]), i, np.uint32))
        for k in ("position", "strand", "n_valid", "n_mod", "n_diff"):
            cols[k].append(r[k])
    cat = {k: np.concatenate(v) for k, v in cols.items()}
    if swap:
        cat["strand"] = np.where(cat["strand"] == ord("+"), ord("-"), ord("+")).astype(np.uint8)
    if perm_seed is not None:
        perm = np.random.default_rng(perm_seed).permutation(len(cat["contig"]))
        assert (np.diff(cat["position"][perm]) < 0).any()
        cat = {k: v[perm] for k, v in cat.items()}
    return cat


def _engine(order, seqs, records, codes=("a", "m"), perm_seed=None, use_diff=True, swap=False):
    """-> (engine with ``order`` resident and the records of ``codes`` in their slots, {code: n_kept})."""
    from nanomotif_amd.contig_methylation import upload_read_statistics
    from nanomotif_amd.engine import ScanEngine
    eng = ScanEngine(0)
    eng.upload_assembly(order, [seqs[n] for n in order], ["b"] * len(order))
    kept = {}
    for code in codes:
        c = _columns(order, records, code, perm_seed, swap)
        kept[code] = upload_read_statistics(eng, code, c["contig"], c["position"], c["strand"], c["n_valid"], c["n_mod"],
                                            c["n_diff"] if use_diff else None, H.MIN_COV, H.MIN_FRAC)
    return eng, kept


def _table(eng, names, output_type="median"):
    from nanomotif_amd.contig_methylation import COLUMNS, read_methylation_table
    return [tuple(r[c] for c in COLUMNS) for r in read_methylation_table(eng, names, output_type)]


def _rows_for(table, names):
    """The rows of ``table`` that belong to ``names``, in the order of ``names`` (contigs keep their order within a motif)."""
    by = {}
    for r in table:
        by.setdefault(r[1:4], []).append(r)
    return [r for n in dict.fromkeys(names) for r in by.get(tuple(n), [])]


def _assert_rows(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for g, w in zip(got, want):
        assert g == w, (what, "got", g, "expected", w)


@pytest.fixture(scope="module")
def geo():
    """The geometry input resident with its rows uploaded in ascending order, and the device's whole table of the interleaved request for
    both output types: computed once, read by the tests below."""
    names, seqs, records = H.meth_input()
    eng, kept = _engine(names, seqs, records)
    req = H.request()
    tables = {ot: _table(eng, req, ot) for ot in ("median", "weighted-mean")}
    yield dict(eng=eng, kept=kept, tables=tables, names=names, seqs=seqs, records=records, req=req)
    eng.close()


LITERAL = dict(position=[1, 2, 5, 6, 9, 3, 157], strand=np.frombuffer(b"+-+-+++", np.uint8), n_valid=[10, 5, 8, 2, 8, 9, 30],
               n_mod=[4, 5, 2, 1, 8, 9, 3], n_diff=[0, 0, 2, 0, 3, 0, 0])


def test_literal_case_by_hand():
    """One contig ``"GATC" * 40``: the '+' A of site k sits at 4 k + 1, its '-' A at 4 k + 2.  Records (position strand coverage modified diff):
        1 + 10 4 0    kept, 0.4           |  2 - 5 5 0    kept, 1.0: the other strand of the same site
        5 + 8 2 2     kept, 0.25: 8 / (8 + 2) = 0.8 exactly
        6 - 2 1 0     dropped: coverage 2 < 3         |  9 + 8 8 3    dropped: 8 / (8 + 3) < 0.8
        3 + 9 9 0     kept, on a C: no site of GATC_a_1       |  157 + 30 3 0    kept, 0.1: the '+' A of the last site
    n_kept = 5; GATC_a_1: 4 sites, coverage 10 + 5 + 8 + 30 = 53, fractions 0.1 0.25 0.4 1.0, modified 4 + 5 + 2 + 3 = 14."""
    from nanomotif_amd.contig_methylation import upload_read_statistics
    from nanomotif_amd.engine import ScanEngine
    eng = ScanEngine(0)
    eng.upload_assembly(["c"], ["GATC" * 40], ["b"])
    assert upload_read_statistics(eng, "a", [0] * 7, LITERAL["position"], LITERAL["strand"], LITERAL["n_valid"], LITERAL["n_mod"], LITERAL["n_diff"], 3, 0.8) == 5
    assert _table(eng, ["GATC_a_1"], "median") == [("c", "GATC", "a", 1, (0.25 + 0.4) / 2.0, 53 / 4, 4)]
    assert _table(eng, ["GATC_a_1"], "weighted-mean") == [("c", "GATC", "a", 1, 14 / 53, 13.25, 4)]
    assert _table(eng, ["C_a_0"], "median") == [("c", "C", "a", 0, 1.0, 9.0, 1)]
    # without the ratio filter the record at 9 is kept as well
    assert upload_read_statistics(eng, "a", [0] * 7, LITERAL["position"], LITERAL["strand"], LITERAL["n_valid"], LITERAL["n_mod"], None, 3, 0.8) == 6
    assert _table(eng, ["GATC_a_1"], "median") == [("c", "GATC", "a", 1, 0.4, 61 / 5, 5)]
    eng.close()


def test_geometry_equals_the_brute_force(geo):
    """The whole table of the interleaved request (19 geometry motifs, 80 reach-0 motifs around one A: three batches of one group, six
    motifs of a second code), both output types, row for row and bit for bit; the same from rows uploaded under a fixed random
    permutation; the same without the n_diff column against the brute force without the ratio filter."""
    seqs, records, req = geo["seqs"], geo["records"], geo["req"]
    assert geo["kept"] == {c: H.n_kept_of(records, c) for c in ("a", "m")}
    for ot in ("median", "weighted-mean"):
        _assert_rows(geo["tables"][ot], H.rows_of(H.expected(), seqs, req, ot), ot)
    eng, kept = _engine(geo["names"], seqs, records, perm_seed=5)
    assert kept == geo["kept"]
    for ot in ("median", "weighted-mean"):
        _assert_rows(_table(eng, req, ot), geo["tables"][ot], ("permuted rows", ot))
    eng.close()
    eng, kept = _engine(geo["names"], seqs, records, use_diff=False)
    assert kept == {c: H.n_kept_of(records, c, use_diff=False) for c in ("a", "m")} and kept["a"] > geo["kept"]["a"]
    for ot in ("median", "weighted-mean"):
        _assert_rows(_table(eng, req, ot), H.rows_of(H.expected(False), seqs, req, ot), ("no n_diff", ot))
    eng.close()


def test_batch_borders(geo):
    """31, 32, 33, 64 and 65 motifs of one (code, reach) group alone, the whole request reversed and with duplicates: always the rows
    of the whole table."""
    eng, table = geo["eng"], geo["tables"]["median"]
    for n in (31, 32, 33, 64, 65):
        names = H.FAMILY[:n]
        _assert_rows(_table(eng, names), _rows_for(table, names), n)
        assert len({r[1:4] for r in _rows_for(table, names)}) == n
    back = geo["req"][::-1]
    _assert_rows(_table(eng, back), _rows_for(table, back), "reversed")
    _assert_rows(_table(eng, back, "weighted-mean"), _rows_for(geo["tables"]["weighted-mean"], back), "reversed")
    assert [r[1:4] for r in _table(eng, back)][0] == tuple(back[0]) != tuple(geo["req"][0])
    twice = geo["req"][:40] + geo["req"][5:70] + geo["req"]
    _assert_rows(_table(eng, twice), table, "duplicates")
    strings = [f"{m}_{c}_{p}" for m, c, p in H.FAMILY[:33]]              # the motif_mod strings binnary passes
    _assert_rows(_table(eng, strings + strings[:3]), _rows_for(table, H.FAMILY[:33]), "strings")


def test_identities_on_the_device_results(geo):
    """(i) the one-letter motifs partition the kept records that sit on a base; (ii) mean_read_cov is the correctly rounded
    coverage sum / n_motif_obs (and times n_motif_obs rounds back to the sum: (a / n) * n itself need not be an integer in
    doubles, so the exact statement is the division); (iii) a motif reads on '+' what its reverse complement with the mirrored mod
    position reads on '-': identical rows once the records' strands are exchanged; (iv) the contigs in reversed order give the
    same rows per contig name."""
    from nanomotif_amd.motif import reverse_compliment
    eng, seqs, records, req, names = geo["eng"], geo["seqs"], geo["records"], geo["req"], geo["names"]
    one = _table(eng, ["A_a_0", "C_a_0", "G_a_0", "T_a_0"])
    on_n = H.kept_on_n(seqs, records, "a")
    assert on_n > 0 and sum(r[6] for r in one) == geo["kept"]["a"] - on_n
    assert ("long", "T", "a", 0) in {r[:4] for r in one}
    exp = H.expected()
    index = {tuple(n): k for k, n in enumerate(req)}
    for r in geo["tables"]["median"]:
        g = exp[(index[r[1:4]], r[0])]
        assert r[5] == g.cov_sum / r[6] and round(r[5] * r[6]) == g.cov_sum, (r, g.cov_sum)
    # (iii)
    pick = [("GAAG", "a", 1), ("A" + "N" * 40 + "C", "a", 0), ("RGATC", "a", 2), ("A" + "N" * 70 + "T", "a", 0), ("CCWGG", "m", 1), ("AGATCS", "a", 2)]
    mirror = [(reverse_compliment(m), c, len(m) - 1 - p) for m, c, p in pick]
    assert mirror[0] == ("CTTC", "a", 2) and mirror[2] == ("GATCY", "a", 2)
    own = _table(eng, pick)
    eng2, kept = _engine(names, seqs, records, swap=True)
    assert kept == geo["kept"]
    other = _table(eng2, mirror)
    assert len(own) >= 30 and [(r[0], r[2]) + r[4:] for r in own] == [(r[0], r[2]) + r[4:] for r in other]
    assert [r[4:] for r in _table(eng, mirror)] != [r[4:] for r in other]                          # not so without the exchange
    eng2.close()
    # (iv)
    back = names[::-1]
    eng3, kept = _engine(back, seqs, records)
    assert kept == geo["kept"]
    got = _table(eng3, req)
    eng3.close()
    assert [r[0] for r in got[:3]] != [r[0] for r in geo["tables"]["median"][:3]]
    place = {n: i for i, n in enumerate(back)}
    want = sorted(geo["tables"]["median"], key=lambda r: (index[r[1:4]], place[r[0]]))
    _assert_rows(got, want, "reversed contigs")


def test_key_budget_switch_halves_batches(geo):
    """NM_METH_MAX_KEYS (read at every call): at 1000 the batches of the whole request split down to what fits, at 1 down to single
    motifs (which proceed: the refusal needs 2^32 - 1 sites as well); unparsable values are the built-in budget.  Always the same table."""
    import os
    eng, req = geo["eng"], geo["req"]
    n_sites = sum(r[6] for r in geo["tables"]["median"])
    assert n_sites > 100 * 1000 and max(r[6] for r in geo["tables"]["median"]) > 1000       # both budgets are exceeded many times over
    for value in ("1000", "1", "0", "-3", "many", ""):
        os.environ["NM_METH_MAX_KEYS"] = value
        try:
            got = {ot: _table(eng, req, ot) for ot in ("median", "weighted-mean")}
        finally:
            del os.environ["NM_METH_MAX_KEYS"]
        for ot in got:
            _assert_rows(got[ot], geo["tables"][ot], (value, ot))
    _assert_rows(_table(eng, req), geo["tables"]["median"], "unset again")


def _write_bed(path, rows):
    """rows: (contig, position, strand char, code, n_valid, n_mod, n_diff) -> modkit bedMethyl, 18 columns."""
    with open(path, "w") as f:
        for name, pos, st, code, cov, mod, diff in rows:
            pct = "%.2f" % (100.0 * mod / cov)
            f.write(f"{name}\t{pos}\t{pos + 1}\t{code}\t{cov}\t{st}\t{pos}\t{pos + 1}\t255,0,0\t{cov}\t{pct}\t{mod}\t{cov - mod}\t0\t0\t0\t{diff}\t0\n")


def test_two_codes_on_one_position_through_the_parsers(tmp_path, monkeypatch, caplog):
    """modkit writes ``m`` and ``21839`` rows for the same C: both sit on one (contig, position, strand) with their own counts.  Through
    methylation_pattern on the device parser's columns (nm_readstats_upload_bedcols skips the rows of other codes before the duplicate
    check) and on the host reader's rows: the brute force per code, no duplicate error; a true duplicate within one code is refused."""
    import logging
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.contig_methylation import COLUMNS, methylation_pattern
    rng = np.random.default_rng(11)
    seqs = {"c1": "".join(rng.choice(list("ACGT"), size=3000)), "c2": "CCAGG" * 30 + "".join(rng.choice(list("ACGT"), size=1200)) + "GATC"}
    with open(tmp_path / "a.fasta", "w") as f:
        for n, s in seqs.items():
            f.write(f">{n}\n{s}\n")
    rows, rec = [], {}
    for name, seq in seqs.items():
        for pos, base in enumerate(seq):
            for st, canon in (("+", base), ("-", base.translate(str.maketrans("ACGT", "TGCA")))):
                if canon == "C" and rng.random() < 0.6:
                    cov = int(rng.integers(1, 25))
                    nm = int(rng.integers(0, cov + 1))
                    nh = int(rng.integers(0, cov - nm + 1))
                    rows.append((name, pos, st, "m", cov, nm, int(rng.integers(0, 3))))
                    if rng.random() < 0.8:                              # most C carry both codes, with other counts
                        rows.append((name, pos, st, "21839", cov + 1, nh, int(rng.integers(0, 3))))
                elif canon == "A" and rng.random() < 0.6:
                    cov = int(rng.integers(1, 25))
                    rows.append((name, pos, st, "a", cov, int(rng.integers(0, cov + 1)), 0))
    for name, pos, st, code, cov, mod, diff in rows:
        r = rec.setdefault((name, code), {k: [] for k in ("position", "strand", "n_valid", "n_mod", "n_diff")})
        for k, v in zip(("position", "strand", "n_valid", "n_mod", "n_diff"), (pos, ord(st), cov, mod, diff)):
            r[k].append(v)
    rec = {k: {c: np.array(v, dtype=np.uint8 if c == "strand" else np.int64) for c, v in r.items()} for k, r in rec.items()}
    both = {(n, p, s) for n, p, s, c, *_ in rows if c == "m"} & {(n, p, s) for n, p, s, c, *_ in rows if c == "21839"}
    assert len(both) > 500
    _write_bed(tmp_path / "p.bed", rows)
    names = [("CCWGG", "m", 1), ("C", "m", 0), ("C", "21839", 0), ("GATC", "a", 1), ("CG", "21839", 0), ("CCWGG", "21839", 1), ("A", "a", 0)]
    motifs = [f"{m}_{c}_{p}" for m, c, p in names]
    seg = H.brute_force(seqs, rec, H.regex_triples(names))
    assert {c for (k, _), g in seg.items() for c in [names[k][1]]} == {"m", "21839", "a"}
    assert seg[(1, "c1")].frac != seg[(2, "c1")].frac
    for host, message in (("0", "from the device parser's columns"), ("1", "from the host parser's rows")):
        monkeypatch.setenv("NANOMOTIF_HOST_PARSER", host)
        for ot in ("median", "weighted-mean"):
            caplog.clear()
            with caplog.at_level(logging.INFO):
                got = methylation_pattern(str(tmp_path / "p.bed"), str(tmp_path / "a.fasta"), motifs, output_type=ot)
            assert message in caplog.text
            _assert_rows([tuple(r[c] for c in COLUMNS) for r in got], H.rows_of(seg, seqs, names, ot), (host, ot))
    first_m = next(i for i, r in enumerate(rows) if r[3] == "m" and r[4] >= 3 and r[6] == 0)
    dup = rows[:first_m + 1] + [rows[first_m][:5] + (0, 0)] + rows[first_m + 1:]                 # the same (contig, position, strand, code), other counts
    _write_bed(tmp_path / "dup.bed", dup)
    for host in ("0", "1"):
        monkeypatch.setenv("NANOMOTIF_HOST_PARSER", host)
        with pytest.raises(NmScanError, match="duplicate"):
            methylation_pattern(str(tmp_path / "dup.bed"), str(tmp_path / "a.fasta"), motifs)


def test_refusals_leave_the_engine_usable():
    """After every refused upload (position beyond the contig, a strand byte that is neither '+' nor '-', a negative n_diff,
    n_modified > n_valid_cov) the slot is empty, and a valid upload and query on the same engine equals the brute force."""
    from nanomotif_amd._lib import NmScanError
    from nanomotif_amd.contig_methylation import read_methylation_table, upload_read_statistics
    from nanomotif_amd.engine import ScanEngine
    _, all_seqs, all_records = H.meth_input()
    seqs = {"c": "GATC" * 40, "small": all_seqs["small"], "edge": all_seqs["edge"]}
    records = {("c", "a"): {k: np.asarray(v, dtype=np.uint8 if k == "strand" else np.int64) for k, v in LITERAL.items()},
               ("small", "a"): all_records[("small", "a")], ("edge", "a"): all_records[("edge", "a")]}
    names = [("GATC", "a", 1), ("A", "a", 0)] + H.FAMILY[:6] + [("A" + "N" * 40 + "C", "a", 0), ("A" + "N" * 94 + "T", "a", 95)]
    want = H.rows_of(H.brute_force(seqs, records, H.regex_triples(names)), seqs, names, "median")
    assert {r[0] for r in want} == {"c", "small", "edge"}
    eng = ScanEngine(0)
    order = list(seqs)
    eng.upload_assembly(order, [seqs[n] for n in order], ["b"] * 3)
    col = _columns(order, records, "a")
    st = lambda b: np.frombuffer(b, np.uint8)
    bad = [("outside the uploaded assembly", dict(contig_local=[0, 0], position=[3, 160], strand=st(b"++"), n_valid_cov=[9, 9], n_modified=[4, 4])),
           ("outside the uploaded assembly", dict(contig_local=[1, 3], position=[3, 3], strand=st(b"++"), n_valid_cov=[9, 9], n_modified=[4, 4])),
           ("strand must be", dict(contig_local=[0, 0], position=[3, 5], strand=st(b"+x"), n_valid_cov=[9, 9], n_modified=[4, 4])),
           ("negative n_diff", dict(contig_local=[0, 0], position=[3, 5], strand=st(b"+-"), n_valid_cov=[9, 9], n_modified=[4, 4], n_diff=[0, -1])),
           ("n_modified outside", dict(contig_local=[0, 2], position=[3, 8191], strand=st(b"+-"), n_valid_cov=[9, 9], n_modified=[4, 10]))]
    for message, columns in bad:
        with pytest.raises(NmScanError, match=message):
            upload_read_statistics(eng, "a", **columns)
        with pytest.raises(NmScanError, match="holds no pileup"):
            read_methylation_table(eng, ["GATC_a_1"])
        assert upload_read_statistics(eng, "a", col["contig"], col["position"], col["strand"], col["n_valid"], col["n_mod"], col["n_diff"],
                                      H.MIN_COV, H.MIN_FRAC) == H.n_kept_of(records, "a")
        _assert_rows(_table(eng, names), want, message)
    eng.close()
