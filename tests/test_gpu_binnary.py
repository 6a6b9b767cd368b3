"""The binnary commands on the device: nm_bed_parse_device_counts (csrc/nmbedgpu.hip) against the host reader
nm_bed_open_counts, nm_readstats_upload_bedcols (csrc/nmmeth.hip) against nm_readstats_upload of the host-read rows,
methylation_pattern's device path against its host path, and detect_contamination / include_contigs end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nanomotif_amd import _lib, synth

pytestmark = pytest.mark.gpu
NM_EINVAL, NM_ESTATE = -1, -3          # include/nmscan.h nm_status
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bed_text(rng, n_contigs=3, rows=400, long_names=False, extreme=True):
    """Plain modkit rows with random count columns (12 N_mod, 17 N_diff), counts 0 and 2147483647 included; long_names: contig
    names that make every line longer than 128 bytes (the walk path of the splitter)."""
    out = []
    for c in range(n_contigs):
        name = (f"contig_{c}_" + "x" * 140) if long_names else f"contig_{c}"
        for k in range(rows):
            pos = 3 * k
            mt = ("m", "a", "21839", "h")[k % 4]
            cov = int(rng.integers(0, 60))
            nmod = int(rng.integers(0, cov + 1))
            ndiff = int(rng.integers(0, 9)) if k % 5 == 0 else 0
            if extreme and k == 7:
                nmod, ndiff = 0, 2147483647
            if extreme and k == 11:
                nmod, ndiff = 2147483647, 0
            out.append(f"{name}\t{pos}\t{pos + 1}\t{mt}\t{cov}\t{'+-'[k % 2]}\t{pos}\t{pos + 1}\t255,0,0\t{cov}\t{rng.integers(0, 10000) / 100:.2f}\t"
                       f"{nmod}\t{max(cov - nmod, 0)}\t0\t0\t0\t{ndiff}\t0\n")
    return "".join(out)


def _host_counts(path):
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.nm_bed_open_counts(os.fsencode(path), 2, C.byref(h)))
    try:
        n, nc = C.c_uint64(0), C.c_uint32(0)
        _lib.check(lib.nm_bed_shape(h, C.byref(n), C.byref(nc)))
        ptr = [C.c_void_p() for _ in range(6)]
        _lib.check(lib.nm_bed_columns(h, *[C.byref(x) for x in ptr]))
        cnt = [C.c_void_p(), C.c_void_p()]
        _lib.check(lib.nm_bed_count_columns(h, C.byref(cnt[0]), C.byref(cnt[1])))
        view = lambda q, ct: np.ctypeslib.as_array(C.cast(q, C.POINTER(ct)), shape=(n.value,)).copy()
        return dict(contig=view(ptr[0], C.c_uint32), position=view(ptr[1], C.c_int64), mod=view(ptr[2], C.c_int8), strand=view(ptr[3], C.c_uint8),
                    frac=view(ptr[4], C.c_double), nvalid=view(ptr[5], C.c_int64), nmod=view(cnt[0], C.c_int32), ndiff=view(cnt[1], C.c_int32))
    finally:
        lib.nm_bed_close(h)


def _device_counts(eng, path):
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.nm_bed_parse_device_counts(eng.ctx, os.fsencode(path), 2, C.byref(h)))
    try:
        n, nc = C.c_uint64(0), C.c_uint32(0)
        _lib.check(lib.nm_bedcols_shape(h, C.byref(n), C.byref(nc), None, None))
        d = [C.c_void_p() for _ in range(7)]
        _lib.check(lib.nm_bedcols_device_columns(h, *[C.byref(x) for x in d]))
        cnt = [C.c_void_p(), C.c_void_p()]
        _lib.check(lib.nm_bedcols_count_columns(h, C.byref(cnt[0]), C.byref(cnt[1])))

        def read(q, dt):
            a = np.zeros(n.value, dt)
            if n.value:
                _lib.check(lib.nm_device_read(eng.ctx, a.ctypes.data_as(C.c_void_p), q, a.nbytes))
            return a
        return dict(contig=read(d[1], np.uint32), position=read(d[2], np.uint32), mod=read(d[3], np.int8), strand=read(d[4], np.uint8),
                    frac=read(d[5], np.float64), nvalid=read(d[6], np.int32), nmod=read(cnt[0], np.int32), ndiff=read(cnt[1], np.int32))
    finally:
        lib.nm_bedcols_close(h)


def _same_rows(host, dev):
    assert len(host["nmod"]) == len(dev["nmod"]) > 0
    assert np.array_equal(host["contig"], dev["contig"])
    assert np.array_equal(host["position"], dev["position"].astype(np.int64))
    assert np.array_equal(host["mod"], dev["mod"]) and np.array_equal(host["strand"], dev["strand"])
    assert np.array_equal(host["frac"].view(np.uint64), dev["frac"].view(np.uint64))
    assert np.array_equal(np.clip(host["nvalid"], -1, 2**31 - 1).astype(np.int32), dev["nvalid"])
    assert np.array_equal(host["nmod"], dev["nmod"]) and np.array_equal(host["ndiff"], dev["ndiff"])


@pytest.mark.parametrize("long_names", [False, True])
def test_count_columns_equal_the_host_reader_plain_and_bgzip(tmp_path, long_names):
    from nanomotif_amd.e2e_synth import bgzip_tabix
    from nanomotif_amd.engine import ScanEngine
    text = _bed_text(np.random.default_rng(5 + long_names), long_names=long_names)
    assert long_names == all(len(l) > 128 for l in text.splitlines())
    plain = str(tmp_path / "p.bed")
    with open(plain, "w") as f:
        f.write(text)
    gz = str(tmp_path / "p.bed.gz")
    bgzip_tabix(plain, gz)
    eng = ScanEngine(0)
    try:
        host = _host_counts(plain)
        assert {0, 2147483647} <= set(host["nmod"].tolist()) and 2147483647 in host["ndiff"].tolist()
        for path in (plain, gz):
            _same_rows(host, _device_counts(eng, path))
        # columns parsed without counts: NM_ESTATE, like nm_bed_count_columns
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.nm_bed_parse_device(eng.ctx, os.fsencode(plain), 2, C.byref(h)))
        a, b = C.c_void_p(), C.c_void_p()
        assert lib.nm_bedcols_count_columns(h, C.byref(a), C.byref(b)) == NM_ESTATE
        lib.nm_bedcols_close(h)
    finally:
        eng.close()


@pytest.mark.parametrize("bad", ["-1", "2147483648", "NA", "1x"])
def test_bad_counts_are_refused_like_the_host_reader(tmp_path, bad):
    from nanomotif_amd.engine import ScanEngine
    lib = _lib.load()
    good = "c1\t5\t6\ta\t9\t+\t5\t6\t255,0,0\t9\t50.00\t4\t5\t0\t0\t0\t0\t0\n"
    for col in (11, 16):
        fields = good.rstrip("\n").split("\t")
        fields[col] = bad
        path = str(tmp_path / f"bad{col}.bed")
        with open(path, "w") as f:
            f.write(good + "\t".join(fields) + "\n" + good.replace("\t5\t6\t", "\t8\t9\t"))
        h = C.c_void_p()
        rc_host = lib.nm_bed_open_counts(os.fsencode(path), 1, C.byref(h))
        msg_host = lib.nm_last_error().decode()
        assert rc_host == NM_EINVAL and "column 12 (N_mod) or 17 (N_diff)" in msg_host
        eng = ScanEngine(0)
        try:
            rc = lib.nm_bed_parse_device_counts(eng.ctx, os.fsencode(path), 1, C.byref(h))
            msg = lib.nm_last_error().decode()
            assert (rc, msg) == (rc_host, msg_host) or rc == _lib.NM_EDECLINED
        finally:
            eng.close()


def test_readstats_from_device_columns_equal_the_host_upload(tmp_path):
    """Per mod code: the same n_kept and the same table as nm_readstats_upload of the host-read rows — with records exactly at
    the coverage and diff-fraction thresholds and a pileup contig the assembly lacks."""
    from nanomotif_amd.contig_methylation import MOD_CODES, read_methylation_table, upload_read_statistics
    from nanomotif_amd.engine import ScanEngine
    mg = synth.make_metagenome(synth.SynthSpec(n_contigs=3, total_bp=150_000, n_bins=1, mod_types=("a", "m", "21839"), seed=17,
                                               min_contig_bp=30_000, fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m"), ("GCGC", 1, "21839"))))
    rng = np.random.default_rng(3)
    lines = []
    for i, name in enumerate(mg.names):
        rows = []
        for mt in mg.spec.mod_types:
            p = mg.contig_pileup(i, mt)
            for pos, st, cov in zip(p["position"].tolist(), p["strand"].tolist(), p["nvalid"].tolist()):
                r = rng.random()
                if r < 0.05:
                    cov, ndiff = 3, 0                  # coverage exactly at --min_valid_read_coverage
                elif r < 0.10:
                    cov, ndiff = 8, 2                  # 8 / 10 = 0.8 exactly
                elif r < 0.15:
                    cov, ndiff = 8, 3                  # below 0.8
                else:
                    ndiff = 0
                nmod = int(rng.integers(0, cov + 1))
                rows.append((pos, mt, chr(st), cov, nmod, ndiff))
        rows.sort(key=lambda r: (r[0], r[1]))
        for pos, mt, st, cov, nmod, ndiff in rows:
            lines.append(f"{name}\t{pos}\t{pos + 1}\t{mt}\t{cov}\t{st}\t{pos}\t{pos + 1}\t255,0,0\t{cov}\t50.00\t{nmod}\t{cov - nmod}\t0\t0\t0\t{ndiff}\t0\n")
    lines.append("stranger\t7\t8\ta\t9\t+\t7\t8\t255,0,0\t9\t50.00\t4\t5\t0\t0\t0\t0\t0\n")
    path = str(tmp_path / "p.bed")
    with open(path, "w") as f:
        f.write("".join(lines))
    motifs = ["GATC_a_1", "CCWGG_m_1", "GCGC_21839_1", "A_a_0", "C_m_0"]
    lib = _lib.load()

    def engine():
        eng = ScanEngine(0)
        eng.upload_assembly(mg.names, [mg.contig_ascii(i) for i in range(len(mg.names))], ["all"] * len(mg.names))
        return eng
    host = _host_counts(path)
    nh = C.c_void_p()
    _lib.check(lib.nm_bed_open_counts(os.fsencode(path), 1, C.byref(nh)))
    names = []
    for i in range(len(set(host["contig"].tolist()))):
        s = C.c_char_p()
        _lib.check(lib.nm_bed_contig_name(nh, i, C.byref(s)))
        names.append(s.value.decode())
    lib.nm_bed_close(nh)
    assert "stranger" in names
    lut = np.array([mg.names.index(n) if n in mg.names else 0xFFFFFFFF for n in names], np.uint32)
    want_kept, want_rows = {}, {}
    eng = engine()
    try:
        for mt in MOD_CODES:
            sel = np.flatnonzero(host["mod"] == MOD_CODES.index(mt))
            want_kept[mt] = upload_read_statistics(eng, mt, lut[host["contig"][sel]], host["position"][sel], host["strand"][sel],
                                                   np.clip(host["nvalid"][sel], -1, 2**31 - 1), host["nmod"][sel], host["ndiff"][sel], 3, 0.8)
        for ot in ("median", "weighted-mean"):
            want_rows[ot] = read_methylation_table(eng, motifs, ot)
    finally:
        eng.close()
    eng = engine()
    h = C.c_void_p()
    try:
        _lib.check(lib.nm_bed_parse_device_counts(eng.ctx, os.fsencode(path), 1, C.byref(h)))
        kept = C.c_uint64(0)
        assert lib.nm_readstats_upload_bedcols(eng.ctx, h, 0, 0, 3, 0.8, C.byref(kept)) == NM_ESTATE      # before the contig map
        dnames = []
        for i in range(len(names)):
            s = C.c_char_p()
            _lib.check(lib.nm_bedcols_contig_name(h, i, C.byref(s)))
            dnames.append(s.value.decode())
        assert dnames == names
        _lib.check(lib.nm_bedcols_map_contigs(h, lut.ctypes.data_as(C.POINTER(C.c_uint32)), len(lut)))
        for mt in MOD_CODES:
            slot = MOD_CODES.index(mt)
            _lib.check(lib.nm_readstats_upload_bedcols(eng.ctx, h, slot, slot, 3, 0.8, C.byref(kept)))
            assert kept.value == want_kept[mt] > 0, mt
        for ot in ("median", "weighted-mean"):
            assert read_methylation_table(eng, motifs, ot) == want_rows[ot]
    finally:
        if h:
            lib.nm_bedcols_close(h)
        eng.close()


def test_methylation_pattern_device_path_equals_host_path(tmp_path, monkeypatch):
    from nanomotif_amd.contig_methylation import methylation_pattern
    from nanomotif_amd.e2e_synth import bgzip_tabix
    mg = synth.make_metagenome(synth.SynthSpec(n_contigs=4, total_bp=200_000, n_bins=2, mod_types=("a", "m"), seed=29, min_contig_bp=20_000))
    mg.write_fasta(str(tmp_path / "a.fasta"))
    mg.write_bed(str(tmp_path / "p.bed"))
    bgzip_tabix(str(tmp_path / "p.bed"), str(tmp_path / "p.bed.gz"))
    motifs = ["GATC_a_1", "CCWGG_m_1", "GAATTC_a_2", "GCGC_m_1", "A_a_0"]
    for pileup in ("p.bed", "p.bed.gz"):
        for ot in ("median", "weighted-mean"):
            got = {}
            for host in ("0", "1"):
                monkeypatch.setenv("NANOMOTIF_HOST_PARSER", host)
                out = tmp_path / f"{pileup}.{ot}.{host}.tsv"
                rows = methylation_pattern(str(tmp_path / pileup), str(tmp_path / "a.fasta"), motifs, threads=2, output=str(out), output_type=ot)
                got[host] = (rows, out.read_bytes())
            assert got["0"][0] and got["0"] == got["1"], (pileup, ot)


def _cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "nanomotif_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_cli_detect_contamination_and_include_contigs(tmp_path):
    import pandas as pd
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import binnary_synth as bs
    mg = bs.make_metagenome()
    paths = bs.write_inputs(mg, str(tmp_path / "in"))
    moved, unbinned, listed = bs.layout(mg)
    common = ["--pileup", paths["pileup"], "--assembly", paths["assembly"], "--bin_motifs", paths["bin_motifs"], "--contig_bins", paths["contig_bins"]]

    out = str(tmp_path / "dc")
    _cli(["detect_contamination"] + common + ["--out", out, "--write_bins"])
    cont = pd.read_csv(os.path.join(out, "bin_contamination.tsv"), sep="\t")
    assert list(cont.columns) == ["contig", "bin", "method", "cluster", "bin_cluster", "bin_length", "n_contigs_bin", "fraction_contigs", "fraction_length"]
    assert set(cont["contig"]) == {moved} and set(cont["bin"]) == {bs.BIN_B}
    new = pd.read_csv(os.path.join(out, "decontaminated_contig_bin.tsv"), sep="\t", dtype=str)
    assert list(new.columns) == ["contig", "bin"] and moved not in set(new["contig"]) and len(new) == len(listed) - 1
    for b in sorted(set(new["bin"])):                                  # --write_bins: the assembly's sequences, 60 per line
        text = open(os.path.join(out, "detect_contamination_bins", f"{b}.fa")).read()
        want = "".join(f">{c}\n" + "".join(mg.contig_str(mg.names.index(c))[k:k + 60] + "\n" for k in range(0, int(mg.lengths[mg.names.index(c)]), 60))
                       for c in new[new["bin"] == b]["contig"])
        assert text == want
    assert os.path.exists(os.path.join(out, "args.detect_contamination.json")) and os.path.isdir(os.path.join(out, "logs"))

    out = str(tmp_path / "ic")
    _cli(["include_contigs"] + common + ["--out", out, "--run_detect_contamination"])
    inc = pd.read_csv(os.path.join(out, "include_contigs.tsv"), sep="\t")
    assert list(inc.columns) == ["contig", "bin", "assigned_bin", "method", "prob", "mean_prob", "confidence"]
    mine = inc[inc["contig"] == unbinned]
    assert len(mine) == 3 and set(mine["assigned_bin"]) == {bs.BIN_A} and set(mine["confidence"]) == {"high_confidence"}
    new = pd.read_csv(os.path.join(out, "new_contig_bin.tsv"), sep="\t", dtype=str)
    assert new[new["contig"] == unbinned]["bin"].tolist() == [bs.BIN_A]

    # the cached table: reused without --force (not rewritten), recomputed with it
    table = os.path.join(out, "motifs-scored-read-methylation_median.tsv")
    before = os.stat(table).st_mtime_ns
    os.utime(table, ns=(before - 10**9, before - 10**9))
    stamp = os.stat(table).st_mtime_ns
    _cli(["include_contigs"] + common + ["--out", out, "--run_detect_contamination"])
    assert os.stat(table).st_mtime_ns == stamp
    _cli(["include_contigs"] + common + ["--out", out, "--run_detect_contamination", "--force"])
    assert os.stat(table).st_mtime_ns != stamp
    assert pd.read_csv(os.path.join(out, "include_contigs.tsv"), sep="\t").equals(inc)

    # weighted_mean: the weighted mean, under that name
    out = str(tmp_path / "wm")
    _cli(["detect_contamination"] + common + ["--out", out, "--methylation_output_type", "weighted_mean"])
    assert os.path.exists(os.path.join(out, "motifs-scored-read-methylation_weighted_mean.tsv"))
