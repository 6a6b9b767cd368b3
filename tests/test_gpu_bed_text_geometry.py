"""The text half of csrc/nmbedgpu.hip — line starts, field split, number parsers, runs, patched rows, slabs of whole lines — against the plain
Python reference of tests/bed_text_geometry.py (NOT against the host reader, which shares csrc/nmbed_parse.h with the device path), by equality
only, on the inputs whose borders tests/test_bed_text_geometry_host.py counts.  Every cell that cuts the text into slabs of whole lines asserts
the slab count, the largest line count of a slab, the runs and the rows handed to the host's routines from the NM_BED_TIMING line, so that no
cell passes on a path it did not take."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import bed_text_geometry as bg
from nanomotif_amd import _lib
from nanomotif_amd import pileup as pp

pytestmark = pytest.mark.gpu
TIMING = re.compile(r"text slabs: (\d+) slabs of at most (\d+) bytes \((\d+) with rows\), at most (\d+) lines in a slab, (\d+) runs, (\d+) rows for the host's routines")
INFLATE = re.compile(r"device inflate: (\d+) slabs")


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def eng():
    from nanomotif_amd.engine import ScanEngine
    e = ScanEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the texts as files, each with its reference rows (computed once, never changed) and a census per slab grid, made when first asked for"""
    from helpers import write_bgzf_tabix
    d = tmp_path_factory.mktemp("bed_text")
    out = {}
    for name, text in (("geometry", bg.geometry_text()), ("crlf", bg.geometry_text_crlf()), ("numbers", bg.number_text())):
        path = str(d / (name + ".bed"))
        open(path, "wb").write(text)
        out[name] = dict(path=path, text=text, ref=bg.reference_parse(text, counts=True), census={})
    for block in (777, 0xFF00):
        gz = str(d / ("geometry_%d.bed.gz" % block))
        write_bgzf_tabix(bg.geometry_text(), gz, block_size=block)
        out["gz_%d" % block] = dict(out["geometry"], path=gz)
    good = bg.good_rows(7)
    out["good"] = dict(path=str(d / "good.bed"), text=good, ref=bg.reference_parse(good, counts=True))
    open(out["good"]["path"], "wb").write(good)
    return out


def census_of(item, grid):
    if grid not in item["census"]:
        item["census"][grid] = bg.census(item["text"], grid)
    return item["census"][grid]


def device_rows(eng, path, counts, threads=0):
    """the device parser's rows in the shape of bed_text_geometry.reference_parse, runs included: DevicePileup (nm_bed_parse_device) or
    nm_bed_parse_device_counts; NmScanError when the file is refused"""
    lib = _lib.load()
    if not counts:
        dev = pp.DevicePileup(eng, path, threads=threads)
        try:
            cols = dev.to_host()
            codes = [dev.mod_code(i) for i in range(3, int(cols["mod_type"].max()) + 1)]
            return dict(names=dev.contig_names, other_codes=codes, contig=cols["file_contig"], position=cols["position"], mod_type=cols["mod_type"],
                        strand=cols["strand"], nvalid_cov=cols["nvalid_cov"], fraction_mod=cols["fraction_mod"], run_row=dev.run_row.copy(),
                        run_contig=dev.run_contig.copy())
        finally:
            dev.close()
    h = C.c_void_p()
    _lib.check(lib.nm_bed_parse_device_counts(eng.ctx, os.fsencode(path), threads, C.byref(h)))
    try:
        n, nc, nr = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        _lib.check(lib.nm_bedcols_shape(h, C.byref(n), C.byref(nc), C.byref(nr), None))
        d = [C.c_void_p() for _ in range(7)]
        _lib.check(lib.nm_bedcols_device_columns(h, *[C.byref(x) for x in d]))
        cnt = [C.c_void_p(), C.c_void_p()]
        _lib.check(lib.nm_bedcols_count_columns(h, C.byref(cnt[0]), C.byref(cnt[1])))

        def read(q, dt):
            a = np.zeros(n.value, dt)
            if n.value:
                _lib.check(lib.nm_device_read(eng.ctx, a.ctypes.data_as(C.c_void_p), q, a.nbytes))
            return a
        out = dict(contig=read(d[1], np.uint32), position=read(d[2], np.uint32), mod_type=read(d[3], np.int8), strand=read(d[4], np.uint8),
                   fraction_mod=read(d[5], np.float64), nvalid_cov=read(d[6], np.int32), nmod=read(cnt[0], np.int32), ndiff=read(cnt[1], np.int32))
        s = C.c_char_p()
        out["names"], out["other_codes"] = [], []
        for i in range(nc.value):
            _lib.check(lib.nm_bedcols_contig_name(h, i, C.byref(s)))
            out["names"].append(s.value.decode())
        for i in range(3, int(out["mod_type"].max()) + 1 if n.value else 3):
            _lib.check(lib.nm_bedcols_mod_code(h, i, C.byref(s)))
            out["other_codes"].append(s.value.decode())
        out["run_row"] = np.zeros(nr.value + 1, np.uint64)
        out["run_contig"] = np.zeros(max(nr.value, 1), np.uint32)
        _lib.check(lib.nm_bedcols_runs(h, out["run_row"].ctypes.data_as(C.POINTER(C.c_uint64)), out["run_contig"].ctypes.data_as(C.POINTER(C.c_uint32))))
        out["run_contig"] = out["run_contig"][:nr.value]
        return out
    finally:
        lib.nm_bedcols_close(h)


def assert_device_equals_reference(got, ref, counts):
    bg.assert_rows_equal(got, ref, counts)
    assert len(got["run_contig"]) == len(ref["run_contig"])                                  # the number of runs, and where they start
    assert np.array_equal(got["run_row"], ref["run_row"]) and np.array_equal(got["run_contig"], ref["run_contig"])


def assert_path_taken(err, item, grid):
    """the NM_BED_TIMING line of a parse that cut the text into slabs of whole lines, against the geometry restated"""
    m = TIMING.search(err)
    assert m, err[-2000:]
    c = census_of(item, grid)
    expect = (c["slabs"], bg.slab_size(grid), c["slabs"] - c.get("slabs_without_rows", 0), c["most_lines_in_a_slab"], c["runs"], c.get("rows_for_host", 0))
    assert tuple(int(x) for x in m.groups()) == expect


@pytest.mark.parametrize("counts", [False, True], ids=["six_columns", "count_columns"])
@pytest.mark.parametrize("threads", [0, 3])
@pytest.mark.parametrize("grid", bg.GRIDS, ids=["unset", "65536", "131072"])
def test_geometry_text_plain(eng, inputs, capfd, grid, threads, counts):
    item = inputs["geometry"]
    with environment({"NM_BED_TIMING": "1", **({"NM_BED_SLAB_BYTES": str(grid)} if grid else {})}):
        got = device_rows(eng, item["path"], counts, threads)
    assert_path_taken(capfd.readouterr().err, item, grid)
    assert_device_equals_reference(got, item["ref"], counts)


@pytest.mark.parametrize("counts", [False, True], ids=["six_columns", "count_columns"])
def test_geometry_text_with_crlf_line_ends(eng, inputs, capfd, counts):
    item = inputs["crlf"]
    with environment({"NM_BED_TIMING": "1", "NM_BED_SLAB_BYTES": "65536"}):
        got = device_rows(eng, item["path"], counts)
    assert_path_taken(capfd.readouterr().err, item, 65536)
    assert census_of(item, 65536)["slabs"] >= 7 and census_of(item, 65536)["crlf_rows"] > 7000
    assert_device_equals_reference(got, item["ref"], counts)


def inflate_slabs(n_text, block, cap):
    """how many slabs of whole BGZF members of `block` bytes of text the device-inflate path makes of n_text bytes (csrc/nmbedgpu.hip)"""
    sizes = [min(block, n_text - o) for o in range(0, n_text, block)]
    slabs, have = 0, None
    for s in sizes:
        if have is None or have + s > cap:
            slabs, have = slabs + 1, 0
        have += s
    return slabs


@pytest.mark.parametrize("counts", [False, True], ids=["six_columns", "count_columns"])
@pytest.mark.parametrize("env", [{}, {"NM_BED_INFLATE_SLAB": "70000"}, {"NM_BED_HOST_INFLATE": "1"}, {"NM_BED_HOST_INFLATE": "1", "NM_BED_SLAB_BYTES": "65536"}],
                         ids=["device_inflate", "device_inflate_slabs_of_70000", "host_inflate", "host_inflate_slabs_of_65536"])
@pytest.mark.parametrize("block", [777, 0xFF00])
def test_geometry_text_through_bgzip(eng, inputs, capfd, block, env, counts):
    item = inputs["gz_%d" % block]
    with environment({"NM_BED_TIMING": "1", **env}):
        got = device_rows(eng, item["path"], counts, threads=3)
    err = capfd.readouterr().err
    if "NM_BED_HOST_INFLATE" in env:
        assert_path_taken(err, item, int(env["NM_BED_SLAB_BYTES"]) if "NM_BED_SLAB_BYTES" in env else None)
    else:
        m = INFLATE.search(err)
        assert m and int(m.group(1)) == inflate_slabs(len(item["text"]), block, int(env.get("NM_BED_INFLATE_SLAB", 3 << 30))), err[-2000:]
        assert not TIMING.search(err)
    assert_device_equals_reference(got, item["ref"], counts)


@pytest.mark.parametrize("counts", [False, True], ids=["six_columns", "count_columns"])
@pytest.mark.parametrize("grid", [None, 65536], ids=["unset", "65536"])
def test_number_text(eng, inputs, capfd, grid, counts):
    item = inputs["numbers"]
    with environment({"NM_BED_TIMING": "1", **({"NM_BED_SLAB_BYTES": str(grid)} if grid else {})}):
        got = device_rows(eng, item["path"], counts)
    assert_path_taken(capfd.readouterr().err, item, grid)
    assert census_of(item, grid)["rows_for_host"] > 3000
    assert_device_equals_reference(got, item["ref"], counts)


@pytest.mark.parametrize("counts", [False, True], ids=["six_columns", "count_columns"])
def test_the_ends_a_text_can_have(eng, tmp_path, counts):
    for name, text in bg.tail_texts().items():
        path = str(tmp_path / (name + ".bed"))
        open(path, "wb").write(text)
        assert_device_equals_reference(device_rows(eng, path, counts), bg.reference_parse(text, counts), counts)


@pytest.mark.parametrize("counts", [False, True], ids=["six_columns", "count_columns"])
@pytest.mark.parametrize("name", list(bg.slab_tail_texts()))
def test_the_ends_of_a_text_of_several_slabs(eng, tmp_path, capfd, name, counts):
    """the rows the several-slab refusals are cut out of, with every end a text can have: three slabs by the timing line (so the refusals below,
    which print no line, do meet more than one slab), the open last line of 127 | 128 bytes on the mask path of a last slab"""
    text = bg.slab_tail_texts()[name]
    path = str(tmp_path / "m.bed")
    open(path, "wb").write(text)
    item = dict(text=text, census={})
    with environment({"NM_BED_TIMING": "1", "NM_BED_SLAB_BYTES": "65536"}):
        got = device_rows(eng, path, counts, threads=3)
    assert_path_taken(capfd.readouterr().err, item, 65536)
    assert census_of(item, 65536)["slabs"] >= 3
    assert_device_equals_reference(got, bg.reference_parse(text, counts), counts)


@pytest.mark.parametrize("case", bg.refusals(), ids=lambda r: r[0])
def test_refusals_and_a_valid_parse_after_each(eng, inputs, tmp_path, case):
    name, text, grid, words = case
    path = str(tmp_path / "r.bed")
    open(path, "wb").write(text)
    for counts in (False, True):
        with environment({"NM_BED_SLAB_BYTES": str(grid)} if grid else {}):
            if words is None:
                assert_device_equals_reference(device_rows(eng, path, counts), bg.reference_parse(text, counts), counts)
            else:
                with pytest.raises(_lib.NmScanError, match=words):
                    device_rows(eng, path, counts)
        assert_device_equals_reference(device_rows(eng, inputs["good"]["path"], counts), inputs["good"]["ref"], counts)
