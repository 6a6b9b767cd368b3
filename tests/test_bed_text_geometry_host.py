"""The inputs of tests/bed_text_geometry.py hold, by count, every border they claim to hold, for each of the three slab grids the GPU test runs
them on (NM_BED_SLAB_BYTES unset, 65 536, 131 072); and the HOST reader (nm_bed_open, nm_bed_open_counts: csrc/nmbed.cpp) equals the reference
parser on them, refusals and their words included.  No GPU: tests/test_gpu_bed_text_geometry.py compares the device parser with the same
reference; this file proves that the comparison meets the code it is meant to meet, and is where a defect of csrc/nmbed_parse.h — shared by
the host reader and the device path's patch routine — shows first."""
import ctypes as C
import os

import numpy as np
import pytest

import bed_text_geometry as bg
from nanomotif_amd import _lib


@pytest.fixture(scope="module")
def counts():
    text = bg.geometry_text()
    return {g: bg.census(text, g) for g in bg.GRIDS}


def host_rows(path, counts=False, threads=1):
    """the host reader's rows in the shape of bed_text_geometry.reference_parse; NmScanError when it refuses the file"""
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check((lib.nm_bed_open_counts if counts else lib.nm_bed_open)(os.fsencode(path), threads, C.byref(h)))
    try:
        n, nc = C.c_uint64(0), C.c_uint32(0)
        _lib.check(lib.nm_bed_shape(h, C.byref(n), C.byref(nc)))
        ptr = [C.c_void_p() for _ in range(6)]
        _lib.check(lib.nm_bed_columns(h, *[C.byref(x) for x in ptr]))
        view = lambda q, ct: np.ctypeslib.as_array(C.cast(q, C.POINTER(ct)), shape=(n.value,)).copy()
        out = dict(contig=view(ptr[0], C.c_uint32), position=view(ptr[1], C.c_int64), mod_type=view(ptr[2], C.c_int8), strand=view(ptr[3], C.c_uint8),
                   fraction_mod=view(ptr[4], C.c_double))
        # nm_bed_columns hands out the 64-bit coverage as parsed; the clamp below is nm_bed_ingest_columns' documented rule applied BY THIS TEST, so
        # the clamp itself is not under test here (test_ingest_columns_clamp_the_coverage reads the reader's own 32-bit column); what is: that the
        # parse saturates and does not wrap (2^64 + 7 must arrive above 2^31 - 1, not as 7)
        out["nvalid_cov"] = np.clip(view(ptr[5], C.c_int64), -1, 2**31 - 1)
        if counts:
            cnt = [C.c_void_p(), C.c_void_p()]
            _lib.check(lib.nm_bed_count_columns(h, C.byref(cnt[0]), C.byref(cnt[1])))
            out["nmod"], out["ndiff"] = view(cnt[0], C.c_int32), view(cnt[1], C.c_int32)
        s = C.c_char_p()
        out["names"] = []
        for i in range(nc.value):
            _lib.check(lib.nm_bed_contig_name(h, i, C.byref(s)))
            out["names"].append(s.value.decode())
        out["other_codes"] = []
        for i in range(3, int(out["mod_type"].max()) + 1 if n.value else 3):
            _lib.check(lib.nm_bed_mod_code(h, i, C.byref(s)))
            out["other_codes"].append(s.value.decode())
        return out
    finally:
        lib.nm_bed_close(h)


def test_geometry_restated():
    assert bg.slab_size(None) == 32 << 20 and bg.slab_size(1) == 65536 and bg.slab_size(1 << 30) == 32 << 20 and bg.slab_size(70000) == 70000
    assert bg.slab_cuts(b"ab\ncd\nef", None) == [0, 8] and bg.slab_cuts(b"", 65536) == [0]
    text = b"x" * 65530 + b"\n" + b"y" * 10 + b"\n" + b"z" * 70000
    assert bg.slab_cuts(text[:65600], 65536) == [0, 65531, 65600]
    with pytest.raises(bg.Refused, match="a line longer than"):
        bg.slab_cuts(text, 65536)
    assert [o for o, _ in bg.lines_of(b"a\n\nb\r\n\r\nc")] == [0, 3, 8] and [l for _, l in bg.lines_of(b"a\r\n\r")] == [b"a"]
    assert bg.fast_path(b"9007199254740991") and not bg.fast_path(b"9007199254740992") and bg.fast_path(b"0." + b"0" * 21 + b"7")
    assert not bg.fast_path(b"0." + b"0" * 22 + b"7") and not bg.fast_path(b"1e2") and not bg.fast_path(b"-") and bg.fast_path(b"+.5")
    assert bg.percent_value(b"0x10") is None and bg.percent_value(b" 1.5") is None and bg.percent_value(b"nan(1)") is None
    assert bg.percent_value(b".") is None and bg.percent_value(b"5.") == 0.05 and bg.percent_value(b"-Infinity") == -np.inf and bg.percent_value(b"NA") == -1.0


def test_text_sizes_slab_counts_and_inflate_tails():
    text = bg.geometry_text()
    assert 600_000 <= len(text) <= 800_000
    ref = bg.reference_parse(text, counts=True)
    assert len(ref["position"]) > 7000 and ref["other_codes"] == ["h", "17596", "21839x"] and len(ref["names"]) >= 12
    assert [len(bg.slab_cuts(text, g)) - 1 for g in bg.GRIDS] == [1, 11, 6]
    numbers = bg.number_text()
    assert 30_000 <= numbers.count(b"\n") <= 32_000 and len(bg.slab_cuts(numbers, 65536)) - 1 >= 20
    for e in bg.inflate_slab_tails(text, 777), bg.inflate_slab_tails(text, 0xFF00):      # bed_tail_kernel walks back over more than one piece
        assert max(e) > 4096


@pytest.mark.parametrize("g", bg.GRIDS, ids=["unset", "65536", "131072"])
def test_line_start_borders(counts, g):
    c = counts[g]
    for key in ("start_on_group_byte_0", "start_on_group_byte_63", "start_on_group_byte_1", "start_on_block_byte_16383", "start_on_block_byte_0",
                "newline_on_63_start_on_0", "newline_on_16383_start_on_0", "nn_inside_group", "nn_on_63_64", "nn_on_16383_16384", "rn_inside_group",
                "rn_on_63_64", "rn_on_16383_16384", "groups_without_start", "blocks_without_start", "text_ends_open"):
        assert c.get(key, 0) >= 1, key
    ends = {k: bg.census(t, g) for k, t in bg.tail_texts().items()}
    assert ends["newline"]["text_ends_n"] and ends["crlf"]["text_ends_rn"] and ends["nn"]["nn_ends_text"] and ends["rn_alone"]["rn_ends_text"]
    assert ends["r_alone"]["rn_inside_group"] + ends["r_alone"].get("rn_on_63_64", 0) == 1
    for ln in (127, 128, 129):
        assert ends["open_%d" % ln]["open_last_line_of_%d" % ln] == 1


@pytest.mark.parametrize("g", bg.GRIDS, ids=["unset", "65536", "131072"])
def test_field_split_borders(counts, g):
    c = counts[g]
    for ln in (63, 64, 79, 80, 95, 96, 111, 112, 126, 127, 128, 129):      # (15 | 16: a line of 17 tabs is longer: tests' refusals hold those)
        assert c.get("newline_on_line_byte_%d" % ln, 0) >= 1, ln
    assert c["open_last_line_of_129"] == 1 and c["mask_lines"] > 6000 and c["walk_lines"] > 100
    for key in ("tab_on_line_byte_63", "tab_on_line_byte_64", "tab11_on_line_byte_63", "tab11_on_line_byte_64", "tab17_on_line_byte_63",
                "tab17_on_line_byte_64", "tab17_on_line_byte_127", "tab17_on_line_byte_128", "tab17_beyond_mask", "wave_one_walk_line",
                "wave_one_mask_line", "crlf_rows"):
        assert c.get(key, 0) >= 1, key
    for col in (10, 11):
        for sp in ("", "NA", "null"):
            assert c["null_%r_in_column_%d" % (sp, col)] >= 1


@pytest.mark.parametrize("g", bg.GRIDS, ids=["unset", "65536", "131072"])
def test_run_and_slab_borders(counts, g):
    c = counts[g]
    for key in ("change_on_line_255", "change_on_line_256", "change_on_last_row_of_slab", "run_comes_back", "one_row_run_inside_slab",
                "names_differ_in_last_byte", "names_differ_in_length"):
        assert c.get(key, 0) >= 1, key
    assert c["runs"] == len(bg.reference_parse(bg.geometry_text())["run_contig"])
    if g:
        for key in ("change_on_first_row_of_slab", "contig_continues_across_slabs", "name_of_63_starts_slab", "name_of_64_starts_slab",
                    "line_ends_on_nominal_end", "straddle_by_1", "straddle_over_4096", "straddle_20000_line"):
            assert c.get(key, 0) >= 1, key
    if g == 65536:
        assert c["slabs"] >= 7                                           # the ring of three and both device buffers are used three times
        assert c["slab_without_rows_between_rows"] == 1 and c["contig_continues_across_empty_slab"] == 1


@pytest.mark.parametrize("g", bg.GRIDS, ids=["unset", "65536", "131072"])
def test_rows_for_the_host_routines(counts, g):
    c = counts[g]
    for key in ("host_code_h", "host_code_17596", "host_code_21839x", "host_exponent", "host_both_flags", "host_first_row_of_slab", "host_last_row_of_slab",
                "host_line_of_1022", "host_line_of_1023", "host_line_of_1024", "host_line_of_1025", "host_line_of_1026"):
        assert c.get(key, 0) >= 1, key
    assert c["host_first_row_of_slab"] >= (1 if g is None else 3) and c["rows_for_host"] >= 20


@pytest.mark.parametrize("which", ["geometry", "geometry_crlf", "numbers"] + ["end_" + k for k in bg.tail_texts()] + ["slab_end_" + k for k in bg.slab_tail_texts()])
def test_host_reader_equals_the_reference(tmp_path, which):
    text = {"geometry": bg.geometry_text, "geometry_crlf": bg.geometry_text_crlf, "numbers": bg.number_text}.get(
        which, lambda: bg.slab_tail_texts()[which[9:]] if which.startswith("slab_end_") else bg.tail_texts()[which[4:]])()
    path = str(tmp_path / "t.bed")
    open(path, "wb").write(text)
    ref = bg.reference_parse(text, counts=True)
    for counts_too, threads in ((False, 1), (True, 1), (True, 3)):
        bg.assert_rows_equal(host_rows(path, counts_too, threads), ref, counts_too)


def test_number_text_reaches_what_it_names():
    ref = bg.reference_parse(bg.number_text(), counts=True)
    strings = bg.number_strings()
    assert len(strings) == len(ref["position"]) and sum(bg.fast_path(s.encode()) for s in strings) > 20_000
    assert sum(not bg.fast_path(s.encode()) for s in strings) > 3_000
    assert {-1, 0, 2**31 - 2, 2**31 - 1} <= set(ref["nvalid_cov"].tolist()) and int((ref["nvalid_cov"] == 2**31 - 1).sum()) >= 6
    assert {0, 4294967294} <= set(ref["position"].tolist())
    f = ref["fraction_mod"]
    assert np.isnan(f).sum() == 2 and np.isinf(f).sum() >= 5 and (np.signbit(f) & (f == 0)).sum() >= 2


@pytest.mark.parametrize("case", [r for r in bg.refusals() if r[3] != "a line longer than"], ids=lambda r: r[0])
def test_host_reader_refuses_what_the_reference_refuses(tmp_path, case):
    name, text, _, words = case
    path = str(tmp_path / "r.bed")
    open(path, "wb").write(text)
    for counts_too, threads in ((False, 1), (True, 2)):
        if words is None:
            bg.assert_rows_equal(host_rows(path, counts_too, threads), bg.reference_parse(text, counts_too), counts_too)
        else:
            with pytest.raises(bg.Refused, match=words):
                bg.reference_parse(text, counts_too)
            with pytest.raises(_lib.NmScanError, match=words):
                host_rows(path, counts_too, threads)


def test_ingest_columns_clamp_the_coverage(tmp_path):
    """the reader's own 32-bit coverage column (NativePileup.ingest_columns) against the reference: negative -> -1, above 2^31 - 1 -> 2^31 - 1"""
    from nanomotif_amd import pileup as pp
    path = str(tmp_path / "n.bed")
    open(path, "wb").write(bg.number_text())
    ref = bg.reference_parse(bg.number_text())
    t = pp.NativePileup(path, threads=2)
    try:
        got = t.ingest_columns(np.arange(len(t.contig_names), dtype=np.uint32))
        assert got["nvalid_cov"].dtype == np.int32 and np.array_equal(got["nvalid_cov"], ref["nvalid_cov"])
        assert np.array_equal(got["position"], ref["position"])
    finally:
        t.close()


def test_slab_tail_texts_end_in_their_last_slab():
    for name, text in bg.slab_tail_texts().items():
        c = bg.census(text, 65536)
        assert c["slabs"] >= 3, name
        if name.startswith("open_"):
            assert c["open_last_line_of_" + name[5:]] == 1 and bg.slab_cuts(text, 65536)[-2] < len(text) - 130
