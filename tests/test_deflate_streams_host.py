"""The hand-built DEFLATE streams of tests/deflate_streams.py on the CPU: every member of the zoo is a valid stream of exactly its text
(zlib is the independent judge), holds the edge it was built for (`inspect` is the witness: a decoder of its own, though it shares the
format's tables and the canonical-code rule with the writer, so an error there would fool both — zlib would not accept the stream), and
the host reader gives the same rows on the .gz as on the plain text — whole file and through the tabix index, whose
regions cut hand-built members in the middle.  The device side is tests/test_gpu_bed_inflate_streams.py."""
import gzip
import hashlib
import zlib

import numpy as np
import pytest

import deflate_streams as ds
from nanomotif_amd import pileup as pp


@pytest.fixture(scope="module")
def zoo():
    return ds.build_zoo()


@pytest.fixture(scope="module")
def inspected(zoo):
    return [ds.inspect_stream(m.stream) for m in zoo.members]


def test_every_member_inflates_with_zlib_to_exactly_its_text(zoo):
    assert len(zoo.members) >= 130 and len(zoo.members) % 64 != 0
    assert 900_000 <= len(zoo.text) <= 2_000_000
    for m in zoo.members:
        d = zlib.decompressobj(-15)
        assert d.decompress(m.stream) == m.text and d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", m.name
        assert ds.expand([t for tokens, _, _ in m.blocks for t in tokens]) == m.text, m.name
    for size in ds.ZOO_SIZES:
        assert any(len(m.text) == size for m in zoo.members), size


def test_inspect_finds_the_edge_of_every_row_of_the_table(zoo, inspected):
    for m, seen in zip(zoo.members, inspected):
        name, size, kinds, planted, edge = m.row
        assert seen["text"] == m.text and len(m.text) == size and seen["consumed"] == len(m.stream), name
        assert [b["type"] for b in seen["blocks"]] == kinds, name
        found = [t for t in seen["tokens"] if isinstance(t, tuple)]
        assert all(t in found for t in planted), name
        assert m.check(seen), (name, edge)
    # the kinds side by side in every wave of 64 members (phase 1 and the one-lane kernel take 64 members per workgroup)
    def kind(seen):
        types = {b["type"] for b in seen["blocks"]}
        return "multi" if len(seen["blocks"]) > 1 else types.pop()
    for first in range(0, len(inspected), 64):
        assert {kind(s) for s in inspected[first:first + 64]} == {"stored", "fixed", "dynamic", "multi"}, first
    # slabs of 70 000 bytes of text (NM_BED_INFLATE_SLAB, cut as csrc/nmbedgpu.hip cuts them): several, every one with a line end in
    # it, and a member that overflows its token region shares a slab with members that do not
    slabs, k = [], 0
    while k < len(zoo.members):
        j, total = k, 0
        while j < len(zoo.members) and (j == k or total + len(zoo.members[j].text) <= 70_000):
            total += len(zoo.members[j].text)
            j += 1
        slabs.append(zoo.members[k:j])
        k = j
    assert len(slabs) >= 10 and all(any(b"\n" in m.text for m in slab) for slab in slabs)
    assert any(len(slab) > 2 and any(m.name.startswith("literals_") for m in slab) for slab in slabs)
    regrouped, total = zoo.regrouped().members, 0
    for k, m in enumerate(regrouped):                      # (the regrouped file: no slab of it without a line end either)
        if total + len(m.text) > 70_000:
            assert any(b"\n" in x.text for x in regrouped[first_of_slab:k])
            total = 0
        if total == 0:
            first_of_slab = k
        total += len(m.text)


def test_which_members_take_the_two_phases(zoo, inspected):
    """The room check of bed_tokens_kernel replayed on every member's tokens: at the default fraction (5/8) phase 1 gives up exactly the
    members that are all literals by construction — stored members, literals_*, texts of a few bytes — so every other edge is decoded by
    bed_tokens_kernel and bed_resolve_kernel and not by the one-lane fallback; with the worst-case region (NM_BED_TOKEN_FRACTION >= 4/3)
    only the six texts of up to 27 bytes cannot fit (56 bytes of slack and a record or two against a region of 48 or 64)."""
    assert ds.token_region_bytes(65280) == 40864 and ds.token_region_bytes(65280, 1.5) == 87072 and ds.token_region_bytes(1, 1.5) == 48
    for m, seen in zip(zoo.members, inspected):
        assert ds.overflows_token_region(seen["tokens"], len(m.text)) == ds.gives_up_by_construction(m), m.name
        assert ds.overflows_token_region(seen["tokens"], len(m.text), 1.5) == (m.name in ds.NEVER_TWO_PHASE), m.name
        assert ds.overflows_token_region(seen["tokens"], len(m.text), 0.0) or len(m.text) <= 65, m.name      # (three literals and a match fit 64 bytes)
    edges = [m for m in zoo.members if not m.name.startswith("rows_")]
    assert sum(1 for m in edges if not ds.gives_up_by_construction(m)) >= 70 and all(max(len(x.text) for x in zoo.members if x.name == n) <= 27
                                                                                      for n in ds.NEVER_TWO_PHASE)


def test_every_length_and_distance_symbol_at_both_ends_of_its_range(inspected):
    lengths = {t[0] for seen in inspected for t in seen["tokens"] if isinstance(t, tuple)}
    dists = {t[1] for seen in inspected for t in seen["tokens"] if isinstance(t, tuple)}
    for s in range(29):
        assert set(ds.length_range(s)) <= lengths, 257 + s
    for s in range(30):
        assert set(ds.dist_range(s)) <= dists, s
    assert ds.length_range(28) == (258, 258) and ds.length_range(27) == (227, 257) and ds.dist_range(29) == (24577, 32768)
    # and the codes: 15 bits in both alphabets, 7 bits in the code-length code, the header fields at both ends
    dyn = [b for seen in inspected for b in seen["blocks"] if b["type"] == "dynamic"]
    assert max(b["max_used_litlen"] for b in dyn) == 15 and max(b["max_used_dist"] for b in dyn) == 15 and max(b["max_used_cl"] for b in dyn) == 7
    assert {257, 286} <= {b["nlen"] for b in dyn} and {1, 30} <= {b["ndist"] for b in dyn} and {5, 19} <= {b["hclen"] for b in dyn}
    assert {16, 17, 18} <= {s for b in dyn for s in b["crossed"]}


def _rows(t):
    cols = {k: v.copy() for k, v in t.ingest_columns(np.arange(len(t.contig_names), dtype=np.uint32)).items()}
    return list(t.contig_names), cols


def _assert_same(a, b):
    assert a[0] == b[0]
    for k in ("contig", "position", "mod_type", "strand", "nvalid_cov"):
        assert np.array_equal(a[1][k], b[1][k]), k
    assert np.array_equal(a[1]["fraction_mod"].view(np.uint64), b[1]["fraction_mod"].view(np.uint64))


def test_host_reader_gives_the_rows_of_the_plain_text(zoo, tmp_path):
    bed, gz = str(tmp_path / "zoo.bed"), str(tmp_path / "zoo.bed.gz")
    open(bed, "wb").write(zoo.text)
    zoo.write(gz)
    assert gzip.open(gz, "rb").read() == zoo.text
    seen = ds.inspect(open(gz, "rb").read())
    assert [s["text"] for s in seen[:-1]] == [m.text for m in zoo.members] and seen[-1]["text"] == b""
    plain, whole = pp.NativePileup(bed), pp.NativePileup(gz)
    rows = _rows(plain)
    assert len(plain) == zoo.text.count(b"\n") and len(rows[0]) >= 8
    _assert_same(_rows(whole), rows)
    whole.close()
    # the tabix subset: every other contig; its regions begin and end inside hand-built members
    wanted = rows[0][1::2][::-1]
    part = pp.NativePileup(gz, contigs=wanted, index_path=gz + ".tbi")
    assert part.indexed and set(part.contig_names) == set(wanted) and 0 < part.bytes_inflated < len(zoo.text)
    got = _rows(part)
    keep = np.isin(rows[1]["contig"], [rows[0].index(n) for n in got[0]])
    lut = np.array([rows[0].index(n) for n in got[0]])
    assert np.array_equal(lut[got[1]["contig"]], rows[1]["contig"][keep])
    for k in ("position", "mod_type", "strand", "nvalid_cov", "fraction_mod"):
        assert np.array_equal(got[1][k], rows[1][k][keep], equal_nan=k == "fraction_mod"), k
    part.close()
    # the members regrouped by kind are another valid pileup
    re_bed, re_gz = str(tmp_path / "re.bed"), str(tmp_path / "re.bed.gz")
    re = zoo.regrouped()
    assert sorted(m.name for m in re.members) == sorted(m.name for m in zoo.members) and re.text != zoo.text
    open(re_bed, "wb").write(re.text)
    re.write_members(re_gz)
    a, b = pp.NativePileup(re_bed), pp.NativePileup(re_gz)
    assert len(a) == len(plain)
    _assert_same(_rows(b), _rows(a))
    a.close(); b.close(); plain.close()


def test_refused_streams_are_refused_by_zlib_and_by_the_host_reader(tmp_path):
    from nanomotif_amd._lib import NmScanError
    kinds = ds.refusals()
    assert len(kinds) == 16
    for name, stream, isize, v1, two_phase, by_zlib in kinds:
        d = zlib.decompressobj(-15)
        if by_zlib:
            with pytest.raises(zlib.error):
                d.decompress(stream)
            with pytest.raises(ValueError):
                ds.inspect_stream(stream)
        else:                                             # a valid stream of another size than the trailer states: the gzip layer refuses
            assert len(d.decompress(stream)) != isize and d.eof
        with pytest.raises((gzip.BadGzipFile, zlib.error)):
            gzip.decompress(ds.bgzf_member(stream, b"", crc=0, isize=isize))
        assert v1 and two_phase and v1 <= two_phase, name
    files, valid, text = ds.refusal_files(str(tmp_path))
    bed = str(tmp_path / "valid.bed")
    open(bed, "wb").write(text)
    a, b = pp.NativePileup(bed), pp.NativePileup(valid)
    _assert_same(_rows(b), _rows(a))
    a.close(); b.close()
    for name, path, _, _ in files:
        with pytest.raises(NmScanError, match="corrupt BGZF block"):
            pp.NativePileup(path)


def test_write_bgzf_tabix_with_default_arguments_writes_the_same_bytes_as_before(tmp_path):
    """The writer of tests/helpers.py gained member_sizes / deflate; what it writes without them is pinned here by digest (the bytes of
    the writer before the change, zlib level 6 — test_bed_reader.py pins the same writer to the bench's native one) and by the
    equivalence of the new arguments with the old ones."""
    from helpers import write_bgzf_tabix
    lines = [f"ctg{k // 700}\t{k * 3}\t{k * 3 + 1}\ta\t{k % 50 + 1}\t+\t{k * 3}\t{k * 3 + 1}\t255,0,0\t{k % 50 + 1}\t{k % 100}.00\t1\t2\t0\t0\t0\t0\t0\n" for k in range(3000)]
    text = "".join(lines).encode()
    a = str(tmp_path / "a.bed.gz")
    write_bgzf_tabix(text, a, block_size=40_000)
    # (the digests are zlib's level-6 output: a zlib upgrade may change them for reasons that have nothing to do with helpers.py — the
    #  durable checks are the equivalence below and test_bed_reader.py, which pins the writer to the bench's native one)
    digest = [hashlib.sha1(open(p, "rb").read()).hexdigest() for p in (a, a + ".tbi")]
    assert digest == ["3793ca039a6c506b256aecf39f8258587bfa6f55", "fab5ef32bb704939cf6b33385cda448fc235aea3"]
    b = str(tmp_path / "b.bed.gz")
    sizes = [40_000] * (len(text) // 40_000) + [len(text) % 40_000]

    def deflate(data):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, 0)
        return c.compress(data) + c.flush()
    write_bgzf_tabix(text, b, member_sizes=sizes, deflate=deflate)
    assert open(a, "rb").read() == open(b, "rb").read() and open(a + ".tbi", "rb").read() == open(b + ".tbi", "rb").read()
