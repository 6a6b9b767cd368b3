"""The device inflate (csrc/nmbedinflate.h: bed_inflate_kernel, bed_tokens_kernel / bed_resolve_kernel, bed_crc_kernel) on DEFLATE
streams zlib never writes: the zoo of tests/deflate_streams.py — one hand-built BGZF member per edge of the decoders, see the table
there — parsed by DevicePileup under every inflate path and compared row by row with the host reader, which inflates with zlib.
The repetitions the edges need stand in the colour column, which no parser reads: a wrong byte there changes no row and is caught by
bed_crc_kernel against the member's trailer, so everything here runs with the CRC check on (the default; nothing turns it off).
tests/test_deflate_streams_host.py shows on the CPU that every edge is in the bytes."""
import os
import re

import pytest

import deflate_streams as ds
from nanomotif_amd import pileup as pp
from helpers import assert_same_rows as _assert_same_rows

pytestmark = pytest.mark.gpu

# At the default token fraction (5/8) phase 1 gives up the stored and the literals_* members (and the tiny ones) by construction, next to
# two-phase neighbours; every other member's tokens fit (tests/test_deflate_streams_host.py asserts both).  NM_BED_TOKEN_FRACTION=1.5
# gives every member its worst-case region: the stored and literal-only members take the two phases too.
ENVS = [{}, {"NM_BED_INFLATE_V1": "1"}, {"NM_BED_TOKEN_FRACTION": "0.0"}, {"NM_BED_TOKEN_FRACTION": "1.5"}, {"NM_BED_HOST_INFLATE": "1"},
        {"NM_BED_INFLATE_SLAB": "70000"}, {"NM_BED_INFLATE_SLAB": "70000", "NM_BED_INFLATE_V1": "1"}]


def _id(env):
    return "+".join(k[7:] + "=" + v for k, v in env.items()) or "default"


@pytest.fixture(scope="module")
def eng():
    from nanomotif_amd.engine import ScanEngine
    e = ScanEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the zoo as text, as .gz + .tbi, regrouped by kind; the host reader's view of each (the reference, computed once)"""
    tmp = tmp_path_factory.mktemp("zoo")
    zoo = ds.build_zoo()
    f = dict(bed=str(tmp / "zoo.bed"), gz=str(tmp / "zoo.bed.gz"), re_bed=str(tmp / "re.bed"), re_gz=str(tmp / "re.bed.gz"))
    open(f["bed"], "wb").write(zoo.text)
    zoo.write(f["gz"])
    re = zoo.regrouped()
    open(f["re_bed"], "wb").write(re.text)
    re.write_members(f["re_gz"])
    f["plain"], f["re_plain"] = pp.NativePileup(f["bed"]), pp.NativePileup(f["re_bed"])
    f["wanted"] = list(f["plain"].contig_names)[1::2][::-1]
    f["part"] = pp.NativePileup(f["gz"], contigs=f["wanted"], index_path=f["gz"] + ".tbi")
    assert f["part"].indexed
    yield f
    for k in ("plain", "re_plain", "part"):
        f[k].close()


def _device(eng, env, path, **kw):
    os.environ.update(env)
    try:
        return pp.DevicePileup(eng, path, **kw)
    finally:
        for k in env:
            del os.environ[k]


@pytest.mark.parametrize("env", ENVS, ids=_id)
def test_the_zoo_on_the_device_equals_the_host_reader(eng, files, env):
    dev = _device(eng, env, files["gz"])
    _assert_same_rows(dev, files["plain"])
    dev.close()


@pytest.mark.parametrize("env", ENVS, ids=_id)
def test_the_tabix_subset_of_the_zoo(eng, files, env):
    """every other contig: the regions begin and end inside hand-built members, whose whole text goes through the scratch buffer"""
    host = files["part"]
    dev = _device(eng, env, files["gz"], contigs=files["wanted"], index_path=files["gz"] + ".tbi")
    assert dev.indexed and dev.bytes_inflated == host.bytes_inflated and set(dev.contig_names) == set(files["wanted"])
    assert 0 < len(dev) < len(files["plain"])
    _assert_same_rows(dev, host)
    dev.close()


@pytest.mark.parametrize("env", ENVS, ids=_id)
def test_the_members_regrouped_by_kind(eng, files, env):
    """all stored members first, then fixed, dynamic, multi-block: whole waves of one kind"""
    dev = _device(eng, env, files["re_gz"])
    _assert_same_rows(dev, files["re_plain"])
    dev.close()


def test_directed_refusals(eng, tmp_path):
    """Streams that zlib refuses too (tests/deflate_streams.py: refusals, with the traced `inflate error` codes): each is a corrupt BGZF
    block with one of its codes under the two-phase inflate and under the one-lane kernel, and a valid file parses to the right rows on
    the same engine straight afterwards."""
    from nanomotif_amd._lib import NmScanError
    listed, valid, text = ds.refusal_files(str(tmp_path))
    bed = str(tmp_path / "valid.bed")
    open(bed, "wb").write(text)
    plain = pp.NativePileup(bed)
    for name, path, v1, two_phase in listed:
        for env, codes in (({}, two_phase), ({"NM_BED_INFLATE_V1": "1"}, v1)):
            with pytest.raises(NmScanError, match="corrupt BGZF block") as e:
                _device(eng, env, path)
            found = re.search(r"block 3 of the slab, inflate error (\d+)\)", str(e.value))
            assert found and int(found.group(1)) in codes, (name, env, str(e.value), codes)
            dev = _device(eng, env, valid)
            _assert_same_rows(dev, plain)
            dev.close()
    plain.close()
