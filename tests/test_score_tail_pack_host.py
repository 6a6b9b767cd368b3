"""The work lists of the heavy scoring kernels (nanomotif_amd/csrc/nmscore_worklist.h) on the CPU: tools/worklist_check/driver.cpp
dumps the plain and the packed list of a geometry, and every property the kernel relies on is held against a restatement that walks
the contigs letter by letter.  The driver is an executable of its own; it runs a second time under the address and
undefined-behaviour sanitizers where those link."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tools", "worklist_check", "driver.cpp")
CXX = os.environ.get("CXX", "g++")
CHUNK_BP, STRIP_BP, GAP_BP, CHUNK_WORDS = 8192, 128, 96, 256
NEED_V, PACKED, NO_STRIP = 1 << 30, 1 << 31, 0xFFFFFFFF

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    return exe, subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", *flags, DRIVER, "-o", exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe, built = _build(tmp_path_factory.mktemp("worklist"), "worklist_dump", ["-O2"])
    assert built.returncode == 0, built.stderr
    return exe


def layout(bins, lengths):
    """nm_upload_contigs restated: contigs grouped by bin (stable), from chunk 1, 96 bp of gap behind each, a pad chunk at either end."""
    order = sorted(range(len(bins)), key=lambda i: bins[i])
    chunk, nxt = [0] * len(bins), 1
    for i in order:
        chunk[i] = nxt
        nxt += (lengths[i] + GAP_BP + CHUNK_BP - 1) // CHUNK_BP
    return order, chunk, nxt + 1


def needs_v_by_letter(lengths, chunk, n_chunks):
    """needs_v_kernel restated on a bit per position: 0 iff the chunk and the three words either side of it are valid."""
    valid = np.zeros(n_chunks * CHUNK_BP, dtype=bool)
    for i, n in enumerate(lengths):
        valid[chunk[i] * CHUNK_BP: chunk[i] * CHUNK_BP + n] = True
    out = np.ones(n_chunks, dtype=np.uint8)
    for c in range(1, n_chunks - 1):
        out[c] = not valid[c * CHUNK_BP - GAP_BP: (c + 1) * CHUNK_BP + GAP_BP].all()
    return out


def run_driver(exe, tmp_path, n_bins, seg_chunks, bins, lengths, chunk, n_chunks, needs_v):
    path = tmp_path / "geometry.txt"
    with open(path, "w") as f:
        f.write(f"{n_bins} {seg_chunks} {n_chunks} {len(bins)}\n")
        f.writelines(f"{b} {n} {c}\n" for b, n, c in zip(bins, lengths, chunk))
        f.write(" ".join(str(int(v)) for v in needs_v) + "\n")
    done = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr
    lists, cur = {}, None
    for line in done.stdout.splitlines():
        key, _, rest = line.partition(":") if not line.startswith("list ") else ("list", "", line[5:])
        if key == "list":
            pack, n_entries, n_rows, n_segs = (int(x) for x in rest.split())
            cur = lists[pack] = {"n": (n_entries, n_rows, n_segs)}
        else:
            cur[key] = np.array(rest.split(), dtype=np.int64)
    for wl in lists.values():
        assert (len(wl["entries"]), len(wl["strips"]) // 64, len(wl["segs"]) // 4) == wl["n"]
        wl["segs"] = wl["segs"].reshape(-1, 4)
    return lists


def check_lists(lists, n_bins, seg_chunks, bins, lengths, order, chunk, n_chunks, needs_v):
    """Every property by count, both lists."""
    # letter by letter: the strips that hold a bp of a contig, and how many letters each holds
    letters = {}
    for i, n in enumerate(lengths):
        for p in range(n):
            g = chunk[i] * CHUNK_BP + p
            letters[(i, g // STRIP_BP)] = letters.get((i, g // STRIP_BP), 0) + 1
    strips_of_bin = [set() for _ in range(n_bins)]
    for (i, s) in letters:
        strips_of_bin[bins[i]].add(s)
    per_chunk = {}
    for b in range(n_bins):
        for s in strips_of_bin[b]:
            per_chunk[s // 64] = per_chunk.get(s // 64, 0) + 1
    for pack in (0, 1):
        wl = lists[pack]
        entries, strips, segs, start, count = wl["entries"], wl["strips"], wl["segs"], wl["bin_start"], wl["bin_len"]
        assert len(start) == len(count) == n_bins
        at, seg_at, next_row = 0, 0, 0
        for b in range(n_bins):
            assert start[b] == at, f"bin {b} starts at {start[b]}, the bins before it end at {at}"
            mine = entries[at: at + count[b]]
            at += count[b]
            covered = {}
            full = [e for e in mine if not e & PACKED]
            rows = [e for e in mine if e & PACKED]
            assert list(mine) == full + rows, "packed rows come after the chunk entries"
            if pack == 0:
                assert not rows
            chunks = [e & (NEED_V - 1) for e in full]
            assert chunks == sorted(chunks) and len(set(chunks)) == len(chunks), "chunk entries in contig and chunk order"
            for e, c in zip(full, chunks):
                assert 1 <= c < n_chunks - 1 and bool(e & NEED_V) == bool(needs_v[c]), f"entry {e:#x}: needs_v of chunk {c} is {needs_v[c]}"
                if pack == 1:
                    assert per_chunk.get(c, 0) == 64, f"chunk {c} is a full entry with {per_chunk.get(c, 0)} strips of sequence"
                for s in range(64):
                    covered[c * 64 + s] = covered.get(c * 64 + s, 0) + 1
            tail_strips = sum(1 for s in strips_of_bin[b] if per_chunk[s // 64] < 64)
            if pack == 1:
                assert len(rows) == -(-tail_strips // 64), f"bin {b}: {len(rows)} packed rows for {tail_strips} tail strips"
            listed = []
            for e in rows:
                assert (e & ~PACKED) == next_row, "rows are numbered in list order"
                listed += list(strips[next_row * 64: next_row * 64 + 64])
                next_row += 1
            real = [w for w in listed if w != NO_STRIP]
            assert listed == real + [NO_STRIP] * (len(listed) - len(real)) and len(listed) - len(real) < 64, "left-over lanes close the bin's last row"
            assert real == sorted(real), "strips in contig order"
            for w in real:
                assert w % 4 == 0 and 0 <= w < n_chunks * CHUNK_WORDS, f"strip value {w}"
                assert w // 4 in strips_of_bin[b], f"strip {w // 4} is listed for bin {b} and holds none of its letters"
                covered[w // 4] = covered.get(w // 4, 0) + 1
            for s in strips_of_bin[b]:
                assert covered.get(s, 0) == 1, f"bin {b}: strip {s} is walked {covered.get(s, 0)} times"
            if pack == 1:
                assert set(covered) == strips_of_bin[b], "the packed list walks nothing but strips that hold sequence"
            # segments tile the bin's list
            pos = start[b]
            while pos < start[b] + count[b]:
                x, y, z, w = segs[seg_at]
                assert (x, z, w) == (pos, b, 0) and y == min(seg_chunks, start[b] + count[b] - pos), f"segment {seg_at} = {(x, y, z, w)} at list position {pos}"
                pos += y
                seg_at += 1
        assert at == len(entries) and seg_at == len(segs) and next_row * 64 == len(strips)
    return len(lists[0]["entries"]), len(lists[1]["entries"])


# the geometry of the issue: bin 0 the border lengths; 1 one contig; 2 tails of exactly 64 strips; 3 of 65; 4 no tail at all; 5 a hundred
# short contigs (many tails in one row); 6 no contig
def geometry():
    rng = np.random.Generator(np.random.PCG64(5))
    per_bin = [
        [1, 127, 128, 129, 8191, 8192, 8193, 16384, 16385],
        [5000],
        [CHUNK_BP + 20 * STRIP_BP, 44 * STRIP_BP - 5],
        [CHUNK_BP + 20 * STRIP_BP - 127, 45 * STRIP_BP],
        [CHUNK_BP, 2 * CHUNK_BP],
        [int(x) for x in rng.integers(200, 901, size=100)],
        [],
    ]
    bins, lengths = [], []
    width = max(len(c) for c in per_bin)
    for k in range(width):                              # upload order mixes the bins
        for b, contigs in enumerate(per_bin):
            if k < len(contigs):
                bins.append(b)
                lengths.append(contigs[k])
    return len(per_bin), bins, lengths


@pytest.mark.parametrize("seg_chunks", [16, 4, 1])
def test_lists_against_the_letters(dump_exe, tmp_path, seg_chunks):
    n_bins, bins, lengths = geometry()
    order, chunk, n_chunks = layout(bins, lengths)
    needs_v = needs_v_by_letter(lengths, chunk, n_chunks)
    lists = run_driver(dump_exe, tmp_path, n_bins, seg_chunks, bins, lengths, chunk, n_chunks, needs_v)
    plain, packed = check_lists(lists, n_bins, seg_chunks, bins, lengths, order, chunk, n_chunks, needs_v)
    wl = lists[1]
    rows = [int((wl["entries"][wl["bin_start"][b]: wl["bin_start"][b] + wl["bin_len"][b]] & PACKED != 0).sum()) for b in range(n_bins)]
    short = sum(-(-n // STRIP_BP) for b, n in zip(bins, lengths) if b == 5)
    assert rows[2] == 1 and rows[3] == 2 and rows[4] == 0 and rows[5] == -(-short // 64) >= 4 and rows[1] == 1
    assert wl["bin_len"][6] == 0 and wl["bin_len"][4] == 3 and wl["bin_len"][5] == rows[5]
    # bin 0: 1, 127, 128 bp one strip each, 129 two, 8193 and 16385 one behind their full chunks: 7 tail strips, one row; 8191 bp fill the
    # 64 strips of a chunk, so with 8192, 8193 (one each), 16384 and 16385 (two each) there are 7 full chunks
    assert rows[0] == 1 and wl["bin_len"][0] == 7 + 1
    assert plain > packed


def test_totals_of_the_benchmark_configurations(dump_exe, tmp_path):
    from nanomotif_amd import synth
    for name, plain_want, packed_want in (("cfg5", 127_084, 122_395), ("cfg3", 12_714, 12_239)):
        mg = synth.make_metagenome(synth.config(name))
        lengths = [int(x) for x in mg.lengths]
        names = sorted(set(mg.bin_names))
        bins = [names.index(b) for b in mg.bin_names]
        order, chunk, n_chunks = layout(bins, lengths)
        lists = run_driver(dump_exe, tmp_path, len(names), 16, bins, lengths, chunk, n_chunks, np.ones(n_chunks, dtype=np.uint8))
        assert len(lists[0]["entries"]) == plain_want and len(lists[1]["entries"]) == packed_want
        # from the lengths alone
        L = np.array(lengths, dtype=np.int64)
        full, tail = L // CHUNK_BP, -(-(L % CHUNK_BP) // STRIP_BP)
        assert int(full.sum() + (tail > 0).sum()) == plain_want
        assert int(full.sum()) + sum(-(-int(tail[np.array(bins) == b].sum()) // 64) for b in range(len(names))) == packed_want
        for pack in (0, 1):                             # segments tile the lists here too
            segs, start, count = lists[pack]["segs"], lists[pack]["bin_start"], lists[pack]["bin_len"]
            assert int(segs[:, 1].sum()) == len(lists[pack]["entries"]) and len(segs) == int((-(-count // 16)).sum())
            assert (segs[1:, 0] == segs[:-1, 0] + segs[:-1, 1]).all() and (start[segs[:, 2]] <= segs[:, 0]).all()


def test_lists_under_address_and_undefined_sanitizers(tmp_path):
    exe, built = _build(tmp_path, "worklist_dump_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the sanitizer runtimes do not link here")
    assert built.returncode == 0, built.stderr
    n_bins, bins, lengths = geometry()
    order, chunk, n_chunks = layout(bins, lengths)
    needs_v = needs_v_by_letter(lengths, chunk, n_chunks)
    for seg_chunks in (16, 3):
        lists = run_driver(exe, tmp_path, n_bins, seg_chunks, bins, lengths, chunk, n_chunks, needs_v)
        check_lists(lists, n_bins, seg_chunks, bins, lengths, order, chunk, n_chunks, needs_v)
