"""The text half of csrc/nmbedgpu.hip restated in plain Python: an independent reference parser of the 18-column bedMethyl text, the geometry
the device parser lays over a text (slabs of whole lines, 16 KiB blocks, 64-byte groups, the 128-byte mask of the field split, the rows left to
the host's routines), and the inputs of tests/test_bed_text_geometry_host.py (no GPU: the borders are there, by count; the host reader equals
the reference) and tests/test_gpu_bed_text_geometry.py (the device parser equals the reference, by equality only).

No GPU and no library here.  The grammar is a decision, written out in reference_parse (polars is not installed to be asked)."""
import re

import numpy as np

SLAB_BYTES = 32 << 20                   # csrc/nmbedgpu.hip
BLOCK_BYTES = 16384
GROUP = 64
MASK = 128
GRIDS = (None, 65536, 131072)           # NM_BED_SLAB_BYTES: unset (one slab), and the two the borders are placed for
S = 65536
KNOWN_CODES = {b"m": 0, b"a": 1, b"21839": 2}
NULLS = (b"", b"NA", b"null")
_DECIMAL = re.compile(rb"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?")
_WORDS = re.compile(rb"[+-]?(inf|infinity|nan)", re.IGNORECASE)
_INT = re.compile(rb"-?[0-9]+")
_COUNT = re.compile(rb"[0-9]+")


class Refused(Exception):
    """the file is refused; .words: what the readers' message must contain"""

    def __init__(self, words, row=None):
        super().__init__(words)
        self.words, self.row = words, row


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference parser
# ---------------------------------------------------------------------------------------------------------------------------------------
def percent_value(f: bytes):
    """column 11 -> the stored fraction; None: no number"""
    if f in NULLS:
        return -1.0
    if _DECIMAL.fullmatch(f) or _WORDS.fullmatch(f):
        return float(f) / 100.0
    return None


def lines_of(text: bytes):
    """(offset, line without its line end) of every non-empty line: split on newlines, one trailing carriage return stripped"""
    at = 0
    for raw in text.split(b"\n"):
        line = raw[:-1] if raw.endswith(b"\r") else raw
        if line:
            yield at, line
        at += len(raw) + 1


def reference_parse(text: bytes, counts: bool = False) -> dict:
    """The rows of `text`, or Refused with the refusal of the FIRST bad row in file order; within a row: columns, start, strand, coverage,
    percentage, counts (the host reader's order)."""
    names, ids, others = [], {}, []
    contig, position, mod, strand, nvalid, frac, nmod, ndiff = [], [], [], [], [], [], [], []
    run_row, run_contig, offsets = [], [], []
    last = None
    for row, (at, line) in enumerate(lines_of(text)):
        f = line.split(b"\t")
        if len(f) != 18:
            raise Refused("exactly 18", row)
        if not _INT.fullmatch(f[1]):
            raise Refused("column 2", row)
        pos = int(f[1])
        if pos < 0:
            raise Refused("negative", row)
        if pos > 4294967294:
            raise Refused("beyond 4 Gbp", row)
        if f[5] not in (b"+", b"-"):
            raise Refused("column 6", row)
        if f[9] in NULLS:
            cov = -1
        elif _INT.fullmatch(f[9]):
            cov = int(f[9])
            cov = -1 if cov < 0 else min(cov, 2**31 - 1)
        else:
            raise Refused("column 10", row)
        pct = percent_value(f[10])
        if pct is None:
            raise Refused("column 11", row)
        if f[3] in KNOWN_CODES:
            mt = KNOWN_CODES[f[3]]
        else:
            if f[3] not in others:
                others.append(f[3])
            mt = 3 + others.index(f[3])
        if counts:
            for k in (11, 16):
                if not _COUNT.fullmatch(f[k]) or int(f[k]) > 2**31 - 1:
                    raise Refused("column 12", row)
            nmod.append(int(f[11]))
            ndiff.append(int(f[16]))
        if f[0] != last:
            last = f[0]
            if last not in ids:
                ids[last] = len(names)
                names.append(last)
            run_row.append(row)
            run_contig.append(ids[last])
        contig.append(ids[last]); position.append(pos); mod.append(mt); strand.append(f[5][0]); nvalid.append(cov); frac.append(pct)
        offsets.append(at)
    out = dict(names=[n.decode() for n in names], other_codes=[c.decode() for c in others], contig=np.array(contig, np.uint32),
               position=np.array(position, np.uint32), mod_type=np.array(mod, np.int8), strand=np.array(strand, np.uint8),
               nvalid_cov=np.array(nvalid, np.int32), fraction_mod=np.array(frac, np.float64), run_row=np.array(run_row + [len(contig)], np.uint64),
               run_contig=np.array(run_contig, np.uint32), offsets=np.array(offsets, np.int64))
    if counts:
        out["nmod"], out["ndiff"] = np.array(nmod, np.int32), np.array(ndiff, np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the geometry restated
# ---------------------------------------------------------------------------------------------------------------------------------------
def slab_size(grid):
    return SLAB_BYTES if grid is None else min(SLAB_BYTES, max(65536, grid))


def slab_cuts(text: bytes, grid=None):
    """[0, end of slab 0, ...]: a slab ends behind the last newline within slab_size bytes of its start (the text's end: as it is)"""
    size, cuts = slab_size(grid), [0]
    while cuts[-1] < len(text):
        e = min(len(text), cuts[-1] + size)
        if e < len(text):
            k = text.rfind(b"\n", cuts[-1], e)
            if k < 0:
                raise Refused("a line longer than")
            e = k + 1
        cuts.append(e)
    return cuts


def fast_path(f: bytes) -> bool:
    """the kernel decides this percentage itself (Clinger's fast path): sign, digits with at most one dot, mantissa < 2^53, <= 22 decimals"""
    q = f[1:] if f[:1] in (b"+", b"-") else f
    mant = ndig = dec = 0
    dot = False
    for c in q:
        if 48 <= c <= 57:
            if mant > (2**64 - 1 - 9) // 10:
                return False
            mant = mant * 10 + c - 48
            dec += dot
            ndig += 1
        elif c == 46 and not dot:
            dot = True
        else:
            return False
    return ndig > 0 and mant < 2**53 and dec <= 22


def host_flags(line: bytes) -> int:
    """1: the mod code, 2: the percentage is left to the host's routines (a valid row)"""
    f = line.split(b"\t")
    return (0 if f[3] in KNOWN_CODES else 1) | (0 if f[10] in NULLS or fast_path(f[10]) else 2)


def census(text: bytes, grid) -> dict:
    """what of the borders the device parser has lies in `text` when it is cut into slabs of `grid` bytes, by count"""
    from collections import Counter
    c = Counter()
    cuts = slab_cuts(text, grid)
    size = slab_size(grid)
    c["slabs"] = len(cuts) - 1
    seen_names, prev_name, prev_slab_had_rows, empty_since_rows = set(), None, False, False
    rows_so_far = 0
    for k in range(len(cuts) - 1):
        lo, hi = cuts[k], cuts[k + 1]
        slab, n, last_slab = text[lo:hi], hi - lo, k == len(cuts) - 2
        # ---- slab ends
        if not last_slab:
            if hi == lo + size:
                c["line_ends_on_nominal_end"] += 1
            else:
                end = text.find(b"\n", hi)
                end = len(text) if end < 0 else end + 1
                over = end - (lo + size)                                    # bytes of the straddling line beyond the nominal end
                c["straddle_by_1"] += over == 1
                c["straddle_over_4096"] += over > 4096
                c["straddle_20000_line"] += end - hi >= 20000
        # ---- line starts
        lines = list(lines_of(slab))
        starts = [o for o, _ in lines]
        for o in starts:
            if o % GROUP in (0, 1, 63):
                c["start_on_group_byte_%d" % (o % GROUP)] += 1
            if o % BLOCK_BYTES in (0, BLOCK_BYTES - 1):
                c["start_on_block_byte_%d" % (o % BLOCK_BYTES)] += 1
            c["newline_on_63_start_on_0"] += o % GROUP == 0 and o > 0
            c["newline_on_16383_start_on_0"] += o % BLOCK_BYTES == 0 and o > 0
        for m in re.finditer(rb"\n(?=\n)", slab):                           # "\n\n": the second newline is an empty line
            i = m.start() + 1
            c["nn_inside_group"] += i % GROUP != 0
            c["nn_on_63_64"] += i % GROUP == 0
            c["nn_on_16383_16384"] += i % BLOCK_BYTES == 0
            c["nn_ends_text"] += last_slab and i == n - 1
        for m in re.finditer(rb"(?:^|(?<=\n))\r(?=\n|$)", slab):            # "\r\n" alone (or "\r" alone at the text's end)
            i = m.start()
            c["rn_inside_group"] += i % GROUP != GROUP - 1
            c["rn_on_63_64"] += i % GROUP == GROUP - 1
            c["rn_on_16383_16384"] += i % BLOCK_BYTES == BLOCK_BYTES - 1
            c["rn_ends_text"] += last_slab and i == n - 2
        groups = {o // GROUP for o in starts}
        blocks = {o // BLOCK_BYTES for o in starts}
        c["groups_without_start"] += (n + GROUP - 1) // GROUP - len(groups)
        c["blocks_without_start"] += (n + BLOCK_BYTES - 1) // BLOCK_BYTES - len(blocks)
        if last_slab:
            c["text_ends_" + ("rn" if text.endswith(b"\r\n") else "n" if text.endswith(b"\n") else "open")] += 1
        # ---- field split
        walk = []
        for o, line in lines:
            raw_end = slab.find(b"\n", o)
            ln = (raw_end if raw_end >= 0 else n) - o                        # the line as the kernel sees it: up to its newline, '\r' included
            w = not (ln < MASK or n - o <= MASK)
            walk.append(w)
            c["mask_lines"] += not w
            c["walk_lines"] += w
            if raw_end >= 0 and ln in (63, 64, 79, 80, 95, 96, 111, 112, 126, 127, 128, 129):
                c["newline_on_line_byte_%d" % ln] += 1
            elif raw_end < 0 and ln in (127, 128, 129):
                c["open_last_line_of_%d" % ln] += 1
            tabs = [i for i, b in enumerate(slab[o:o + ln]) if b == 9]
            if len(tabs) == 17:
                for t in tabs:
                    if t in (63, 64):
                        c["tab_on_line_byte_%d" % t] += 1
                if tabs[10] in (63, 64):
                    c["tab11_on_line_byte_%d" % tabs[10]] += 1
                if tabs[16] in (63, 64, 127, 128):
                    c["tab17_on_line_byte_%d" % tabs[16]] += 1
                c["tab17_beyond_mask"] += tabs[16] > MASK
                f = line.split(b"\t")
                for col in (9, 10):
                    for sp in NULLS:
                        c["null_%r_in_column_%d" % (sp.decode(), col + 1)] += f[col] == sp
                c["crlf_rows"] += slab[o + ln - 1:o + ln] == b"\r"
                fl = host_flags(line)
                c["rows_for_host"] += fl != 0
                c["host_both_flags"] += fl == 3
                if fl & 1:
                    c["host_code_" + f[3].decode()] += 1
                c["host_exponent"] += bool(fl & 2) and (b"e" in f[10].lower())
                c["host_first_row_of_slab"] += fl != 0 and o == starts[0]
                c["host_last_row_of_slab"] += fl != 0 and o == starts[-1]
                if fl and ln + 1 in (1022, 1023, 1024, 1025, 1026):
                    c["host_line_of_%d" % (ln + 1)] += 1
        for w0 in range(0, len(walk) - 63, 64):
            wave = walk[w0:w0 + 64]
            c["wave_one_walk_line"] += sum(wave) == 1
            c["wave_one_mask_line"] += sum(wave) == 63
        # ---- runs
        names = [line.split(b"\t")[0] for _, line in lines]
        if not names:
            c["slabs_without_rows"] += 1
            c["slab_without_rows_between_rows"] += prev_slab_had_rows and any(True for _ in lines_of(text[hi:]))
            empty_since_rows = True
            continue
        c["most_lines_in_a_slab"] = max(c["most_lines_in_a_slab"], len(names))
        for i, nm in enumerate(names):
            before = names[i - 1] if i else prev_name
            change = before != nm
            if change:
                nxt = names[i + 1] if i + 1 < len(names) else None
                c["runs"] += 1
                c["run_comes_back"] += nm in seen_names
                seen_names.add(nm)
                c["change_on_line_255"] += i % 256 == 255
                c["change_on_line_256"] += i % 256 == 0 and i > 0
                c["change_on_first_row_of_slab"] += i == 0 and k > 0
                c["change_on_last_row_of_slab"] += i == len(names) - 1
                c["one_row_run_inside_slab"] += nxt is not None and nxt != nm
                if i == 0 and len(nm) in (63, 64):
                    c["name_of_%d_starts_slab" % len(nm)] += 1
                if before is not None:
                    c["names_differ_in_last_byte"] += len(before) == len(nm) and before[:-1] == nm[:-1]
                    c["names_differ_in_length"] += before != nm and (before.startswith(nm) or nm.startswith(before))
            elif i == 0 and k > 0:
                c["contig_continues_across_slabs"] += 1
                c["contig_continues_across_empty_slab"] += empty_since_rows
        prev_name, prev_slab_had_rows, empty_since_rows = names[-1], True, False
        rows_so_far += len(names)
    return dict(c)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def fields(contig=b"ctgA", start=0, code=b"m", strand=b"+", cov=b"12", pct=b"50.00", nmod=b"6", ndiff=b"0", last=b"0"):
    s = str(start).encode() if isinstance(start, int) else start
    e = str(int(s) + 1).encode() if _COUNT.fullmatch(s) and len(s) < 12 else b"1"
    return [contig, s, e, code, b"12", strand, s if len(s) < 12 else b"0", e, b"0", cov, pct, nmod, b"6", b"0", b"0", b"0", ndiff, last]


def fit(f, length, pad=8):
    """the row of fields f as a line of exactly `length` bytes, its newline not counted: field `pad` is filled up with digits"""
    have = sum(len(x) for x in f) + 17
    assert have <= length, (have, length)
    f = list(f)
    f[pad] = f[pad] + b"0" * (length - have)
    return b"\t".join(f)


def tab_at(f, k, index, pad):
    """the row with its k-th tab (1-based) on byte `index` of the line: field `pad` (before that tab) is filled up"""
    f = list(f)
    have = sum(len(x) for x in f[:k]) + k - 1
    assert have <= index and pad < k
    f[pad] = f[pad] + b"0" * (index - have)
    return b"\t".join(f)


class Builder:
    def __init__(self):
        self.buf = bytearray()
        self.k = 0
        self.contig = b"ctgA"
        self.marks = {}

    @property
    def at(self):
        return len(self.buf)

    def filler_fields(self, **kw):
        self.k += 1
        k = self.k
        row = dict(contig=self.contig, start=3 * k, code=(b"m", b"a", b"21839")[k % 3], strand=b"+-"[k % 2:k % 2 + 1], cov=str(k % 97).encode(),
                   pct=b"%.2f" % ((k * 37 % 10001) / 100), nmod=str(k % 13).encode(), ndiff=str(k % 5).encode())
        row.update(kw)
        return fields(**row)

    def line(self, data: bytes, eol=b"\n"):
        self.buf += data + eol

    def filler(self, n=1, **kw):
        for _ in range(n):
            self.line(b"\t".join(self.filler_fields(**kw)))

    def fill_to(self, target):
        """filler rows up to exactly `target`: the next line starts there"""
        while self.at < target:
            f = self.filler_fields()
            natural, room = sum(len(x) for x in f) + 18, target - self.at
            assert room >= natural, (target, self.at)
            self.line(b"\t".join(f) if room >= 2 * natural + 16 else fit(f, room - 1))
        assert self.at == target

    def next_on(self, residue, modulus=GROUP, room=90):
        """filler rows until the next line starts on byte `residue` of a group (of a block)"""
        t = self.at + room
        t += (residue - t) % modulus
        self.fill_to(t)


_GEOMETRY = None


def geometry_text() -> bytes:
    global _GEOMETRY
    if _GEOMETRY is None:
        _GEOMETRY = _build_geometry()
    return _GEOMETRY


def _build_geometry() -> bytes:
    b = Builder()
    # ---- [0, 65536): slab 0 of every grid starts on byte 0 of the text, so groups and blocks lie alike in all three
    b.line(b"\t".join(b.filler_fields(code=b"h")))                       # row 0: starts on byte 0, and is a row for the host's routines
    # runs: a change on line 255 and on line 256 of the slab, one-row runs, names that differ in the last byte and in length only
    b.filler(253)
    assert b.buf.count(b"\n") == 254
    b.filler(contig=b"ctgA")                                             # line 254
    b.filler(contig=b"ctgB1")                                            # line 255: a change, a one-row run
    b.filler(contig=b"ctgB2")                                            # line 256: a change; differs in the last byte
    b.filler(contig=b"ctgB")                                             # differs in length only
    b.filler(contig=b"ctgB2")
    b.contig = b"ctgC"
    # block borders (16 383 | 16 384)
    b.next_on(BLOCK_BYTES - 1, BLOCK_BYTES); assert b.at == BLOCK_BYTES - 1      # a line starts on the last byte of a block
    b.filler()
    # line starts inside the 64-byte groups
    for residue in (0, 63, 1):
        b.next_on(residue)
        b.filler()
    b.next_on(20); b.line(b"")                                           # "\n\n" inside a group
    b.next_on(0); b.line(b"")                                            # the first newline on byte 63, the second on byte 64
    b.next_on(20); b.line(b"\r")                                         # "\r\n" alone inside a group
    b.next_on(63); b.line(b"\r")                                         # the '\r' on byte 63, the '\n' on byte 64
    b.next_on(0, BLOCK_BYTES)                                            # newline on 16 383, start on byte 0 of the next block
    b.filler()
    b.next_on(BLOCK_BYTES - 1, BLOCK_BYTES)
    b.line(b"\r")                                                        # "\r\n" alone across the block border
    # the field split: where the line ends (every 16-byte piece's border, and the mask's), open and CRLF rows
    for ln in (63, 64, 79, 80, 95, 96, 111, 112, 126, 127, 128, 129):
        b.line(fit(b.filler_fields(), ln))
    for ln in (126, 127, 128, 129):
        b.line(fit(b.filler_fields(), ln - 1), eol=b"\r\n")              # the '\r' in the eighteenth field
    b.line(tab_at(b.filler_fields(), 11, 63, 4)); b.line(tab_at(b.filler_fields(), 11, 64, 4))
    for index in (63, 64, 127, 128, 140):
        b.line(tab_at(b.filler_fields(), 17, index, 13))
    b.line(tab_at(b.filler_fields(last=b""), 17, 127, 13))               # the last tab is the line's last byte (an empty eighteenth field)
    for cov in NULLS:
        for pct in NULLS:
            b.filler(cov=cov, pct=pct)
    # rows for the host's routines
    for code, pct in ((b"h", b"1.50"), (b"17596", b"2.5"), (b"21839x", b"3"), (b"m", b"1e1"), (b"a", b"2.5E-1"), (b"h", b"1e2"), (b"17596", b"12345678901234567890.5")):
        b.filler(code=code, pct=pct)
    for ln in (1021, 1022, 1023, 1024, 1025):                            # field_in reads 1024 bytes first: the newline inside | behind them
        b.line(fit(b.filler_fields(code=b"h", pct=b"7e0"), ln))
    assert b.at < S - 400, b.at
    b.fill_to(S)                                                         # grid 65 536: a line ends exactly on the nominal slab end
    # ---- [65536, 131072): block 1 of this stretch has no line start at all (one row with a contig name of 20 000 bytes)
    b.next_on(0, BLOCK_BYTES); assert b.at == S + BLOCK_BYTES
    b.line(b""); assert b.at % BLOCK_BYTES == 1                          # "\n\n" across a block border: 16 383 | 16 384
    b.fill_to(S + 2 * BLOCK_BYTES - 100)
    b.filler(contig=b"L" * 20000)
    b.filler(2)
    b.fill_to(2 * S)                                                     # both grids: a line ends exactly on the nominal slab end
    # ---- [131072, ...): the slab ends that are not the nominal ones
    # a wave of 64 lines with one mask-path line among walk-path lines, whichever
    # line of the slab the wave begins on
    for k in range(127):
        b.line(fit(b.filler_fields(), 131 if k != 63 else 100))
    b.filler(63); b.line(fit(b.filler_fields(), 131)); b.filler(63)       # ... and one walk-path line among mask-path lines
    b.fill_to(3 * S - 70)
    b.line(fit(b.filler_fields(), 70))                                   # its newline is byte 3 S: grid 65 536 cuts 70 bytes early
    a = 3 * S - 70
    b.fill_to(a + S - 100)                                               # the 20 000-byte name again, across the ends of both grids' slabs
    b.filler(contig=b"L" * 20000, code=b"17596")                         # (first row of a slab, for the host's routines, name longer than a slot)
    start_b = a + S - 100
    b.marks["b"] = start_b
    # a slab that holds only empty lines (grid 65 536) between two slabs with rows; the contig goes on behind it
    # (a line the inflate path's slabs of 70 000 bytes cut far from its end when the BGZF blocks hold 65 280 bytes; with blocks of 777
    #  bytes the 20 000-byte line above is one)
    b.fill_to(5 * 0xFF00 - 5500)
    b.filler(contig=b"T" * 6000)
    assert b.at < start_b + S - 500
    b.fill_to(start_b + S - 300)
    b.buf += b"\n" * (S + 400)
    c0 = start_b + 2 * S
    b.fill_to(c0 + 200)
    # from c0 the slabs of both grids begin on the same bytes again
    def border(at, name):
        b.fill_to(at - 200)
        b.line(fit(b.filler_fields(contig=b"one_" + name[:8], code=b"h"), 199))        # last row of the slab: a change, a one-row run, for the host
        assert b.at == at
        b.contig = name
        b.filler(code=b"a", pct=b"5e0")                                  # first row of the slab: a change, for the host's routines
    border(c0 + S, b"n" * 64)
    c1 = c0 + 2 * S - 140                                                # both grids: a line whose newline is the byte behind the nominal end;
    b.fill_to(c1)                                                        # it becomes the first row of the next slab, a run with a name of 63 bytes
    b.contig = b"m" * 63
    b.line(fit(b.filler_fields(), 140))
    border(c1 + S, b"k" * 63)
    border(c1 + 2 * S, b"j" * 64)
    b.contig = b"ctgA"                                                   # a contig that comes back
    b.filler(40)
    b.filler(3)
    b.line(fit(b.filler_fields(contig=b"last", code=b"h"), 129), eol=b"")      # the last row: a one-row run, for the host, 129 bytes, no line end
    return bytes(b.buf)


def tail_texts():
    """short texts for the ends a text can have only one of"""
    b = Builder()
    b.filler(5)
    head = bytes(b.buf)
    out = {"newline": head, "crlf": head.replace(b"\n", b"\r\n"), "nn": head + b"\n", "rn_alone": head + b"\r\n", "r_alone": head + b"\r"}
    for ln in (127, 128, 129):
        out["open_%d" % ln] = head + fit(b.filler_fields(), ln)
    return out


_NUMBERS = None


def number_strings():
    rng = np.random.default_rng(20240611)
    out = ["%.2f" % (k / 100) for k in range(10001)]
    for _ in range(20000):
        nd = int(rng.integers(1, 26))
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
        dec = int(rng.integers(0, min(nd, 24) + 1))
        sign = ("", "", "-", "+")[int(rng.integers(0, 4))]
        out.append(sign + (digits[:nd - dec] + "." + digits[nd - dec:] if dec else digits))
    for m in (2**53 - 1, 2**53, 2**53 + 1):
        out += [str(m), str(m) + ".0", "0." + str(m), str(m)[:3] + "." + str(m)[3:]]
    for dec in range(0, 26):
        out.append("0." + "0" * (dec - 1) + "7" if dec else "7")
        for sig in (15, 16, 17):
            if dec >= sig:
                out.append("0." + "0" * (dec - sig) + "123456789012345678"[:sig])
            else:
                out.append("123456789012345678"[:sig - dec] + "." + "123456789012345678"[sig - dec:sig] if dec else "123456789012345678"[:sig])
    out += ["1" * 19, "1" * 20, "1" * 21, "9" * 19, "18446744073709551615", "18446744073709551616", "1844674407370955161", "1844674407370955162"]
    out += ["000000000000000000000012.5", "0000000000000000000000000.25", "00.50", "9007199254740.99200000", "90071992547409.9300000", "900719925474099.10000"]
    out += ["-0", "-0.0", "+1.5", ".5", "5.", "1e2", "1E-2", "1e400", "inf", "-Infinity", "nan", "1e+2", "-1.5e-3", "INF", "NaN", "+inf"]
    return out


def number_text() -> bytes:
    global _NUMBERS
    if _NUMBERS is None:
        covs = ["0", str(2**31 - 2), str(2**31 - 1), str(2**31), "4000000000", str(2**63 - 1), str(2**63), str(2**64 + 7), "-3", "-0", "007"]
        rows = []
        for k, s in enumerate(number_strings()):
            start = (0, 4294967294)[k % 2] if k < 4 else k
            cov = covs[k % len(covs)] if k % 50 == 0 else str(k % 90)
            rows.append("c\t%d\t%d\tm\t1\t+\t\t\t\t%s\t%s\t%d\t\t\t\t\t%d\t\n" % (start, start + 1, cov, s, k % 7, k % 3))
        _NUMBERS = "".join(rows).encode()
    return _NUMBERS


def good_rows(n, contig=b"g"):
    b = Builder()
    b.contig = contig
    b.filler(n)
    return bytes(b.buf)


_MANY = None


def many_rows() -> bytes:
    """3000 plain rows: three slabs of 65 536 bytes (the refusals' several-slab files are cut out of it)"""
    global _MANY
    if _MANY is None:
        _MANY = good_rows(3000)
    return _MANY


def slab_tail_texts():
    """many_rows() with each end a text can have as the end of its LAST slab: an open last line of 127 | 128 | 129 bytes takes the mask path
    through "at most 128 bytes left in the slab" there"""
    many = many_rows()
    b = Builder()
    b.contig = b"g"
    out = {"newline": many, "crlf": many[:-1] + b"\r\n", "nn": many + b"\n", "rn_alone": many + b"\r\n"}
    for ln in (127, 128, 129):
        out["open_%d" % ln] = many + fit(b.filler_fields(), ln)
    return out


def refusals():
    """(name, text, NM_BED_SLAB_BYTES or None, the words of the refusal or None when the file is read)"""
    head = good_rows(5)
    row = lambda **kw: b"\t".join(fields(contig=b"g", **{"start": 7, **kw})) + b"\n"
    out = []
    for tag, start, words in (("lone_minus", b"-", "column 2"), ("plus_5", b"+5", "column 2"), ("4294967295", b"4294967295", "beyond 4 Gbp"),
                              ("2_32", str(2**32).encode(), "beyond 4 Gbp"), ("2_64_10", str(2**64 + 10).encode(), "beyond 4 Gbp"),
                              ("2_63", str(2**63).encode(), "beyond 4 Gbp"), ("minus_1", b"-1", "negative"), ("minus_2_64", str(-2**64 - 1).encode(), "negative")):
        out.append(("start_" + tag, head + row(start=start) + head[:0], None, words))
    for tag, cov in (("lone_minus", b"-"), ("9x", b"9x"), ("plus", b"+9")):
        out.append(("coverage_" + tag, head + row(cov=cov), None, "column 10"))
    for tag, pct in (("hex", b"0x10"), ("blank", b" 1.5"), ("nan_paren", b"nan(1)"), ("dot", b"."), ("minus", b"-"), ("two_dots", b"1.0.0"),
                     ("e_alone", b"1e"), ("hex_float", b"0x1p3"), ("blank_behind", b"1.5 "), ("two_signs", b"+-1")):
        out.append(("percent_" + tag, head + row(pct=pct), None, "column 11"))
    good = fields(contig=b"g", start=7)
    out.append(("columns_17", head + b"\t".join(good[:17]) + b"\n", None, "exactly 18"))
    out.append(("columns_19", head + b"\t".join(good + [b"0"]) + b"\n", None, "exactly 18"))
    out.append(("line_of_15", head + b"g\t1\t2\tm\t1\t+\t1\t2\n", None, "exactly 18"))          # (a valid row has 17 tabs: no valid line is that short)
    out.append(("line_of_16", head + b"g\t1\t2\tm\t1\t+\t1\t22\n", None, "exactly 18"))
    out.append(("strand_and_coverage", head + row(strand=b".", cov=b"9x"), None, "column 6"))
    # the order of refusals
    bad_strand, bad_start, host_pct = row(strand=b"."), row(start=b"x"), row(pct=b"1.0.0")
    out.append(("two_kernel_faults", head + bad_strand + head + bad_start, None, "column 6"))
    out.append(("host_before_kernel", head + host_pct + head + bad_strand, None, "column 11"))
    out.append(("kernel_before_host", head + bad_strand + head + host_pct, None, "column 6"))
    # several slabs (grid 65 536): the bad row's number counts the rows of the slabs before it
    many = many_rows()
    assert len(many) > 2 * S + 1000
    cut1 = many.rfind(b"\n", 0, S + 3000) + 1
    cut2 = many.rfind(b"\n", 0, 2 * S + 500) + 1
    out.append(("second_slab", many[:cut1] + bad_strand + many[cut1:], S, "column 6"))
    out.append(("last_slab", many + bad_start, S, "column 2"))
    out.append(("host_in_slab_1_kernel_in_slab_2", many[:cut1] + row(pct=b"0x10") + many[cut1:cut2] + bad_strand + many[cut2:], S, "column 11"))
    out.append(("kernel_in_slab_1_host_in_slab_2", many[:cut1] + bad_start + many[cut1:cut2] + row(pct=b"0x10") + many[cut2:], S, "column 2"))
    out.append(("kernel_in_slab_2_kernel_in_slab_1", many[:cut1] + bad_strand + many[cut1:cut2] + bad_start + many[cut2:], S, "column 6"))
    long_line = head + b"\t".join(fields(contig=b"W" * 70000, start=9, code=b"h", pct=b"1e1")) + b"\n" + head
    out.append(("line_longer_than_the_slab", long_line, S, "a line longer than"))
    out.append(("line_longer_than_the_slab_unset", long_line, None, None))
    return out


def inflate_slab_tails(text: bytes, block: int, slab: int = 70000):
    """the bytes behind the last newline of every slab but the last when the device-inflate path cuts a bgzip file of `block`-byte members
    into slabs of at most `slab` bytes of text (NM_BED_INFLATE_SLAB): what bed_tail_kernel walks back over"""
    step = slab // block * block
    return [e - (text.rfind(b"\n", 0, e) + 1) for e in range(step, len(text), step)]


def assert_rows_equal(got: dict, ref: dict, counts: bool = False):
    """a reader's rows against reference_parse's, by equality only: names and their order, the other codes and their order, every column,
    the fractions by their bits"""
    assert got["names"] == ref["names"]
    assert got["other_codes"] == ref["other_codes"]
    assert len(got["position"]) == len(ref["position"])
    for k in ("contig", "position", "mod_type", "strand", "nvalid_cov") + (("nmod", "ndiff") if counts else ()):
        bad = np.flatnonzero(np.asarray(got[k]).astype(np.int64) != ref[k].astype(np.int64))
        assert len(bad) == 0, (k, bad[:5].tolist(), np.asarray(got[k])[bad[:5]].tolist(), ref[k][bad[:5]].tolist())
    a, b = np.ascontiguousarray(got["fraction_mod"]).view(np.uint64), ref["fraction_mod"].view(np.uint64)
    bad = np.flatnonzero(a != b)
    assert len(bad) == 0, ("fraction_mod", bad[:5].tolist(), got["fraction_mod"][bad[:5]].tolist(), ref["fraction_mod"][bad[:5]].tolist())


def geometry_text_crlf() -> bytes:
    """geometry_text() with "\\r\\n" line ends (a line that has one keeps it)"""
    return re.sub(rb"(?<!\r)\n", b"\r\n", geometry_text())
