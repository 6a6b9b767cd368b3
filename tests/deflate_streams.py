"""A DEFLATE writer and inspector for tests, written from RFC 1951 (and RFC 1952 / SAM spec 4.1 for the BGZF member around a stream).

Every compressed byte the suite used to feed csrc/nmbedinflate.h came out of zlib, which uses little of the freedom the format gives an
encoder.  The writer here takes a text as an EXPLICIT tokenisation — literal bytes and (length, distance) pairs — and emits it as one
deflate block of a chosen type (stored, fixed, dynamic with given or computed code lengths), with every header field under the caller's
control: BFINAL, HLIT / HDIST / HCLEN padding, run-length symbols 16 / 17 / 18 computed per table or across the border of the two tables,
or spelled out one by one.  ``inspect`` is a small independent inflate (puff-style: canonical codes from lengths, one symbol at a time)
that reports what a stream contains — block types, code lengths, symbols in use, tokens — so that a test can assert that the edge a stream
was built for is in its bytes, whatever code put it there.

Plain Python, no GPU, not a conftest.
"""
from __future__ import annotations

import struct
import zlib

LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32                         # (30 and 31 have codewords and no meaning)


def length_symbol(length):
    """(symbol - 257, extra value) of a match length; 258 is symbol 285, never 284 + 31."""
    assert 3 <= length <= 258
    if length == 258:
        return 28, 0
    s = max(k for k in range(28) if LENGTH_BASE[k] <= length)
    return s, length - LENGTH_BASE[s]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    s = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return s, dist - DIST_BASE[s]


def length_range(s):
    """smallest and largest length of symbol 257 + s"""
    return LENGTH_BASE[s], (258 if s == 28 else 257 if s == 27 else LENGTH_BASE[s] + (1 << LENGTH_EXTRA[s]) - 1)


def dist_range(s):
    return DIST_BASE[s], DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1


class BitWriter:
    """Bits are packed from the least significant bit of each byte; Huffman codes go in most significant bit first (RFC 1951, 3.1.1)."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        assert 0 <= value < (1 << n) if n else value == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def kraft(lengths):
    """sum of 2^-len over the codes, in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - n) for n in lengths if n)


def canonical_codes(lengths):
    """symbol -> (code, length) for the nonzero lengths (RFC 1951, 3.2.2)"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def _reversed_codes(lengths):
    """symbol -> (codeword with its first bit in bit 0, length): what BitWriter.bits takes"""
    return {s: (int(format(c, f"0{n}b")[::-1], 2), n) for s, (c, n) in canonical_codes(lengths).items()}


def huffman_lengths(freq, limit):
    """Code lengths of at most `limit` bits from symbol frequencies (0 = unused).  One used symbol gets one bit (an incomplete code, which
    the format allows for exactly that case); frequencies are flattened until the longest code fits — not optimal, always valid."""
    import heapq
    used = [s for s, f in enumerate(freq) if f]
    lengths = [0] * len(freq)
    if len(used) == 1:
        lengths[used[0]] = 1
        return lengths
    f = {s: freq[s] for s in used}
    while used:
        heap = [(f[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            a = heapq.heappop(heap)
            b = heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            for s in used:
                lengths[s] = depth[s]
            break
        f = {s: (v + 1) // 2 for s, v in f.items()}
    return lengths


def ladder_lengths(n_symbols, rare, maxbits):
    """A COMPLETE code over n_symbols with two codewords of `maxbits` bits: the ladder 2, 3, ..., maxbits - 1, maxbits, maxbits on the
    `maxbits` symbols of `rare` (half the code space; the last two get the longest codes), a balanced code on all the others (the other
    half)."""
    rare = list(rare)
    assert len(rare) == maxbits and len(set(rare)) == maxbits
    lengths = [0] * n_symbols
    for k, s in enumerate(rare):
        lengths[s] = min(2 + k, maxbits)
    rest = [s for s in range(n_symbols) if s not in set(rare)]
    m = len(rest)
    assert m >= 1
    k = m.bit_length() - 1
    r = m - (1 << k)
    for j, s in enumerate(rest):
        lengths[s] = 1 + (k + 1 if j >= m - 2 * r else k)
    assert kraft(lengths) == 32768 and max(lengths) == maxbits
    return lengths


def expand(tokens, history=b""):
    """the text of a token list; every pair is checked against what stands in front of it in the member"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(out), (t, len(out))
            for _ in range(length):
                out.append(out[-dist])
        else:
            assert 0 <= t < 256
            out.append(t)
    return bytes(out[len(history):])


def rle_code_lengths(seq, allow=(16, 17, 18)):
    """code lengths -> code-length symbols (symbol, extra value), greedily, with the repeat symbols of `allow` only"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        j = i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11 and 18 in allow:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            while run >= 3 and 17 in allow:
                k = min(run, 10)
                out.append((17, k - 3))
                run -= k
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3 and 16 in allow:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


def expand_code_lengths(symbols):
    out = []
    for s, x in symbols:
        if s < 16:
            out.append(s)
        elif s == 16:
            assert out, "symbol 16 with nothing in front of it"
            out += [out[-1]] * (3 + x)
        elif s == 17:
            out += [0] * (3 + x)
        else:
            out += [0] * (11 + x)
    return out


def write_block(w, tokens, kind, final, history=b"", *, litlen=None, dist=None, nlen=None, ndist=None, hclen=None, cross=False,
                allow=(16, 17, 18), cl_symbols=None, cl_lengths=None, check=True):
    """One deflate block into BitWriter `w`.

    kind: "stored" (the tokens' text goes out as bytes), "fixed", "dynamic".  For a dynamic block `litlen` / `dist` are explicit code
    lengths (Kraft-checked here; None: computed from the token frequencies), `nlen` / `ndist` / `hclen` pad HLIT / HDIST / HCLEN up to
    the given COUNTS (257..286, 1..30, 4..19), `cross` runs the code-length repeats over the concatenation of the two tables instead
    of over each table on its own (what zlib does), `allow` names the repeat symbols that may be used, `cl_symbols` spells the
    code-length symbols out ((symbol, extra) pairs, checked to expand to the tables), `cl_lengths` gives the code-length code itself.
    check=False skips the validity checks (streams that are meant to be refused).
    """
    text = expand(tokens, history) if check else None
    w.bits(1 if final else 0, 1)
    if kind == "stored":
        w.bits(0, 2)
        w.align()
        assert len(text) <= 65535
        w.out += struct.pack("<HH", len(text), len(text) ^ 0xFFFF) + text
        return text
    if kind == "fixed":
        w.bits(1, 2)
        ll, dl = FIXED_LITLEN, FIXED_DIST
    else:
        assert kind == "dynamic"
        w.bits(2, 2)
        fl, fd = [0] * 286, [0] * 30
        fl[256] = 1
        for t in tokens:
            if isinstance(t, tuple):
                fl[257 + length_symbol(t[0])[0]] += 1
                fd[dist_symbol(t[1])[0]] += 1
            elif not isinstance(t, str):
                fl[t] += 1
        ll = list(litlen) if litlen is not None else huffman_lengths(fl, 15)
        dl = list(dist) if dist is not None else huffman_lengths(fd, 15)
        ll += [0] * (286 - len(ll))
        dl += [0] * (30 - len(dl))
        if check:
            for lens, fr, what in ((ll, fl, "literal/length"), (dl, fd, "distance")):
                k, used = kraft(lens), sum(1 for n in lens if n)
                assert k <= 32768, f"{what} code over-subscribed"
                assert k == 32768 or used <= 1 and max(lens) <= 1, f"{what} code incomplete with more than one symbol"
                assert all(lens[s] for s, f in enumerate(fr) if f), f"{what} symbol in use without a code"
        n_l = max(257, max((s + 1 for s in range(286) if ll[s]), default=257))
        n_d = max(1, max((s + 1 for s in range(30) if dl[s]), default=1))
        if nlen is not None:
            assert not check or n_l <= nlen <= 286
            n_l = nlen
        if ndist is not None:
            assert not check or n_d <= ndist <= 30
            n_d = ndist
        tables = (ll + [0] * 40)[:n_l], (dl + [0] * 40)[:n_d]
        if cl_symbols is None:
            cl_symbols = rle_code_lengths(tables[0] + tables[1], allow) if cross else rle_code_lengths(tables[0], allow) + rle_code_lengths(tables[1], allow)
        if check:
            assert expand_code_lengths(cl_symbols) == tables[0] + tables[1], "the code-length symbols do not spell the tables"
        fc = [0] * 19
        for s, _ in cl_symbols:
            fc[s] += 1
        cl = list(cl_lengths) if cl_lengths is not None else huffman_lengths(fc, 7)
        if check:
            assert kraft(cl) == 32768, "the code-length code must be complete"
            assert max(cl) <= 7 and all(cl[s] for s in range(19) if fc[s])
        n_c = max(4, max((k + 1 for k in range(19) if cl[CL_ORDER[k]]), default=4))
        if hclen is not None:
            assert not check or n_c <= hclen <= 19
            n_c = hclen
        w.bits(n_l - 257, 5)
        w.bits(n_d - 1, 5)
        w.bits(n_c - 4, 4)
        for k in range(n_c):
            w.bits(cl[CL_ORDER[k]], 3)
        cc = _reversed_codes(cl)
        for s, x in cl_symbols:
            w.bits(*cc[s])
            if s >= 16:
                w.bits(x, (2, 3, 7)[s - 16])
    lc, dc = _reversed_codes(ll), _reversed_codes(dl)
    for t in tokens:
        if isinstance(t, tuple):
            s, x = length_symbol(t[0])
            w.bits(*lc[257 + s])
            w.bits(x, LENGTH_EXTRA[s])
            s, x = dist_symbol(t[1])
            w.bits(*dc[s])
            w.bits(x, DIST_EXTRA[s])
        elif isinstance(t, str):                 # a raw symbol, "L286" / "D30", or raw bits, "B1": for streams that are meant to be refused
            if t[0] == "B":
                w.bits(int(t[:0:-1], 2), len(t) - 1)
            else:
                w.bits(*(lc if t[0] == "L" else dc)[int(t[1:])])
        else:
            w.bits(*lc[t])
    if 256 in lc:
        w.bits(*lc[256])
    return text


def deflate_stream(blocks):
    """blocks: (tokens, kind, options) in order; the last one is final unless its options say otherwise.  Returns the raw stream."""
    w, history = BitWriter(), b""
    for k, (tokens, kind, opts) in enumerate(blocks):
        opts = dict(opts)
        final = opts.pop("final", k + 1 == len(blocks))
        history += write_block(w, tokens, kind, final, history, **opts)
    return w.getvalue()


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_member(stream, text, crc=None, isize=None):
    """header with the BC subfield, the stream, CRC-32 and ISIZE (as tests/helpers.py builds them)"""
    assert len(stream) + 25 <= 0xFFFF, "a BGZF member is at most 64 KiB in the file"
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(stream) + 25) + stream
            + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize))


# ---------------------------------------------------------------------------------------------------------------------------------
# the inspector
# ---------------------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.d, self.at, self.acc, self.n = data, 0, 0, 0

    def need(self, n):
        while self.n < n:
            if self.at >= len(self.d):
                raise ValueError("the stream ends inside a block")
            self.acc |= self.d[self.at] << self.n
            self.at += 1
            self.n += 8

    def get(self, n):
        self.need(n)
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.n -= n
        return v

    def decode(self, codes):
        """codes: {(code, length): symbol}; one bit at a time, as puff does"""
        code = 0
        for n in range(1, 16):
            code = (code << 1) | self.get(1)
            s = codes.get((code, n))
            if s is not None:
                return s, n
        raise ValueError("a codeword that no symbol has")


def _decoder(lengths):
    return {v: s for s, v in canonical_codes(lengths).items()}


def inspect_stream(stream):
    """What one raw deflate stream holds: a dict with
       blocks      one dict per block: type, final, n_tokens, n_literals, text (bytes of the block), pad (bits skipped in front of a stored
                   block's LEN: the alignment it was entered at), and for dynamic blocks nlen, ndist, hclen, cl_lengths, litlen, dist (the
                   code lengths), cl_symbols ((symbol, extra, index it starts at)), crossed (the repeat symbols that ran across the
                   literal/distance border), used_litlen / used_dist (symbols decoded), max_used_litlen / max_used_dist (longest codeword
                   decoded), max_used_cl
       tokens      the member's token list (literal bytes and (length, distance) pairs; a stored block's bytes are literals)
       token_at    output position of every token
       text        the whole text
       consumed    bytes of the stream that were read
    """
    b, out, tokens, token_at, blocks = _Bits(stream), bytearray(), [], [], []
    while True:
        final, kind = b.get(1), b.get(2)
        info = dict(final=bool(final), start=len(out), first_token=len(tokens))
        if kind == 0:
            info["type"] = "stored"
            info["pad"] = b.n % 8
            b.get(b.n % 8)
            n, nn = b.get(16), b.get(16)
            if n ^ 0xFFFF != nn:
                raise ValueError("LEN / NLEN mismatch")
            for _ in range(n):
                token_at.append(len(out))
                tokens.append(b.get(8))
                out.append(tokens[-1])
        elif kind == 3:
            raise ValueError("block type 3")
        else:
            if kind == 1:
                info["type"] = "fixed"
                ll, dl = FIXED_LITLEN, FIXED_DIST
            else:
                info["type"] = "dynamic"
                n_l, n_d, n_c = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                if n_l > 286 or n_d > 30:
                    raise ValueError("too many length or distance symbols")
                cl = [0] * 19
                for k in range(n_c):
                    cl[CL_ORDER[k]] = b.get(3)
                if kraft(cl) != 32768:
                    raise ValueError("the code-length code is not complete")
                cd, lens, syms, max_cl = _decoder(cl), [], [], 0
                while len(lens) < n_l + n_d:
                    s, n = b.decode(cd)
                    max_cl = max(max_cl, n)
                    x = b.get((2, 3, 7)[s - 16]) if s >= 16 else 0
                    syms.append((s, x, len(lens)))
                    if s == 16 and not lens:
                        raise ValueError("symbol 16 first")
                    lens += [lens[-1]] * (3 + x) if s == 16 else expand_code_lengths([(s, x)])
                if len(lens) > n_l + n_d:
                    raise ValueError("a repeat past the end of the tables")
                ll, dl = lens[:n_l], lens[n_l:]
                if ll[256] == 0:
                    raise ValueError("no code for 256")
                for lens_, what in ((ll, "literal/length"), (dl, "distance")):
                    k = kraft(lens_)
                    if k > 32768 or (k < 32768 and sum(1 for n in lens_ if n) > 1):
                        raise ValueError(f"{what} code over-subscribed or incomplete")
                info.update(nlen=n_l, ndist=n_d, hclen=n_c, cl_lengths=cl, litlen=ll, dist=dl, cl_symbols=syms, max_used_cl=max_cl,
                            crossed=sorted({s for s, x, at in syms if s >= 16 and at < n_l < at + (3 + x if s < 18 else 11 + x)}))
            ld, dd = _decoder(ll), _decoder(dl)
            used_l, used_d, max_l, max_d = set(), set(), 0, 0
            while True:
                s, n = b.decode(ld)
                used_l.add(s)
                max_l = max(max_l, n)
                if s == 256:
                    break
                token_at.append(len(out))
                if s < 256:
                    tokens.append(s)
                    out.append(s)
                    continue
                if s > 285:
                    raise ValueError("length symbol 286 / 287")
                length = LENGTH_BASE[s - 257] + b.get(LENGTH_EXTRA[s - 257])
                ds, n = b.decode(dd)
                used_d.add(ds)
                max_d = max(max_d, n)
                if ds > 29:
                    raise ValueError("distance symbol 30 / 31")
                dist = DIST_BASE[ds] + b.get(DIST_EXTRA[ds])
                if dist > len(out):
                    raise ValueError("a distance beyond the start of the member")
                tokens.append((length, dist))
                for _ in range(length):
                    out.append(out[-dist])
            info.update(used_litlen=used_l, used_dist=used_d, max_used_litlen=max_l, max_used_dist=max_d)
        info["text"] = bytes(out[info["start"]:])
        info["n_tokens"] = len(tokens) - info["first_token"]
        info["n_literals"] = sum(1 for t in tokens[info["first_token"]:] if not isinstance(t, tuple))
        blocks.append(info)
        if final:
            break
    return dict(blocks=blocks, tokens=tokens, token_at=token_at, text=bytes(out), consumed=b.at)


def members_of(data):
    """(stream, crc, isize) of every BGZF member of a file's bytes"""
    off, out = 0, []
    while off < len(data):
        assert data[off:off + 4] == b"\x1f\x8b\x08\x04" and data[off + 12:off + 16] == b"BC\x02\0"
        size = int.from_bytes(data[off + 16:off + 18], "little") + 1
        crc, isize = struct.unpack("<II", data[off + size - 8:off + size])
        out.append((data[off + 18:off + size - 8], crc, isize))
        off += size
    return out


def inspect(data):
    """inspect_stream of every member of a BGZF file's bytes (the empty EOF member included), with the trailer checked"""
    out = []
    for stream, crc, isize in members_of(data):
        m = inspect_stream(stream)
        assert m["consumed"] == len(stream) and len(m["text"]) == isize and zlib.crc32(m["text"]) == crc
        out.append(m)
    return out


def literal_runs(tokens):
    """(literals in front of it, token index) of every match, and the literals behind the last match as (run, None)"""
    out, run = [], 0
    for k, t in enumerate(tokens):
        if isinstance(t, tuple):
            out.append((run, k))
            run = 0
        else:
            run += 1
    out.append((run, None))
    return out


def balanced_lengths(n):
    """a complete code over n symbols whose lengths differ by at most one (the last symbols get the longer codes)"""
    k = n.bit_length() - 1
    r = n - (1 << k)
    return [k] * (n - 2 * r) + [k + 1] * (2 * r)


# ---------------------------------------------------------------------------------------------------------------------------------
# The zoo: one bgzip pileup whose members are hand-built streams, one member per edge of csrc/nmbedinflate.h.
#
# The text is valid bedMethyl, so that the host reader (nm_bed_open, which inflates with zlib) is the oracle of every row.  What the edges
# need — runs, periods, far repeats, incompressible stretches — stands in the COLOUR column (column 9), which no parser reads: a wrong
# byte there changes no row and is caught by the member's CRC-32 (bed_crc_kernel), so the zoo is only worth anything with the CRC check
# on, which is the default.  Every member begins and ends INSIDE a colour column (lines straddle members), so the members can be put
# in any order and still concatenate to valid lines: the second file holds the same members regrouped by kind.
# ---------------------------------------------------------------------------------------------------------------------------------
ALPHA = bytes(range(33, 127))
INF2_CAP = 1536                                  # text bytes of a chunk of phase 2 (csrc/nmbedinflate.h)
ZOO_SIZES = (1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 61440, 61441, 65280, 65535, 65536)
V1_DISTS, V1_LENS = (8, 11, 15, 16, 23, 31, 32, 100), (3, 16, 17, 32, 33, 258)
RUNS = (254, 255, 256, 509, 510, 511)


def token_region_bytes(out_len, fraction=0.625):
    """inf2_region_bytes of csrc/nmbedinflate.h: the bytes phase 1 may fill with a member's tokens"""
    worst = (out_len * 4 // 3 + 32 + 15) & ~15
    want = (int(out_len * fraction) + 64 + 15) & ~15
    return min(want, worst)


def overflows_token_region(tokens, out_len, fraction=0.625):
    """The room check of bed_tokens_kernel replayed on a member's tokens (a stored block's bytes are literals): True = phase 1 gives the
    member up (INF2_FULL) and bed_inflate_kernel, one lane per member, inflates it instead of bed_resolve_kernel."""
    room, records, literals, run = token_region_bytes(out_len, fraction), 0, 0, 0
    for t in tokens:
        if 4 * records + (literals | 7) + 56 > room:
            return True
        if isinstance(t, tuple):
            records, run = records + 1, 0
        else:
            literals, run = literals + 1, run + 1
            if run == 255:
                records, run = records + 1, 0
    return False


# members that phase 1 gives up at the default fraction BY CONSTRUCTION: stored members (their text is all literals: 1 byte each against
# 5/8), the literals_* members, and texts of a few bytes (56 bytes of slack exceed the region of a tiny member at ANY fraction: these,
# and the 23 / 27 bytes that open and close the file, can never take the two phases).  Every other member gets a CUSHION of long
# matches in front of its edge until its tokens fit the region, so that its edge is decoded by bed_tokens_kernel / bed_resolve_kernel
NEVER_TWO_PHASE = ("opening", "closing", "size_1", "size_3", "size_4", "size_5")


def gives_up_by_construction(m):
    return m.group == "stored" or m.name.startswith("literals_") or m.name in NEVER_TWO_PHASE


class Member:
    def __init__(self, name, group, edge, check):
        self.name, self.group, self.edge, self.check = name, group, edge, check
        self.blocks, self.planted, self.text, self.stream = [], [], b"", b""

    @property
    def row(self):
        """the zoo's table: (name, text size, blocks, planted tokens, which edge it is there for)"""
        return self.name, len(self.text), [kind for _, kind, _ in self.blocks], self.planted, self.edge


class ZooBuilder:
    def __init__(self, seed=20, members_per_contig=12):
        import random
        self.rng, self.pos, self.n_built, self.per_contig = random.Random(seed), 0, 0, members_per_contig
        self.suffix, self.members = None, []

    def _row(self):
        r = self.rng
        self.pos += r.randint(1, 9)
        pos, cov = self.pos, r.randint(1, 60)
        nmod = r.randint(0, cov)
        pct = nmod * 10000 // cov
        prefix = f"zoo_{self.n_built // self.per_contig:02d}\t{pos}\t{pos + 1}\t{r.choice(('a', 'm', '21839'))}\t{cov}\t{r.choice('+-')}\t{pos}\t{pos + 1}\t"
        return prefix.encode(), f"\t{cov}\t{pct // 100}.{pct % 100:02d}\t{nmod}\t{cov - nmod}\t0\t0\t0\t0\t0\n".encode()

    # ---- one member
    def begin(self, name, group, edge, check):
        self.m = Member(name, group, edge, check)
        self.out, self.col, self.toks, self.run_start = bytearray(), bytearray(), [], 0

    def lit(self, data, colour=1):
        self.toks += data
        self.out += data
        self.col += bytes([colour]) * len(data)

    def colour(self, n, alpha=ALPHA):
        self.lit(bytes(self.rng.choice(alpha) for _ in range(n)))

    def newrow(self):
        prefix, suffix = self._row()
        self.lit(self.suffix + prefix, 0)
        self.suffix, self.run_start = suffix, len(self.out)

    def is_safe(self, length, dist):
        """the source holds colour bytes only: the copy changes no row"""
        o = len(self.out)
        return dist <= o and all(self.col[o - dist:o - dist + min(length, dist)])

    def match(self, length, dist, plant=True, safe=True):
        assert 3 <= length <= 258 and 1 <= dist <= min(len(self.out), 32768), (length, dist, len(self.out))
        assert not safe or self.is_safe(length, dist), (self.m.name, length, dist)
        for _ in range(length):
            self.out.append(self.out[-dist])
            self.col.append(self.col[-dist])
        self.toks.append((length, dist))
        if plant:
            self.m.planted.append((length, dist))

    def match_far(self, length, dist):
        """literals until the bytes `dist` back are colour, then the match"""
        while not self.is_safe(length, dist):
            self.colour(1)
        self.match(length, dist)

    def grow(self, n):
        """n more bytes of the colour column the member is in: a few literals, then matches from inside this column"""
        end = len(self.out) + n
        while len(self.out) < end:
            left = end - len(self.out)
            self.colour(min(left, self.rng.randint(4, 24)))
            left = end - len(self.out)
            while left >= 3 and self.rng.random() < 0.8:
                length = min(258, left)
                length -= 3 if left - length in (1, 2) and length >= 6 else 0
                self.match(length, self.rng.randint(1, len(self.out) - self.run_start), plant=False)
                left = end - len(self.out)

    def bulk(self, n, literal=False):
        """n more bytes of ordinary rows: a line end at least every 1 500 bytes"""
        end = len(self.out) + n
        while len(self.out) < end:
            if end - len(self.out) >= 160:
                self.newrow()
            left = end - len(self.out)
            k = min(left, self.rng.randint(200, 1400))
            if literal:
                self.colour(k)
            else:
                self.grow(k)

    def cushion(self):
        """cushion_bytes of long matches out of the colour column the member is in (build_zoo sets the amount)"""
        left = self.cushion_bytes
        if left <= 0:
            return
        self.colour(6)
        left = max(left - 6, 6)
        while left >= 3:
            length = min(258, left)
            length -= 3 if left - length in (1, 2) and length >= 6 else 0
            self.match(length, self.rng.randint(1, len(self.out) - self.run_start), plant=False)
            left -= length

    def pad_to(self, size, literal=False):
        assert len(self.out) <= size, (self.m.name, len(self.out), size)
        self.bulk(size - len(self.out), literal)

    def block(self, kind, **opts):
        self.m.blocks.append((self.toks, kind, opts))
        self.toks = []

    def end(self):
        assert not self.toks, "tokens without a block"
        m = self.m
        m.text, m.stream = bytes(self.out), deflate_stream(m.blocks)
        self.members.append(m)
        self.n_built += 1
        return m


def _matches(m):
    return [t for t in m["tokens"] if isinstance(t, tuple)]


def _kinds(m):
    return [b["type"] for b in m["blocks"]]


def _dyn(m, k=0):
    return [b for b in m["blocks"] if b["type"] == "dynamic"][k]


def _consecutive(tokens, want, n):
    best = run = 0
    for t in tokens:
        run = run + 1 if (isinstance(t, tuple) and want(t)) else 0
        best = max(best, run)
    return best >= n


def _recipes():
    """(name, group, edge, build(z), check(inspected member)) of every member.  group: which deflate block types the member holds —
    "stored", "fixed", "dynamic" or "multi" — the kinds that are interleaved within every wave of 64 members."""
    R = []

    def add(name, group, edge, build, check, cushion="start"):
        """cushion: where the matches go that make the member's tokens fit their region, if they do not — "start": in front of everything,
        in the first block; "block": a fixed block of their own in front; "own": the recipe calls z.cushion() itself"""
        R.append((name, group, edge, build, check, cushion))

    ENC = (("fixed", "fixed"), ("dynamic", "dynamic"))

    # ---- length and distance arithmetic
    ends_l = sorted({v for s in range(29) for v in length_range(s)})
    ends_d = sorted({v for s in range(30) for v in dist_range(s)})
    for group, kind in ENC:
        def build(z, kind=kind):
            z.newrow()
            z.colour(300)
            for length in ends_l:
                z.colour(1)
                z.match(length, z.rng.randint(1, 290))
            z.block(kind)
        add(f"lengths_{kind}", group, "every length symbol 257..285 at its smallest and largest extra-bits value", build,
            lambda m: {t[0] for t in _matches(m)} >= set(ends_l))

    def build(z):
        z.newrow()
        z.colour(64)
        for d in [v for v in ends_d if v <= 3072]:
            if len(z.out) - z.run_start < d:
                z.grow(d - (len(z.out) - z.run_start))
            z.match(z.rng.choice((3, 4, 9, 40)), d)
        z.grow(4097 - len(z.out))
        z.block("dynamic")
    add("size_4097_distances", "dynamic", "4097 bytes of text (first_pass of bed_crc_kernel moves); distance symbols 0..22 at both ends, one line", build,
        lambda m: len(m["text"]) == 4097 and {t[1] for t in _matches(m)} >= {v for v in ends_d if v <= 3072})

    def build(z):
        z.colour(40)
        z.match(10, 40)
        z.grow(250)
        z.pad_to(32768)
        z.match(258, 32768)
        for d in ends_d:
            z.match_far(z.rng.choice((3, 5, 11, 258)), d)
        z.pad_to(65280)
        z.block("dynamic")
    add("size_65280_distances", "dynamic", "every distance symbol 0..29 at both ends (1..32768); distance == output position in the first chunk "
        "of phase 2 and at 32768; 65280 bytes of text", build,
        lambda m: len(m["text"]) == 65280 and {t[1] for t in _matches(m)} >= set(ends_d)
        and {m["token_at"][k] for k, t in enumerate(m["tokens"]) if isinstance(t, tuple) and t[1] == m["token_at"][k]} >= {40, 32768})

    # ---- code shapes
    def build(z):
        z.newrow()
        z.colour(100)
        for _ in range(6):
            z.lit(b"{}}{")
            z.match(z.rng.randint(3, 40), z.rng.randint(1, 90))
        z.block("dynamic", litlen=ladder_lengths(286, list(range(1, 14)) + [ord("{"), ord("}")], 15))
    add("litlen_15_bits", "dynamic", "15-bit literal/length codes, both codewords decoded", build,
        lambda m: _dyn(m)["max_used_litlen"] == 15 and {ord("{"), ord("}")} <= _dyn(m)["used_litlen"] and max(_dyn(m)["litlen"]) == 15)

    def build(z):
        z.newrow()
        z.colour(200)
        for d in (100, 150, 97, 192, 3, 40):
            z.colour(2)
            z.match(z.rng.randint(3, 60), d)
        z.block("dynamic", dist=ladder_lengths(30, list(range(16, 29)) + [13, 14], 15), ndist=30)
    add("dist_15_bits", "dynamic", "15-bit distance codes, both codewords decoded; ndist 30", build,
        lambda m: _dyn(m)["max_used_dist"] == 15 and {13, 14} <= _dyn(m)["used_dist"] and _dyn(m)["ndist"] == 30)

    def build(z):
        z.newrow()
        z.colour(150)
        for _ in range(5):
            z.colour(3)
            z.match(z.rng.randint(3, 30), z.rng.randint(1, 100))
        z.block("dynamic", cl_lengths=ladder_lengths(19, [1, 2, 3, 13, 14, 17, 18], 7))
    add("codelen_7_bits_hclen_19", "dynamic", "7-bit code-length codes, both codewords (17 and 18) decoded; HCLEN 19", build,
        lambda m: _dyn(m)["max_used_cl"] == 7 and _dyn(m)["hclen"] == 19 and {17, 18} <= {s for s, _, _ in _dyn(m)["cl_symbols"]})

    for where in ("first", "middle", "last"):
        def build(z, where=where):
            if where == "first":
                z.block("dynamic")
            z.newrow()
            z.grow(120)
            z.block("fixed")
            if where == "middle":
                z.block("dynamic")
            z.colour(30)
            z.match(20, 7)
            z.block("dynamic")
            if where == "last":
                z.block("dynamic")
        add(f"only_256_{where}", "multi", f"a dynamic block whose only symbol is 256, {where} in its member (one 1-bit literal/length code, no distance code)",
            build, lambda m, where=where: [b for b in m["blocks"] if b["type"] == "dynamic" and b["n_tokens"] == 0 and sum(b["litlen"]) == 1
                                          and not any(b["dist"])] and m["blocks"][{"first": 0, "middle": 1, "last": -1}[where]]["n_tokens"] == 0)

    def build(z):
        z.newrow()
        z.colour(200)
        z.block("dynamic")
    add("nlen_257_no_distance_code", "multi", "nlen 257, ndist 1 with length 0: no distance code (behind a fixed block of matches)", build,
        lambda m: (_dyn(m)["nlen"], _dyn(m)["dist"]) == (257, [0]), cushion="block")

    def build(z):
        z.newrow()
        z.grow(300)
        z.block("dynamic", nlen=286, ndist=30, hclen=19)
    add("nlen_286_ndist_30", "dynamic", "HLIT / HDIST / HCLEN padded to nlen 286, ndist 30, HCLEN 19", build,
        lambda m: (_dyn(m)["nlen"], _dyn(m)["ndist"], _dyn(m)["hclen"]) == (286, 30, 19))

    def build(z):
        z.newrow()
        z.colour(20)
        for _ in range(8):
            z.colour(2)
            z.match(z.rng.randint(3, 100), 1)
        z.block("dynamic")
    add("ndist_1_single_code", "dynamic", "ndist 1: exactly one distance code (incomplete, allowed), symbol 0", build,
        lambda m: _dyn(m)["dist"] == [1] and len(_matches(m)) == 8)

    def build(z):
        z.newrow()
        z.colour(20)
        for _ in range(8):
            z.colour(2)
            z.match(z.rng.randint(3, 100), z.rng.choice((5, 6)))
        z.block("dynamic")
    add("single_distance_code_symbol_4", "dynamic", "exactly one distance code, on symbol 4 (distances 5 and 6)", build,
        lambda m: _dyn(m)["dist"] == [0, 0, 0, 0, 1] and {t[1] for t in _matches(m)} == {5, 6})

    tail3 = [9] * 230 + [10] * 52 + [3] * 4                       # complete: the four last length symbols take half the code space
    assert kraft(tail3) == 32768 and len(tail3) == 286

    def build(z):
        z.newrow()
        z.colour(60)
        for _ in range(6):
            z.colour(2)
            z.match(z.rng.choice((227, 240, 257, 258)), z.rng.randint(1, 8))
        z.block("dynamic", litlen=tail3, dist=[3] * 8, cross=True)
    add("repeat_16_across_border", "dynamic", "symbol 16 running across the literal/distance border", build, lambda m: 16 in _dyn(m)["crossed"])

    def build(z):
        z.newrow()
        z.colour(60)
        for _ in range(6):
            z.colour(2)
            z.match(z.rng.choice((227, 240, 257, 258)), z.rng.randint(1, 8))
        z.block("dynamic", litlen=tail3, dist=[3] * 8, cl_symbols=rle_code_lengths(tail3) + [(16, 3), (3, 0), (3, 0)])
    add("repeat_16_first_of_distances", "dynamic", "symbol 16 as the first symbol of the distance lengths (it repeats the last literal/length length)", build,
        lambda m: any(s == 16 and at == _dyn(m)["nlen"] for s, _, at in _dyn(m)["cl_symbols"]))

    for sym, allow in ((17, (16, 17)), (18, (16, 17, 18))):
        def build(z, allow=allow):
            z.newrow()
            z.colour(60)
            for _ in range(6):
                z.colour(2)
                z.match(z.rng.randint(67, 82), z.rng.choice((5, 6)))            # length symbol 277, distance symbol 4
            z.block("dynamic", nlen=286, cross=True, allow=allow)
        add(f"repeat_{sym}_across_border", "dynamic", f"symbol {sym} running across the literal/distance border", build,
            lambda m, sym=sym: sym in _dyn(m)["crossed"])

    def build(z):
        z.colour(400, alpha=bytes(range(40, 118)))
        z.lit(b"u!u")
        z.block("dynamic")
    add("repeat_18_of_138", "multi", "symbol 18 with 138 zeros (no literal above 'u': lengths 118..255; behind a fixed block of matches)", build,
        lambda m: any(s == 18 and x == 127 for s, x, _ in _dyn(m)["cl_symbols"]), cushion="block")

    def build(z):
        z.newrow()
        z.colour(200)
        z.block("dynamic", litlen=[8] * 255 + [0, 8], allow=())
    add("hclen_5", "multi", "HCLEN 5, the fewest a valid block can have (HCLEN 4 gives no symbol a nonzero length: a refusal); a flat 8-bit code "
        "(behind a fixed block of matches)", build, lambda m: _dyn(m)["hclen"] == 5 and _dyn(m)["nlen"] == 257, cushion="block")

    # ---- block structure
    cycle = ("stored", "fixed", "dynamic")
    for n in (3, 4, 5, 6):
        def build(z, n=n):
            for k in range(n):
                z.bulk(z.rng.randint(170, 400), literal=cycle[(k + n) % 3] == "stored")
                if cycle[(k + n) % 3] != "stored":
                    z.match(z.rng.randint(3, 258), z.rng.randint(1, len(z.out) - z.run_start))
                z.block(cycle[(k + n) % 3])
        add(f"mixed_{n}_blocks", "multi", f"{n} blocks mixing stored, fixed and dynamic: run, literal word and turn counter carried across block borders", build,
            lambda m, n=n: len(m["blocks"]) == n and set(_kinds(m)) == set(cycle))

    for where in ("start", "middle", "end", "everywhere"):
        def build(z, where=where):
            if where in ("start", "everywhere"):
                z.block("stored")
            z.bulk(250)
            z.block("fixed")
            if where in ("middle", "everywhere"):
                z.block("stored")
            z.bulk(250)
            z.block("dynamic")
            if where in ("end", "everywhere"):
                z.block("stored")
                z.block("stored" if where == "end" else "fixed")
        add(f"empty_stored_{where}", "multi", f"a non-final empty stored block (00 00 FF FF) at the {where}", build,
            lambda m, where=where: [k for k, b in enumerate(m["blocks"]) if b["type"] == "stored" and not b["text"] and not b["final"]]
            == {"start": [0], "middle": [1], "end": [2], "everywhere": [0, 2, 4]}[where])

    def build(z):
        z.colour(8)
        for j in range(8):
            z.colour(1)
            for _ in range(j):
                z.match(z.rng.randint(3, 10), z.rng.choice((5, 6)))              # 7 + 5 + 1 bits
            z.block("fixed")
            z.colour(5)
            z.block("stored")
        z.cushion()                                                # (behind the edge: in front it would move the first alignment)
        z.block("fixed")
    add("stored_at_8_alignments", "multi", "a stored block entered at every one of the eight bit alignments", build,
        lambda m: {b["pad"] for b in m["blocks"] if b["type"] == "stored"} == set(range(8)), cushion="own")

    def build(z):
        z.colour(4)
        for k in range(10):
            z.colour(1)
            if k % 3 != 2:
                z.match(4, 2)
            z.block(("fixed", "dynamic", "stored")[k % 3])
    add("block_borders_n_lit_mod_8", "multi", "block borders at every value of n_lit % 8", build,
        lambda m: {sum(b["n_literals"] for b in m["blocks"][:k + 1]) % 8 for k in range(len(m["blocks"]))} == set(range(8)))

    def build(z):
        z.newrow()
        z.colour(10)
        z.match(6, 4)
        z.colour(200)
        z.block("fixed")
        z.colour(100)
        z.match(6, 4)
        z.colour(3)
        z.block("dynamic")
    add("run_255_in_next_block", "multi", "a literal run that reaches 255 in the block after the one it started in", build,
        lambda m: (300, m["blocks"][1]["first_token"] + 100) in literal_runs(m["tokens"]) and _kinds(m) == ["fixed", "dynamic"])

    def build(z):
        z.newrow()
        z.colour(100)
        z.block("stored")
        for d in (100, 51, 7, 1):
            z.match(z.rng.randint(10, 50), d)
        z.block("fixed")
    add("fixed_matches_from_stored", "multi", "matches in a fixed block whose source lies in a preceding stored block", build,
        lambda m: _kinds(m) == ["stored", "fixed"] and m["tokens"][m["blocks"][1]["first_token"]][1] == 100)

    # ---- token and phase-2 edges, one-lane kernel edges: each in the fixed and in a dynamic code
    def lits(z, n):
        """n literals that end inside a colour column"""
        at = len(z.out)
        if n >= 120:
            z.newrow()
        z.colour(n - (len(z.out) - at))

    for group, kind in ENC:
        def build(z, kind=kind):
            for run in RUNS:
                lits(z, run)
                z.match(5, 3)
            z.colour(2)
            z.block(kind)
        add(f"runs_{kind}", group, "literal runs of 254, 255, 256, 509, 510 and 511 in front of a match", build,
            lambda m: [r for r, k in literal_runs(m["tokens"]) if k is not None][-len(RUNS):] == list(RUNS))

        def build(z, kind=kind):
            z.colour(10)
            z.match(4, 3)
            lits(z, 255)
            z.block(kind)
        add(f"ends_on_run_255_{kind}", group, "a member that ends on a literal run of exactly 255", build,
            lambda m: literal_runs(m["tokens"])[-1] == (255, None) and m["tokens"][-256] == (4, 3))

        def build(z, kind=kind):
            lits(z, 200)
            z.match(33, 20)
            z.block(kind)
        add(f"ends_on_match_{kind}", group, "a member that ends on a match (one-lane kernel: a match ending exactly at the member's end)", build,
            lambda m: m["tokens"][-1] == (33, 20))

        def build(z, kind=kind):
            lits(z, 200)
            z.match(100, 50)
            z.colour(10)
            z.block(kind)
        add(f"match_in_last_40_{kind}", group, "one-lane kernel: a match ending inside the last 40 bytes of a member (copied byte by byte)", build,
            lambda m: m["tokens"][-11] == (100, 50) and not any(isinstance(t, tuple) for t in m["tokens"][-10:]))

        for shift, what in ((0, "a chunk of exactly INF2_CAP = 1536 bytes"), (-1, "one byte short of INF2_CAP"), (4, "shifted by a 4-byte sequence")):
            def build(z, kind=kind, shift=shift):
                if shift > 0:
                    z.colour(1)
                    z.match(3, 1)
                for k in range(3):
                    lits(z, 254 - (1 if shift < 0 and k == 0 else 0))
                    z.match(258, z.rng.randint(1, 150))
                z.colour(10)
                z.match(50, 30)                                   # its source straddles the start of its chunk where the chunk was full
                z.colour(5)
                z.block(kind)
            add(f"three_full_sequences_{kind}_{shift + 1}", group, f"three sequences of 254 + 258 bytes in a row: {what}; then a match whose source "
                "straddles the start of its chunk", build,
                lambda m, shift=shift: [r for r, k in literal_runs(m["tokens"]) if k is not None][-4:-1] == [254 - (shift < 0), 254, 254]
                and [t[0] for t in _matches(m)][-4:] == [258, 258, 258, 50] and (shift != 0 or m["token_at"][-6] == INF2_CAP + 10))

        def build(z, kind=kind):
            z.newrow()
            z.colour(10)
            for _ in range(200):
                z.match(3, z.rng.randint(1, 10))
            z.colour(4)
            z.block(kind)
        add(f"200_short_matches_{kind}", group, "200 consecutive length-3 matches without literals: the 64-sequence limit of a chunk binds, not its bytes", build,
            lambda m: _consecutive(m["tokens"], lambda t: t[0] == 3, 200))

        def build(z, kind=kind):
            z.newrow()
            z.colour(5)
            for _ in range(70):
                z.match(5, 5)
            z.colour(4)
            z.block(kind)
        add(f"chain_of_70_{kind}", group, "a chain of 70 short matches, each copying the one before, 64 of them in one chunk", build,
            lambda m: _consecutive(m["tokens"], lambda t: t == (5, 5), 70))

        def build(z, kind=kind):
            z.newrow()
            z.colour(20)
            start = len(z.out) - 10                               # inside the colour column of one line ...
            z.newrow()
            z.colour(20)
            length = len(z.out) - 10 - start                      # ... to the same place of the next: one line end, one whole set of columns
            z.match(length, len(z.out) - start, safe=False)
            z.bulk(3000)
            z.match(length, len(z.out) - start, safe=False)
            z.colour(3)
            z.block(kind)
        add(f"line_repeats_{kind}", group, "repeats of a whole earlier line (its end and the next line's first columns), next to it and 3 000 bytes on: "
            "the copies are rows of their own", build,
            lambda m: len([k for k, t in enumerate(m["tokens"]) if isinstance(t, tuple)
                           and m["text"][m["token_at"][k] - t[1]:m["token_at"][k] - t[1] + t[0]].count(b"\n") == 1 and t[1] > t[0]]) >= 2)

        for d in range(1, 8):
            def build(z, kind=kind, d=d):
                z.newrow()
                z.colour(d)
                for _ in range(5):
                    z.match(258, d)
                z.colour(3)
                z.block(kind)
            add(f"period_{d}_{kind}", group, f"five length-258 matches at distance {d} back to back: {d} literal(s) feed 1290 bytes across a chunk border; "
                "one-lane kernel: the periodic store", build, lambda m, d=d: _consecutive(m["tokens"], lambda t: t == (258, d), 5))

        def build(z, kind=kind):
            z.newrow()
            z.colour(120)
            for d in V1_DISTS:
                for length in V1_LENS:
                    z.colour(1)
                    z.match(length, d)
            z.colour(45)
            z.block(kind)
        add(f"word_copies_{kind}", group, "one-lane kernel: distances 8..15, 16..31 and >= 32 with match lengths 3, 16, 17, 32, 33 and 258", build,
            lambda m: set(_matches(m)) == {(a, d) for d in V1_DISTS for a in V1_LENS})

    # ---- sizes for bed_crc_kernel and the scratch path (4097 and 65280 are above)
    plan = {1: ("stored", "stored"), 3: ("fixed", "fixed"), 4: ("dynamic", "dynamic"), 5: ("stored", "stored"), 63: ("fixed", "fixed"), 64: ("dynamic", "dynamic"),
            65: ("fixed", "fixed"), 4095: ("fixed", "fixed"), 4096: ("stored", "stored"), 61440: ("dynamic", "dynamic"), 61441: ("fixed", "fixed"),
            65535: ("multi", None), 65536: ("fixed", "fixed")}
    for size, (group, kind) in plan.items():
        def build(z, size=size, kind=kind):
            if size < 10:
                z.colour(size)
            elif size < 100:                                       # (mostly one match: 63 literals would not fit the token region)
                z.colour(3)
                z.match(size - 3, z.rng.randint(1, 3))
            elif kind is None:                                     # stored, then dynamic: 65 535 bytes do not fit one member as a stored block
                z.pad_to(30000, literal=True)
                z.block("stored")
                z.pad_to(size)
                kind = "dynamic"
            else:
                z.pad_to(size, literal=kind == "stored")
            z.block(kind)
        add(f"size_{size}", group, f"{size} bytes of text (bed_crc_kernel: n <= 64, the chunk with the first four bytes, first_pass; the format's maximum)", build,
            lambda m, size=size: len(m["text"]) == size)

    # ---- literals only: the tokens overflow the default 5/8 region -> INF2_FULL in the middle of a slab
    for name, group, size, kinds in (("literals_fixed", "fixed", 3000, ("fixed",)), ("literals_dynamic", "dynamic", 5000, ("dynamic",)),
                                     ("literals_two_blocks", "multi", 2500, ("fixed", "dynamic"))):
        def build(z, size=size, kinds=kinds):
            for k, kind in enumerate(kinds):
                z.pad_to(size * (k + 1) // len(kinds), literal=True)
                z.block(kind)
        add(name, group, "literals only: the tokens overflow the default token region (INF2_FULL), the one-lane kernel takes the member", build,
            lambda m: not _matches(m) and len(m["text"]) + 4 * (len(m["text"]) // 255) + 56 > int(len(m["text"]) * 0.625) + 64)
    return R


def _neighbour(group, k):
    def build(z):
        n = z.rng.randint(300, 20000)
        if group == "multi":
            for j, kind in enumerate(("dynamic", "stored", "fixed")):
                z.pad_to(n * (j + 1) // 3, literal=kind == "stored")
                z.block(kind)
        else:
            z.pad_to(n, literal=group == "stored")
            z.block(group)
    return (f"rows_{group}_{k}", group, "ordinary rows: a neighbour in the wave", build,
            lambda m: set(_kinds(m)) == ({"dynamic", "stored", "fixed"} if group == "multi" else {group}), "start")


class Zoo:
    """members: the Members in file order (the first opens the first line, the last closes the last one); text: the whole bedMethyl text"""

    def __init__(self, members):
        self.members = members
        self.text = b"".join(m.text for m in members)

    def write(self, gz_path):
        """the zoo as a bgzip file with its tabix index (tests/helpers.py writes both; the streams are the hand-built ones)"""
        from helpers import write_bgzf_tabix
        todo = iter(self.members)

        def deflate(text):
            m = next(todo)
            assert m.text == text
            return m.stream
        write_bgzf_tabix(self.text, gz_path, member_sizes=[len(m.text) for m in self.members], deflate=deflate)

    def regrouped(self):
        """the same members, all stored ones first, then fixed, dynamic, multi-block (first and last member stay where they are)"""
        inner = self.members[1:-1]
        return Zoo([self.members[0]] + [m for g in ("stored", "fixed", "dynamic", "multi") for m in inner if m.group == g] + [self.members[-1]])

    def write_members(self, gz_path):
        with open(gz_path, "wb") as f:
            f.write(b"".join(bgzf_member(m.stream, m.text) for m in self.members) + BGZF_EOF)


def build_zoo(n_members=141, seed=20, edges=True):
    """The zoo (built once per process).  Kinds are interleaved in proportion, so that every wave of 64 members holds stored, fixed,
    dynamic and multi-block members side by side.  edges=False: ordinary rows only (the valid members around a refused stream)."""
    if (n_members, seed) in _ZOO_CACHE:
        return _ZOO_CACHE[(n_members, seed)]
    recipes = _recipes() if edges else []
    k = 0
    while len(recipes) + 2 < n_members:                         # neighbours, most of them of the kinds the edges leave rare
        counts = {g: sum(1 for r in recipes if r[1] == g) for g in ("stored", "multi", "fixed", "dynamic")}
        recipes.append(_neighbour(min(counts, key=counts.get), k))
        k += 1
    by_group = {}
    for r in recipes:
        by_group.setdefault(r[1], []).append(r)
    order = sorted(((j + 0.5) / len(rs), g, j) for g, rs in by_group.items() for j in range(len(rs)))
    z = ZooBuilder(seed)
    z.cushion_bytes = 0
    z.begin("opening", "fixed", "opens the first line", lambda m: True)
    prefix, z.suffix = z._row()
    z.lit(prefix, 0)
    z.colour(1)
    z.block("fixed")
    z.end()
    for _, g, j in order:
        name, group, edge, build, check, mode = by_group[g][j]
        state, z.cushion_bytes = (z.rng.getstate(), z.pos, z.suffix), 0
        while True:
            z.begin(name, group, edge, check)
            if mode != "own":
                z.cushion()
                if mode == "block":
                    z.block("fixed")
            build(z)
            # the tokens against the region, with every record and literal of the member counted at once (never less than the kernel counts)
            tokens = [t for toks, kind, _ in z.m.blocks for t in (expand(toks, b"\0" * 32768) if kind == "stored" else toks)]
            literals = sum(1 for t in tokens if not isinstance(t, tuple))
            need = 4 * (len(tokens) - literals + literals // 255 + 1) + (literals | 7) + 56
            room = token_region_bytes(len(z.out))
            if need <= room or gives_up_by_construction(z.m):
                break
            assert z.cushion_bytes < 20000, name
            z.rng.setstate(state[0])
            z.pos, z.suffix = state[1:]
            z.cushion_bytes += (need - room) * 8 // 5 + 64
        z.end()
    z.begin("closing", "stored", "closes the last line", lambda m: True)
    z.colour(1)
    z.lit(z.suffix, 0)
    z.block("stored")
    z.end()
    _ZOO_CACHE[(n_members, seed)] = Zoo(z.members)
    return _ZOO_CACHE[(n_members, seed)]


_ZOO_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# Directed refusals: streams that zlib refuses too.  Per kind: the `inflate error` code of bed_inflate_kernel (one lane per block decodes
# symbol by symbol and stops at the first check that fails) and the codes bed_tokens_kernel may report — its symbol loop is straight-line
# code that ORs the codes of every check that failed in the turn (12 | 14 | 15 | 16 | 13, masked to 5 bits), so a bad length or distance
# symbol may come out as 15, 30 or 31 depending on the garbage decoded behind it.  Each was traced by reading both kernels
# (csrc/nmbedinflate.h; the codes are the `err = N` of the check named in the comment).
# ---------------------------------------------------------------------------------------------------------------------------------
def refusals():
    """(name, raw stream, ISIZE the trailer states, codes of the one-lane kernel, codes of phase 1, refused by zlib itself)"""
    out = []
    row = b"\t255,0,0"
    text = bytes(ALPHA[(7 * k) % len(ALPHA)] for k in range(40))
    flat = balanced_lengths(286)

    def raw(fn):
        w = BitWriter()
        fn(w)
        w.align()
        return w.getvalue() + bytes(8)

    def block(tokens, kind, **opts):
        w = BitWriter()
        write_block(w, tokens, kind, True, check=False, **opts)
        w.align()
        return w.getvalue() + bytes(8)

    def stored(w):
        w.bits(1, 1); w.bits(0, 2); w.align()
        w.out += struct.pack("<HH", 40, (40 ^ 0xFFFF) ^ 0x0100) + text
    out.append(("len_nlen_mismatch", raw(stored), 40, {2}, {2}, True))                                   # (len ^ 0xFFFF) != nlen
    out.append(("block_type_3", raw(lambda w: (w.bits(1, 1), w.bits(3, 2))), 40, {3}, {3}, True))        # type == 3
    out.append(("nlen_287", raw(lambda w: (w.bits(1, 1), w.bits(2, 2), w.bits(30, 5), w.bits(0, 5), w.bits(15, 4))), 40, {4}, {4}, True))   # nlen > 286

    def oversubscribed(w):
        w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
        for _ in range(19):
            w.bits(1, 3)
    out.append(("code_length_code_oversubscribed", raw(oversubscribed), 40, {5}, {5}, True))             # construct(19) != 0
    lits = list(text)
    out.append(("repeat_past_the_tables", block(lits, "dynamic", litlen=[8] * 255 + [0, 8], dist=[0], cl_symbols=[(8, 0)] * 250 + [(18, 127)]),
                40, {8}, {8}, True))                                                                       # idx + rep > nlen + ndist
    out.append(("symbol_16_first", block(lits, "dynamic", litlen=[8] * 255 + [0, 8], dist=[0], cl_symbols=[(16, 0)] + [(8, 0)] * 252 + [(0, 0), (8, 0), (0, 0)]),
                40, {7}, {7}, True))                                                                       # sym == 16 && idx == 0
    out.append(("no_code_for_256", block(lits, "dynamic", litlen=[8] * 256, dist=[0]), 40, {9}, {9}, True))   # lengths[256] == 0
    few = [0] * 286
    few[65] = few[66] = few[256] = 2
    out.append(("literal_code_incomplete", block([65, 66, 65], "dynamic", litlen=few, dist=[0]), 3, {10}, {10}, True))   # r > 0, more than one code
    # one distance code of one bit, '0'; the match spells '1': the one-lane kernel finds no symbol (15); phase 1 finds a code "longer than
    # 15 bits" (15) and goes on with symbol 0, distance 1, which fits: 15 — or 15 | 16 = 31 should that distance not fit
    out.append(("unused_codeword_of_single_distance_code", block(lits + ["L257", "B1"], "dynamic", litlen=flat, dist=[1]), 43, {15}, {15, 31}, True))
    # fixed code: length symbols 286 / 287 have codewords; the one-lane kernel stops at once (14), phase 1 ORs in what it decodes behind
    # them as a distance (| 15, | 16)
    for sym in (286, 287):
        out.append((f"fixed_length_symbol_{sym}", block(lits + [f"L{sym}", "D0"], "fixed"), 43, {14}, {14, 15, 30, 31}, True))
    for sym in (30, 31):
        out.append((f"fixed_distance_symbol_{sym}", block(lits + ["L257", f"D{sym}"], "fixed"), 43, {15}, {15, 31}, True))
    out.append(("distance_beyond_the_start", block(lits + [(3, 41)], "fixed"), 43, {16}, {16}, True))    # dist > o
    # valid streams of 40 bytes, all literals, under trailers that state 41 and 39: o != out_len at the end (17); the literal at
    # o >= out_len (13)
    out.append(("one_byte_fewer_than_isize", block(lits, "fixed"), 41, {17}, {17}, False))
    out.append(("one_byte_more_than_isize", block(lits, "fixed"), 39, {13}, {13}, False))
    return out


def refusal_files(tmp_dir):
    """One file per refusal — an opening member, a valid member, the bad one, a valid one, the closing member — and `valid.bed.gz`, the same
    without a bad member, with its text.  Returns ([(name, path, codes one-lane, codes phase 1)], valid path, valid text)."""
    import os
    z = build_zoo(6, seed=5, edges=False)
    members = [bgzf_member(m.stream, m.text) for m in z.members]
    valid = os.path.join(tmp_dir, "valid.bed.gz")
    z.write_members(valid)
    out = []
    for name, stream, isize, v1, p1, _ in refusals():
        path = os.path.join(tmp_dir, f"refuse_{name}.bed.gz")
        with open(path, "wb") as f:
            f.write(b"".join(members[:3]) + bgzf_member(stream, b"", crc=0, isize=isize) + b"".join(members[3:]) + BGZF_EOF)
        out.append((name, path, v1, p1))
    return out, valid, z.text
