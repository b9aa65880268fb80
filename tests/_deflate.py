"""A DEFLATE (RFC 1951) / zlib (RFC 1950) writer and a PNG wrapper for the inflate tests, written from the RFCs and sharing no code
with the oracle: every bit of a stream is the test's own choice -- block types, HLIT / HDIST / HCLEN, how the code lengths are
run-length coded, which length code a match uses, the zlib header and trailer -- so streams can be made that no encoder writes.
Also the PNG reconstruction filters (forward, and the numpy model that turns filtered rows back into pixels)."""
import heapq
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


class BitWriter:
    """bits LSB first into bytes (RFC 1951 3.1.1)"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    @property
    def pos(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0 and v == 0, (v, n)
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        """a Huffman code: most significant bit first (an over-subscribed code's overflowing codes keep their low n bits)"""
        self.bits(int(format(c & ((1 << n) - 1), "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """RFC 1951 3.2.2 for any list of lengths (complete, incomplete or over-subscribed): [code or None]"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else None)
        if l:
            nxt[l] += 1
    return out


def kraft(lengths):
    """2^15 * the code space the lengths use: 32768 complete, less incomplete, more over-subscribed"""
    return sum(1 << (15 - l) for l in lengths if l)


def huffman_lengths(freq, limit):
    """lengths of a Huffman code over the symbols with freq > 0, at most `limit` bits (flattened and built again until it fits);
    a lone symbol gets length 1"""
    used = [i for i, f in enumerate(freq) if f]
    out = [0] * len(freq)
    if not used:
        return out
    if len(used) == 1:
        out[used[0]] = 1
        return out
    f = list(freq)
    while True:
        heap = [(f[i], i, (i,)) for i in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        k = len(freq)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], k, a[2] + b[2]))
            k += 1
        if max(depth.values()) <= limit:
            for s, d in depth.items():
                out[s] = d
            return out
        f = [(x + 1) // 2 if x else 0 for x in f]


def length_symbol(n, alias=False):
    """(symbol, extra value, extra bits) of a match length; alias: 258 as 284 + 31 instead of 285"""
    if n == 258 and not alias:
        return 285, 0, 0
    assert 3 <= n <= 258 and (not alias or n == 258)
    i = max(k for k in range(28) if LEN_BASE[k] <= n)
    return 257 + i, n - LEN_BASE[i], LEN_EXTRA[i]


def dist_symbol(d):
    assert 1 <= d <= 32768
    i = max(k for k in range(30) if DIST_BASE[k] <= d)
    return i, d - DIST_BASE[i], DIST_EXTRA[i]


class Match(tuple):
    """a match token: Match(length, distance[, alias])"""

    def __new__(cls, length, dist, alias=False):
        return super().__new__(cls, (length, dist, alias))


def expand(tokens, history=b""):
    """what the tokens produce behind `history` (the decoder's own semantics: a match copies byte by byte; one that reaches in front
    of the stream copies zeros, for the invalid streams that ask for it)"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, Match):
            n, d, _ = t
            for _ in range(n):
                out.append(out[-d] if d <= len(out) else 0)
        else:
            out.append(t)
    return bytes(out[len(history):])


def rle_lengths(lens):
    """the usual run-length coding of a code length sequence with 16 / 17 / 18: [(symbol, extra)]"""
    out, i = [], 0
    while i < len(lens):
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            take = min(r, 138)
            out.append((18, take - 11) if take >= 11 else (17, take - 3))
            i += take
            continue
        out.append((v, 0))
        i += 1
        r -= 1
        while r >= 3:
            take = min(r, 6)
            out.append((16, take - 3))
            i += take
            r -= take
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def run_lengths_expand(seq):
    """the code length sequence a list of (symbol, extra) stands for"""
    out = []
    for s, e in seq:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + e)
        else:
            out += [0] * ((3 if s == 17 else 11) + e)
    return out


class Deflate:
    """a raw DEFLATE stream, block by block; `data` is what it decodes to"""

    def __init__(self):
        self.w = BitWriter()
        self.data = bytearray()
        # what was written, for the coverage checks: a dict per block (type, final, first bit behind the header, HLIT / HDIST /
        # HCLEN, the code length sequence, EOB's first bit and the block's last); a tuple per token (first bit, bits, output
        # position, litlen codeword length, distance codeword length or 0, match length or 0, distance or 0, alias)
        self.blocks, self.toks = [], []

    @property
    def pos(self):
        return self.w.pos

    def header(self, final, btype):
        self.blocks.append(dict(type=btype, final=final, at=self.pos))
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, payload, final=False, nlen=None):
        self.header(final, 0)
        self.w.align()
        n = len(payload)
        self.blocks[-1].update(start=self.pos + 32, stored=n, out=len(self.data))
        self.w.bits(n, 16)
        self.w.bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
        for b in payload:
            self.w.bits(b, 8)
        self.data += payload
        self.blocks[-1]["end"] = self.pos

    def tokens(self, tokens, lit, dist, eob=True):
        """tokens with the codes of `lit` / `dist` (lists of lengths); the data they stand for is appended"""
        lc, dc = canonical(lit), canonical(dist)
        blk = self.blocks[-1]
        blk.update(start=self.pos, out=len(self.data), lit=list(lit), dist=list(dist))
        at = len(self.data)
        for t in tokens:
            p = self.pos
            if isinstance(t, Match):
                n, d, alias = t
                s, e, eb = length_symbol(n, alias)
                self.w.code(lc[s], lit[s])
                self.w.bits(e, eb)
                ls = lit[s]
                s, e, eb = dist_symbol(d)
                self.w.code(dc[s], dist[s])
                self.w.bits(e, eb)
                self.toks.append((p, self.pos - p, at, ls, dist[s], n, d, alias))
                at += n
            else:
                self.w.code(lc[t], lit[t])
                self.toks.append((p, self.pos - p, at, lit[t], 0, 0, 0, False))
                at += 1
        self.data += expand(tokens, bytes(self.data))
        eob = eob and lit[256] > 0   # (a code without EOB: the invalid streams)
        blk["eob"] = self.pos if eob else None
        if eob:
            self.w.code(lc[256], lit[256])
        blk["end"] = self.pos

    def fixed(self, tokens, final=False, eob=True):
        self.header(final, 1)
        self.tokens(tokens, FIXED_LIT, FIXED_DIST, eob)

    def dynamic_header(self, lit, dist, hlit=None, hdist=None, hclen=None, seq=None, cl=None):
        """BTYPE 2's header: HLIT / HDIST / HCLEN default to the shortest that hold the lengths; seq: the code length sequence as
        (symbol, extra) (default: rle_lengths over the litlen and distance lengths as ONE sequence, so runs cross between them);
        cl: the code length code's lengths (default: Huffman over seq, 7 bits)"""
        hlit = hlit or max([257] + [i + 1 for i, l in enumerate(lit) if l])
        hdist = hdist or max([1] + [i + 1 for i, l in enumerate(dist) if l])
        if seq is None:
            seq = rle_lengths(list(lit[:hlit]) + [0] * (hlit - len(lit)) + list(dist[:hdist]) + [0] * (hdist - len(dist)))
        if cl is None:
            freq = [0] * 19
            for s, _ in seq:
                freq[s] += 1
            cl = huffman_lengths(freq, 7)
        if hclen is None:
            hclen = max(4, max(k + 1 for k in range(19) if cl[CL_ORDER[k]]))
        self.w.bits(hlit - 257, 5)
        self.w.bits(hdist - 1, 5)
        self.w.bits(hclen - 4, 4)
        for k in range(hclen):
            self.w.bits(cl[CL_ORDER[k]], 3)
        self.blocks[-1].update(hlit=hlit, hdist=hdist, hclen=hclen, seq=list(seq), cl=list(cl))
        cc = canonical(cl)
        for s, e in seq:
            self.w.code(cc[s], cl[s])
            if s >= 16:
                self.w.bits(e, CL_EXTRA[s])
        return seq

    def dynamic(self, tokens, final=False, lit=None, dist=None, eob=True, **hdr):
        """BTYPE 2; lit / dist default to Huffman codes (15 bits at most) of the tokens' symbols"""
        if lit is None or dist is None:
            lf, df = symbol_counts(tokens)
            lit = lit if lit is not None else huffman_lengths(lf, 15)
            dist = dist if dist is not None else huffman_lengths(df, 15)
        self.header(final, 2)
        seq = self.dynamic_header(lit, dist, **hdr)
        self.tokens(tokens, lit, dist, eob)
        return lit, dist, seq

    def getvalue(self):
        return self.w.getvalue()


def symbol_counts(tokens):
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, Match):
            lf[length_symbol(t[0], t[2])[0]] += 1
            df[dist_symbol(t[1])[0]] += 1
        else:
            lf[t] += 1
    return lf, df


def zlib_header(cinfo=7, flevel=2, fdict=False, cm=8):
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (0x20 if fdict else 0)
    flg |= (31 - ((cmf << 8) | flg) % 31) % 31
    return bytes([cmf, flg])


def zlib_wrap(raw_deflate, data, cinfo=7, flevel=2, fdict=False, adler=True, tail=b""):
    """header + stream + Adler-32 of `data` (adler=False: none) + whatever `tail` holds"""
    out = zlib_header(cinfo, flevel, fdict) + (b"\0\0\0\0" if fdict else b"") + raw_deflate
    if adler:
        out += zlib.adler32(bytes(data)).to_bytes(4, "big")
    return out + tail


# ---------------------------------------------------------------- PNG
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def rowbytes(width, ctype, depth):
    return (width * CHANNELS[ctype] * depth + 7) // 8


def chunk(t, d):
    return len(d).to_bytes(4, "big") + t + d + zlib.crc32(t + d).to_bytes(4, "big")


def png_file(zstream, width, height, ctype, depth, idat_sizes=None, plte=None, trns=None):
    """a PNG of one zlib stream; idat_sizes: the sizes of the first IDAT chunks (0 and 1 allowed), the rest in one more"""
    ihdr = width.to_bytes(4, "big") + height.to_bytes(4, "big") + bytes([depth, ctype, 0, 0, 0])
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr)
    if plte is not None:
        out += chunk(b"PLTE", plte)
    if trns is not None:
        out += chunk(b"tRNS", trns)
    at = 0
    for n in idat_sizes or []:
        out += chunk(b"IDAT", zstream[at:at + n])
        at += n
    out += chunk(b"IDAT", zstream[at:])
    return out + chunk(b"IEND", b"")


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows, bpp, types):
    """PNG forward filters: (h, rowbytes) uint8 pixels -> the filtered stream, row k with filter types[k % len(types)]"""
    h, n = rows.shape
    x = rows.astype(np.int32)
    out = bytearray()
    for y in range(h):
        ft = types[y % len(types)]
        cur = x[y]
        up = x[y - 1] if y else np.zeros(n, np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        pred = [0 * cur, a, up, (a + up) >> 1, _paeth(a, up, c)][ft]
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def unfilter(raw, width, height, ctype, depth):
    """the model: filtered stream -> (height, rowbytes) uint8 rows (PNG spec 9.2-9.4).  None / Up by whole rows, Sub as a running
    sum per byte of the pixel, Average and Paeth a pixel at a time"""
    bpp = max(1, CHANNELS[ctype] * depth // 8)
    n = rowbytes(width, ctype, depth)
    f = np.frombuffer(bytes(raw), np.uint8)[:height * (n + 1)].reshape(height, n + 1)
    out = np.zeros((height, n), np.uint8)
    prev = np.zeros(n, np.int64)
    for y in range(height):
        ft, v = int(f[y, 0]), f[y, 1:].astype(np.int64)
        assert ft <= 4, ("filter type", y, ft)
        if ft == 0:
            cur = v
        elif ft == 2:
            cur = (v + prev) & 255
        elif ft == 1:
            pad = np.zeros((-n) % bpp, np.int64)
            cur = (np.cumsum(np.concatenate([v, pad]).reshape(-1, bpp), axis=0).reshape(-1)[:n]) & 255
        else:
            cur = np.zeros(n, np.int64)
            for i in range(0, n, bpp):
                sl = slice(i, min(n, i + bpp))
                k = sl.stop - sl.start
                a = cur[i - bpp:i - bpp + k] if i >= bpp else np.zeros(k, np.int64)
                c = prev[i - bpp:i - bpp + k] if i >= bpp else np.zeros(k, np.int64)
                b = prev[sl]
                cur[sl] = (v[sl] + ((a + b) >> 1 if ft == 3 else _paeth(a, b, c))) & 255
        out[y] = cur
        prev = cur
    return out


def pillow_view(rows, width, height, ctype, depth, plte=None):
    """what np.asarray(Pillow's image) holds for these rows (the modes Pillow opens each PNG format as)"""
    if depth < 8:
        per = 8 // depth
        bits = np.unpackbits(rows, axis=1)[:, :width * depth].reshape(height, width, depth)
        v = (bits * (1 << np.arange(depth - 1, -1, -1))).sum(axis=2).astype(np.uint8)
        if ctype == 3:
            return v
        if depth == 1:
            return v.astype(bool)
        return (v.astype(np.int32) * (255 // ((1 << depth) - 1))).astype(np.uint8)
    nc = CHANNELS[ctype]
    if depth == 16:
        s = rows.reshape(height, width, nc, 2)
        if ctype == 0:
            return (s[..., 0, 0].astype(np.uint16) << 8) | s[..., 0, 1]
        if ctype == 4:   # grey + alpha at 16 bits opens as RGBA (high bytes)
            return np.stack([s[..., 0, 0]] * 3 + [s[..., 1, 0]], axis=2)
        return s[..., 0].copy()
    v = rows.reshape(height, width, nc)
    return v[..., 0] if nc == 1 else v
