"""A reader of DEFLATE streams written from RFC 1951 (and RFC 1950 for the wrapper, the PNG specification for the chunks), independent of this
repository's inflate kernel: it decodes a stream and keeps, for every dynamic block, the three transmitted codes' lengths and the number of times
each of their symbols is actually used -- the code-length symbols of the block's own header included.  tests/test_code_tables_emul.py holds those
lengths to tests/_prefix_model.py.

    blocks, data = read(raw_deflate)      blocks: [Block]; a Block of type 2 has cl_len / cl_count (19), ll_len / ll_count (286), d_len / d_count (30);
                                          one of type 1 or 2 has tokens
    blocks, data = read_png(png_bytes)    the concatenated IDAT chunks without the zlib wrapper
"""
import zlib

from _vp8l_parse import Bits   # an LSB-first bit reader (RFC 1951 3.1.1: the same packing as lossless WebP)

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Code:
    """RFC 1951 3.2.2: the canonical code of a list of lengths, as a table over the next `maxlen` bits of the stream (a code arrives most significant bit first).
    A code may be incomplete (one distance code of one bit is legal): reading a bit pattern without a symbol fails"""

    def __init__(self, lengths):
        self.maxlen = max(lengths)
        assert self.maxlen > 0, "a code without symbols"
        count = [0] * (self.maxlen + 2)
        for l in lengths: count[l] += 1
        count[0] = 0
        nxt, c = [0] * (self.maxlen + 2), 0
        for b in range(1, self.maxlen + 1):
            c = (c + count[b - 1]) << 1
            nxt[b] = c
        self.table = [None] * (1 << self.maxlen)
        for s, l in enumerate(lengths):
            if not l: continue
            assert nxt[l] < 1 << l, "over-subscribed code"
            rev = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
            for i in range(rev, 1 << self.maxlen, 1 << l): self.table[i] = (s, l)

    def read(self, br):
        s, l = self.table[br.peek(self.maxlen)]
        br.pos += l
        return s


class Block:
    """btype 0 stored, 1 fixed, 2 dynamic; final; for a dynamic block the lengths as transmitted (padded with zeros to the whole alphabet) and the counts;
    for every block that is not stored its tokens in stream order, (0, byte) or (length, distance)"""


def _fixed():
    return Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), Code([5] * 32)


def read(raw):
    br, out, blocks = Bits(raw), bytearray(), []
    while True:
        b = Block()
        b.final, b.btype = br.read(1), br.read(2)
        assert b.btype != 3, "block type 3"
        blocks.append(b)
        if b.btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, nn = br.read(16), br.read(16)
            assert n ^ nn == 0xFFFF
            out += br.data[br.pos >> 3:(br.pos >> 3) + n]
            br.pos += 8 * n
        else:
            if b.btype == 1:
                ll, dd = _fixed()
            else:
                hlit, hdist, hclen = br.read(5) + 257, br.read(5) + 1, br.read(4) + 4
                assert hlit <= 286 and hdist <= 30
                b.cl_len = [0] * 19
                for i in range(hclen): b.cl_len[CL_ORDER[i]] = br.read(3)
                cc, b.cl_count, lens = Code(b.cl_len), [0] * 19, []
                while len(lens) < hlit + hdist:
                    s = cc.read(br)
                    b.cl_count[s] += 1
                    if s < 16: lens.append(s)
                    elif s == 16:
                        assert lens, "a repeat with nothing in front of it"
                        lens += [lens[-1]] * (3 + br.read(2))
                    else: lens += [0] * (3 + br.read(3) if s == 17 else 11 + br.read(7))
                assert len(lens) == hlit + hdist, "a run past the end of the lengths"
                b.ll_len, b.d_len = lens[:hlit] + [0] * (286 - hlit), lens[hlit:] + [0] * (30 - hdist)
                assert b.ll_len[256], "no end-of-block code"
                ll, dd = Code(b.ll_len), Code(b.d_len) if any(b.d_len) else None
            b.ll_count, b.d_count, b.tokens = [0] * 286, [0] * 30, []
            while True:
                s = ll.read(br)
                b.ll_count[s] += 1
                if s < 256:
                    out.append(s)
                    b.tokens.append((0, s))
                elif s == 256: break
                else:
                    n = LEN_BASE[s - 257] + br.read(LEN_EXTRA[s - 257])
                    d = dd.read(br)
                    b.d_count[d] += 1
                    dist = DIST_BASE[d] + br.read(DIST_EXTRA[d])
                    assert dist <= len(out), "a distance in front of the stream"
                    for _ in range(n): out.append(out[-dist])
                    b.tokens.append((n, dist))
        assert br.pos <= br.nbits, "the stream ends inside a block"
        if b.final:
            return blocks, bytes(out)


def idat(png):
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, z = 8, b""
    while pos < len(png):
        n, t = int.from_bytes(png[pos:pos + 4], "big"), png[pos + 4:pos + 8]
        if t == b"IDAT": z += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return z


def read_png(png):
    z = idat(png)
    assert z[0] & 15 == 8 and ((z[0] << 8) | z[1]) % 31 == 0 and not z[1] & 0x20, "RFC 1950 header"
    blocks, data = read(z[2:-4])
    assert zlib.adler32(data) == int.from_bytes(z[-4:], "big")
    return blocks, data
