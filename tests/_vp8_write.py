"""A VP8 key-frame WRITER for the tests (RFC 6386): the boolean encoder of section 7 and a frame writer that takes every field of the frame header as
an argument and the macroblocks token by token -- segment id, skip flag, prediction modes through their trees with the contextual probabilities,
coefficient tokens through the token tree with bands, contexts and zigzag.  It exists to show the decoder (caesium-clt_amd/csrc/vp8_dec.h) the
stream shapes libwebp's encoder never writes; libwebp's DECODER stays the judge of what such a stream decodes to.

The constant tables (default coefficient probabilities and their update probabilities, sub-block mode probabilities, bands, zigzag, the extra-bit
probabilities of the four large categories, the quantiser tables) are read out of include/vp8_tables.h with a regular expression.  That does not
make the decoder its own judge: the tables only steer which symbols get short codes and which content is written.  A wrong table would still give a
valid stream, libwebp and the decoder under test would both read it -- alike or not, and that is what the tests compare.

Two bounds keep the content where libwebp's scalar and SIMD inverse transforms agree (beyond them libwebp's answer depends on its build):
per 4 x 4 block the sum of |dequantised coefficient| stays <= 8191 (every intermediate of the two transform passes is then below 2^15), the Y2 block
included -- each luma DC it produces is then <= 1024 -- and the luma AC of an i16 macroblock <= 4095.  write_frame asserts both, and that no partition
starts with byte 0xFF (a state no encoder can produce, and in which boolean decoders differ)."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vp8_tables.h")


def _table(name, text=[]):
    if not text:
        text.append(open(HEADER).read())
    m = re.search(r"\b%s\[[^\]]*\]\s*=\s*\{([^}]*)\}" % name, text[0])
    assert m, name
    return [int(v) for v in re.findall(r"\d+", m.group(1))]


COEF_PROBS = _table("kVp8CoefProbs")                # [4 types][8 bands][3 contexts][11 nodes]
COEF_UPDATE_PROBS = _table("kVp8CoefUpdateProbs")
BMODE_PROBS = _table("kVp8BModeProbs")              # [10 above][10 left][9 nodes]
BANDS = _table("kVp8Bands")
ZIGZAG = _table("kVp8Zigzag")
CAT = [_table("kVp8Cat3")[:-1], _table("kVp8Cat4")[:-1], _table("kVp8Cat5")[:-1], _table("kVp8Cat6")[:-1]]
DC_Q, AC_Q = _table("kVp8DcQ"), _table("kVp8AcQ")
assert (len(COEF_PROBS), len(COEF_UPDATE_PROBS), len(BMODE_PROBS), len(BANDS), len(ZIGZAG), len(DC_Q), len(AC_Q)) == (1056, 1056, 900, 17, 16, 128, 128)
assert [len(c) for c in CAT] == [3, 4, 5, 11]

BLOCK_SUM_MAX, I16_AC_SUM_MAX = 8191, 4095
# sub-block modes in the order of the probability table: DC, TM, VE, HE, RD, VR, LD, VL, HD, HU; their bits down the tree (node, bit)
BMODE_BITS = [[(0, 0)], [(0, 1), (1, 0)], [(0, 1), (1, 1), (2, 0)], [(0, 1), (1, 1), (2, 1), (3, 0), (4, 0)], [(0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 0)],
              [(0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 1)], [(0, 1), (1, 1), (2, 1), (3, 1), (6, 0)], [(0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 0)],
              [(0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 0)], [(0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 1)]]


class BoolEnc:
    """RFC 6386 section 7.3.  The interval's lower end is kept exactly: its settled bytes in `buf`, the 8 + pending bits below them in `low`; a carry out of
    `low` walks back through `buf`"""

    def __init__(self):
        self.buf, self.low, self.range, self.pending = bytearray(), 0, 255, 0

    def put(self, bit, prob=128):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if bit:
            self.low += split
            self.range -= split
            if self.low >> (8 + self.pending):
                self.low -= 1 << (8 + self.pending)
                i = len(self.buf) - 1
                while self.buf[i] == 255:
                    self.buf[i] = 0
                    i -= 1
                self.buf[i] += 1
        else:
            self.range = split
        if self.range < 128:
            s = 8 - self.range.bit_length()
            self.range <<= s
            self.low <<= s
            self.pending += s
            while self.pending >= 8:
                self.buf.append(self.low >> self.pending)
                self.low &= (1 << self.pending) - 1
                self.pending -= 8

    def lit(self, v, n):
        assert 0 <= v < (1 << n)
        for i in range(n - 1, -1, -1):
            self.put((v >> i) & 1)

    def slit(self, v, n):
        self.lit(abs(v), n)
        self.put(1 if v < 0 else 0)

    def opt_slit(self, v, n):
        """flag + signed value; None: the flag alone"""
        self.put(0 if v is None else 1)
        if v is not None:
            self.slit(v, n)

    def finish(self):
        """the interval's lower end, rounded up to bytes, and two bytes of flush as every encoder's final flush leaves some"""
        pad = -self.pending % 8
        out = bytes(self.buf) + (self.low << pad).to_bytes((8 + self.pending + pad) // 8, "big") + b"\0\0"
        assert out[0] != 0xFF, "a partition that starts with 0xFF: no encoder writes that"
        return out


def _clip(v, hi):
    return 0 if v < 0 else hi if v > hi else v


def quantisers(base_q=0, q_delta=(0, 0, 0, 0, 0), segment=None):
    """per segment (y1 dc, y1 ac, y2 dc, y2 ac, uv dc, uv ac), RFC 6386 9.6 / 14.1 as libwebp applies it"""
    out = []
    for s in range(4):
        q = base_q
        if segment is not None:
            sq = (segment.get("quant") or [None] * 4)[s] or 0
            if not segment.get("update_data", 1):
                sq, absolute = 0, 1       # nothing sent: absolute zeros
            else:
                absolute = segment.get("abs", 1)
            q = sq if absolute else q + sq
        y2ac = max(8, (AC_Q[_clip(q + q_delta[2], 127)] * 101581) >> 16)
        out.append((DC_Q[_clip(q + q_delta[0], 127)], AC_Q[_clip(q, 127)], DC_Q[_clip(q + q_delta[1], 127)] * 2, y2ac,
                    DC_Q[_clip(q + q_delta[3], 117)], AC_Q[_clip(q + q_delta[4], 127)]))
    return out


class MB:
    """one macroblock as it is written.  levels[b][n]: quantised level of block b (0..15 luma in raster order, 16..19 U, 20..23 V, 24 the Y2 block of an i16
    macroblock) at SCAN position n; tail[b]: instead of the end-of-block token behind the last level, "no end" and zero tokens up to position 16"""

    def __init__(self, segment=0, skip=0, i4=0, ymode=0, bmodes=None, uvmode=0, levels=None, tail=None):
        self.segment, self.skip, self.i4, self.ymode, self.uvmode = segment, skip, i4, ymode, uvmode
        self.bmodes = list(bmodes) if bmodes is not None else [0] * 16
        self.levels = np.zeros((25, 16), np.int64) if levels is None else np.asarray(levels, np.int64)
        self.tail = np.zeros(25, bool) if tail is None else np.asarray(tail, bool)


def _put_block(enc, probs, btype, ctx, first, levels, tail):
    """the mirror of the token reader; returns what the reader returns (the position behind the last token read)"""
    def P(n, c):
        at = ((btype * 8 + BANDS[n]) * 3 + c) * 11
        return probs[at:at + 11]
    nzpos = [n for n in range(first, 16) if levels[n]]
    last = nzpos[-1] if nzpos else -1
    n, p = first, P(first, ctx)
    while n < 16:
        if n > last and not tail:
            enc.put(0, p[0])
            return n
        enc.put(1, p[0])
        while levels[n] == 0:
            enc.put(0, p[1])
            n += 1
            if n == 16:
                return 16
            p = P(n, 0)
        enc.put(1, p[1])
        v = abs(int(levels[n]))
        if v == 1:
            enc.put(0, p[2])
            nctx = 1
        else:
            enc.put(1, p[2])
            nctx = 2
            if v <= 4:
                enc.put(0, p[3])
                if v == 2:
                    enc.put(0, p[4])
                else:
                    enc.put(1, p[4])
                    enc.put(v - 3, p[5])
            elif v <= 10:
                enc.put(1, p[3])
                enc.put(0, p[6])
                if v <= 6:
                    enc.put(0, p[7])
                    enc.put(v - 5, 159)
                else:
                    enc.put(1, p[7])
                    enc.put((v - 7) >> 1, 165)
                    enc.put((v - 7) & 1, 145)
            else:
                enc.put(1, p[3])
                enc.put(1, p[6])
                cat = 0 if v < 19 else 1 if v < 35 else 2 if v < 67 else 3
                assert v <= 66 + 2048 - 1 + 1
                enc.put(cat >> 1, p[8])
                enc.put(cat & 1, p[9 + (cat >> 1)])
                x = v - 3 - (8 << cat)
                tab = CAT[cat]
                assert 0 <= x < (1 << len(tab))
                for i, pr in enumerate(tab):
                    enc.put((x >> (len(tab) - 1 - i)) & 1, pr)
        enc.put(1 if levels[n] < 0 else 0, 128)
        n += 1
        if n < 16:
            p = P(n, nctx)
    return 16


def write_frame(width, height, mbs, *, color_space=0, clamp=0, segment=None, simple=0, level=0, sharpness=0, lf_delta=None, log2_parts=0, base_q=0,
                q_delta=(0, 0, 0, 0, 0), refresh=0, coef_updates=None, use_skip=1, skip_p=128, version=0, riff=True):
    """segment: None or {update_map, update_data, abs, quant: 4 x (int | None), level: 4 x (int | None), probs: 3 x (int | None)};
    lf_delta: None or {update, ref: 4 x (int | None), mode: 4 x (int | None)}; coef_updates: {flat index into the probability table: new value};
    mbs: the macroblocks in raster order (MB)"""
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4
    assert len(mbs) == mbw * mbh and 0 < width < 16384 and 0 < height < 16384
    hd = BoolEnc()
    hd.put(color_space); hd.put(clamp)
    update_map = 0
    hd.put(1 if segment is not None else 0)
    if segment is not None:
        update_map = segment.get("update_map", 0)
        hd.put(update_map)
        hd.put(segment.get("update_data", 1))
        if segment.get("update_data", 1):
            hd.put(segment.get("abs", 1))
            for v in (segment.get("quant") or [None] * 4):
                hd.opt_slit(v, 7)
            for v in (segment.get("level") or [None] * 4):
                hd.opt_slit(v, 6)
        if update_map:
            for v in (segment.get("probs") or [None] * 3):
                hd.put(0 if v is None else 1)
                if v is not None:
                    hd.lit(v, 8)
    seg_probs = [255 if v is None else v for v in ((segment or {}).get("probs") or [None] * 3)]
    hd.put(simple); hd.lit(level, 6); hd.lit(sharpness, 3)
    hd.put(1 if lf_delta is not None else 0)
    if lf_delta is not None:
        hd.put(lf_delta.get("update", 1))
        if lf_delta.get("update", 1):
            for v in list(lf_delta.get("ref") or [None] * 4) + list(lf_delta.get("mode") or [None] * 4):
                hd.opt_slit(v, 6)
    hd.lit(log2_parts, 2)
    hd.lit(base_q, 7)
    for v in q_delta:
        hd.opt_slit(v if v else None, 4)
    hd.put(refresh)
    probs = list(COEF_PROBS)
    for i in range(1056):
        if coef_updates and i in coef_updates:
            hd.put(1, COEF_UPDATE_PROBS[i]); hd.lit(coef_updates[i], 8)
            probs[i] = coef_updates[i]
        else:
            hd.put(0, COEF_UPDATE_PROBS[i])
    hd.put(use_skip)
    if use_skip:
        hd.lit(skip_p, 8)
    quant = quantisers(base_q, q_delta, segment)
    nparts = 1 << log2_parts
    toks = [BoolEnc() for _ in range(nparts)]
    top_modes = [[0] * 4 for _ in range(mbw)]
    top_nz = [[0] * 9 for _ in range(mbw)]
    for my in range(mbh):
        tk = toks[my & (nparts - 1)]
        left_modes, lnz = [0] * 4, [0] * 9
        for mx in range(mbw):
            mb = mbs[my * mbw + mx]
            tm, tnz = top_modes[mx], top_nz[mx]
            if update_map:
                hd.put(mb.segment >> 1, seg_probs[0])
                hd.put(mb.segment & 1, seg_probs[1 + (mb.segment >> 1)])
            else:
                assert mb.segment == 0
            if use_skip:
                hd.put(mb.skip, skip_p)
            hd.put(0 if mb.i4 else 1, 145)
            if not mb.i4:
                bits = {0: [(0, 156), (0, 163)], 2: [(0, 156), (1, 163)], 3: [(1, 156), (0, 128)], 1: [(1, 156), (1, 128)]}[mb.ymode]   # 0 DC, 1 TM, 2 V, 3 H
                for b, p in bits:
                    hd.put(b, p)
                for k in range(4):
                    tm[k] = left_modes[k] = mb.ymode
            else:
                for y in range(4):
                    for x in range(4):
                        m = mb.bmodes[4 * y + x]
                        at = (tm[x] * 10 + left_modes[y]) * 9
                        for node, b in BMODE_BITS[m]:
                            hd.put(b, BMODE_PROBS[at + node])
                        tm[x] = left_modes[y] = m
            for b, p in {0: [(0, 142)], 2: [(1, 142), (0, 114)], 3: [(1, 142), (1, 114), (0, 183)], 1: [(1, 142), (1, 114), (1, 183)]}[mb.uvmode]:
                hd.put(b, p)
            if use_skip and mb.skip:
                for k in range(8):
                    tnz[k] = lnz[k] = 0
                if not mb.i4:
                    tnz[8] = lnz[8] = 0
                continue
            q = quant[mb.segment]
            first, ytype = 0, 3
            if not mb.i4:
                lv = mb.levels[24]
                assert int(abs(lv[0]) * q[2] + np.abs(lv[1:]).sum() * q[3]) <= BLOCK_SUM_MAX, "Y2 block beyond the transform bound"
                nz = _put_block(tk, probs, 1, tnz[8] + lnz[8], 0, lv, mb.tail[24])
                tnz[8] = lnz[8] = int(nz > 0)
                first, ytype = 1, 0
            for y in range(4):
                for x in range(4):
                    lv = mb.levels[4 * y + x]
                    if mb.i4:
                        assert int(abs(lv[0]) * q[0] + np.abs(lv[1:]).sum() * q[1]) <= BLOCK_SUM_MAX, "luma block beyond the transform bound"
                    else:
                        assert int(np.abs(lv[1:]).sum() * q[1]) <= I16_AC_SUM_MAX, "i16 luma AC beyond the transform bound"
                    nz = _put_block(tk, probs, ytype, tnz[x] + lnz[y], first, lv, mb.tail[4 * y + x])
                    tnz[x] = lnz[y] = int(nz > first)
            for ch in range(2):
                for y in range(2):
                    for x in range(2):
                        b = 16 + 4 * ch + 2 * y + x
                        lv = mb.levels[b]
                        assert int(abs(lv[0]) * q[4] + np.abs(lv[1:]).sum() * q[5]) <= BLOCK_SUM_MAX, "chroma block beyond the transform bound"
                        nz = _put_block(tk, probs, 2, tnz[4 + 2 * ch + x] + lnz[4 + 2 * ch + y], 0, lv, mb.tail[b])
                        tnz[4 + 2 * ch + x] = lnz[4 + 2 * ch + y] = int(nz > 0)
    part0 = hd.finish()
    parts = [t.finish() for t in toks]
    assert len(part0) < (1 << 19)
    tag = (version << 1) | (1 << 4) | (len(part0) << 5)
    frame = tag.to_bytes(3, "little") + b"\x9d\x01\x2a" + width.to_bytes(2, "little") + height.to_bytes(2, "little") + part0
    frame += b"".join(len(p).to_bytes(3, "little") for p in parts[:-1]) + b"".join(parts)   # every partition its honest length
    if not riff:
        return frame
    body = b"WEBP" + b"VP8 " + len(frame).to_bytes(4, "little") + frame + (b"\0" if len(frame) & 1 else b"")
    return b"RIFF" + len(body).to_bytes(4, "little") + body


# ---- content

MAGNITUDES = [(1, 1), (2, 2), (3, 4), (5, 6), (7, 10), (11, 18), (19, 34), (35, 66), (67, 2047)]   # one range per token (the four small ones, the six categories)


def random_block(rng, first, q_dc, q_ac, budget):
    """16 levels in scan order (zero below `first`) whose dequantised magnitudes sum to <= budget, and the tail flag.  Styles: empty, one level, sparse,
    dense, one large value; magnitudes drawn per token category, then cut to what the budget still allows"""
    lv = np.zeros(16, np.int64)
    style = rng.choice(["empty", "one", "sparse", "dense", "large", "zeros"], p=[0.2, 0.15, 0.25, 0.2, 0.1, 0.1])
    budget = min(budget, int(rng.choice([budget, 2000, 500, 120])))
    def mag(hi_cat):
        lo, hi = MAGNITUDES[int(rng.integers(0, hi_cat))]
        return int(rng.integers(lo, hi + 1))
    if style == "one":
        lv[int(rng.integers(first, 16))] = mag(9)
    elif style == "sparse":
        for n in rng.choice(np.arange(first, 16), int(rng.integers(2, 6)), replace=False):
            lv[n] = mag(7)
    elif style == "dense":
        for n in range(first, 16):
            lv[n] = mag(4) if rng.random() < 0.9 else 0
    elif style == "large":
        lv[int(rng.integers(first, 16))] = mag(9)
        lv[int(rng.integers(first, 16))] = int(rng.integers(67, 2048))
    rem = budget
    for n in rng.permutation(16):
        q = q_dc if n == 0 else q_ac
        lv[n] = min(int(lv[n]), rem // q)
        rem -= int(lv[n]) * q
    lv *= rng.choice([-1, 1], 16)
    tail = style == "zeros" or rng.random() < 0.08
    return lv, bool(tail)


def random_mbs(rng, mbw, mbh, quant, *, nseg=1, p_skip=0.15, p_i4=0.5, p_empty=0.1, skip_rows=(), amplitude=1.0):
    """macroblocks with every mode drawn uniformly; quant = quantisers(...) of the frame they go into.  p_empty: macroblocks whose skip flag is clear and
    that code nothing; half of those that are i16 get a Y2 block of zero tokens up to position 16 (it counts as coded and transforms to nothing)"""
    out = []
    for my in range(mbh):
        for mx in range(mbw):
            mb = MB(segment=int(rng.integers(0, nseg)), skip=int(my in skip_rows or rng.random() < p_skip), i4=int(rng.random() < p_i4),
                    ymode=int(rng.integers(0, 4)), bmodes=[int(m) for m in rng.integers(0, 10, 16)], uvmode=int(rng.integers(0, 4)))
            q = quant[mb.segment]
            if rng.random() < p_empty:
                if not mb.i4 and rng.random() < 0.5:
                    mb.tail[24] = True
            else:
                for b in range(25):
                    if b == 24 and mb.i4:
                        continue
                    if b == 24:
                        lv, tail = random_block(rng, 0, q[2], q[3], int(BLOCK_SUM_MAX * amplitude))
                    elif b < 16:
                        lv, tail = random_block(rng, 0 if mb.i4 else 1, q[0], q[1], int((BLOCK_SUM_MAX if mb.i4 else I16_AC_SUM_MAX) * amplitude))
                    else:
                        lv, tail = random_block(rng, 0, q[4], q[5], int(BLOCK_SUM_MAX * amplitude))
                    mb.levels[b], mb.tail[b] = lv, tail
            out.append(mb)
    return out


def random_frame(rng, width, height, mb_kw=None, **hdr):
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4
    quant = quantisers(hdr.get("base_q", 0), hdr.get("q_delta", (0, 0, 0, 0, 0)), hdr.get("segment"))
    mb_kw = dict(mb_kw or {})
    if hdr.get("segment") and hdr["segment"].get("update_map"):
        mb_kw.setdefault("nseg", 4)
    return write_frame(width, height, random_mbs(rng, mbw, mbh, quant, **mb_kw), **hdr)
