"""The catalogue of the inflate tests: PNG files whose IDAT streams take every shape a DEFLATE stream can take (valid ones, from zlib
and from tests/_deflate.py), and streams every decoder must refuse.  Each case says what it is for; facts() measures what a case
really exercises from what the writer recorded, and VALID_ITEMS / INVALID_ITEMS list what the catalogue as a whole must reach.

k_png_huff's round geometry is read from its source (CSP_HUFF_SUB / _PRE / _WAVES), so the boundary cases follow a retune; the
emulation build plays one wave of 64 lanes, so boundaries are placed for both 64 and 64 * CSP_HUFF_WAVES lanes."""
import functools
import os
import re
import zlib

import numpy as np

import _deflate as D
from _deflate import Match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def geometry():
    src = open(os.path.join(ROOT, "caesium-clt_amd", "csrc", "k_png_inflate.hip")).read()

    def get(pat):
        return int(re.search(pat, src).group(1))
    return dict(sub=get(r"#define CSP_HUFF_SUB (\d+)"), pre=get(r"#define CSP_HUFF_PRE (\d+)"), lanes=64 * get(r"#define CSP_HUFF_WAVES (\d+)"),
                piece=get(r"LZ_PIECE = (\d+)"))


class Case:
    """one PNG: `data` is everything its zlib stream decodes to (zlib's view), `raw` the image's share of it"""

    def __init__(self, name, items, z, data, width, height, ctype=0, depth=8, plte=None, idat_sizes=None, d=None, complete=True, irreducible=False):
        self.name, self.items, self.z, self.data = name, set(items), z, bytes(data)
        self.width, self.height, self.ctype, self.depth, self.plte = width, height, ctype, depth, plte
        self.raw = self.data[:height * (1 + D.rowbytes(width, ctype, depth))]
        self.d, self.complete, self.irreducible = d, complete, irreducible
        self.png = D.png_file(z, width, height, ctype, depth, idat_sizes=idat_sizes, plte=plte)

    def __repr__(self):
        return "Case(%s)" % self.name


# ---------------------------------------------------------------- pictures
PICTURES = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]


def picture(ctype, depth, w, h, seed):
    """(rows, palette) of a textured picture; RGB / RGBA at 8 bits have thousands of colours, are not grey and not opaque (irreducible)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    nc = D.CHANNELS[ctype]
    maxv = (1 << depth) - 1
    chans = []
    for c in range(nc):
        v = (xx * (3 + 2 * c) + yy * (5 - c) + 40 * np.sin((xx + 3 * yy) / (7.0 + c))) / (w + h) * maxv * 0.8 + rng.normal(0, maxv * 0.06, (h, w))
        chans.append(np.clip(v, 0, maxv).astype(np.int64))
    if ctype == 3:
        chans = [chans[0] % min(200, maxv + 1)]
    s = np.stack(chans, axis=2)
    if depth == 16:
        rows = np.stack([s >> 8, s & 255], axis=3).reshape(h, -1).astype(np.uint8)
    elif depth == 8:
        rows = s.reshape(h, -1).astype(np.uint8)
    else:
        bits = ((s.reshape(h, w, 1) >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, -1).astype(np.uint8)
        rows = np.packbits(bits, axis=1)
    plte = bytes(rng.integers(0, 256, 3 * min(200, 1 << depth), dtype=np.uint8)) if ctype == 3 else None
    return rows, plte


def zlib_case(name, items, ctype, depth, w, h, seed, level=6, wbits=15, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, every=1, idat_sizes=None):
    rows, plte = picture(ctype, depth, w, h, seed)
    bpp = max(1, D.CHANNELS[ctype] * depth // 8)
    raw = D.filter_rows(rows, bpp, [(seed + k) % 5 for k in range(5)])
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    rb = 1 + rows.shape[1]
    z = b""
    for y in range(h):
        z += c.compress(raw[y * rb:(y + 1) * rb])
        if flush is not None and y % every == every - 1:
            z += c.flush(flush)
    z += c.flush()
    return Case(name, items, z, raw, w, h, ctype, depth, plte=plte, idat_sizes=idat_sizes, irreducible=depth == 8 and ctype in (2, 6))


def encoder_variety():
    out = []
    pics = [(2, 8, 96, 64), (6, 8, 70, 50), (0, 8, 120, 90), (4, 8, 80, 60), (3, 8, 100, 70), (0, 16, 60, 50), (2, 16, 50, 40), (6, 16, 40, 30),
            (4, 16, 50, 40), (0, 1, 300, 90), (0, 2, 200, 80), (0, 4, 150, 70), (3, 1, 260, 60), (3, 2, 190, 50), (3, 4, 130, 40)]
    k = 0

    def nxt():
        nonlocal k
        k += 1
        return pics[k % len(pics)]
    for level in range(10):
        ct, dp, w, h = nxt()
        out.append(zlib_case("zlib_level%d" % level, {"zlib_level_%d" % level}, ct, dp, w, h, 100 + level, level=level))
    for sname, st in (("default", zlib.Z_DEFAULT_STRATEGY), ("filtered", zlib.Z_FILTERED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("fixed", zlib.Z_FIXED)):
        for level in (1, 9):
            ct, dp, w, h = nxt()
            out.append(zlib_case("zlib_%s_l%d" % (sname, level), {"strategy_" + sname}, ct, dp, w, h, 120 + k, level=level, strategy=st))
    for wbits in range(9, 16):
        ct, dp, w, h = nxt()
        out.append(zlib_case("zlib_wbits%d" % wbits, {"wbits_%d" % wbits}, ct, dp, w, h, 140 + wbits, level=9, wbits=wbits))
    for mem in (1, 9):
        ct, dp, w, h = nxt()
        out.append(zlib_case("zlib_mem%d" % mem, {"memlevel_%d" % mem}, ct, dp, w, h, 160 + mem, level=6, mem=mem))
    for fname, fl in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH), ("partial", zlib.Z_PARTIAL_FLUSH), ("block", zlib.Z_BLOCK)):
        for every in (1, 5):
            ct, dp, w, h = nxt()
            out.append(zlib_case("zlib_flush_%s_%d" % (fname, every), {"flush_%s_%s" % (fname, "row" if every == 1 else "rows")}, ct, dp, w, h, 170 + k,
                                 level=6, flush=fl, every=every))
    for ct, dp in PICTURES:   # every colour type and depth once more, a default stream each
        w = {1: 170, 2: 120, 4: 90, 8: 64, 16: 40}[dp]
        out.append(zlib_case("picture_ct%d_d%d" % (ct, dp), set(), ct, dp, w, 48, 200 + 10 * ct + dp))
    out.append(zlib_case("idat_split", {"idat_split"}, 2, 8, 64, 40, 300, idat_sizes=[1, 0, 1, 0, 3, 1, 200, 0, 1]))
    return out


# ---------------------------------------------------------------- hand-written streams
def row_case(name, items, d, image_len=None, adler=True, tail=b"", cut=None, **zkw):
    """a one-row 8-bit grey picture of what `d` decodes to (its first byte is the filter byte), or of the first image_len bytes of it"""
    data = bytes(d.data)
    n = image_len or len(data)
    assert data[0] <= 4, name
    z = D.zlib_wrap(d.getvalue(), data, adler=adler, tail=tail, **zkw)
    if cut is not None:
        z = z[:cut]
    return Case(name, items, z, data, n - 1, 1, d=d, complete=adler and cut is None and any(b["final"] for b in d.blocks))


def lits(rng, n, lo=0, hi=256):
    return [int(v) for v in rng.integers(lo, hi, n)]


def fill_fixed(rng, bits, first=None):
    """fixed-code literals that take exactly `bits` bits (8-bit codes for 0..143, 9-bit codes for 144..255)"""
    y = bits % 8
    x = (bits - 9 * y) // 8
    assert x >= 0 and 8 * x + 9 * y == bits, bits
    out = lits(rng, x, 0, 144) + lits(rng, y, 144, 256)
    if first is not None:
        out[0] = first
    return out


def code_shapes():
    rng = np.random.default_rng(7)
    out = []
    # empty blocks of all three types between blocks with data; a dynamic empty block is a litlen code holding only EOB, at length 1
    d = D.Deflate()
    d.fixed([1] + lits(rng, 200))
    d.fixed([])
    d.dynamic([])
    d.stored(b"")
    d.dynamic(lits(rng, 300, 0, 40) + [Match(20, 250)])
    d.stored(b"")
    d.fixed(lits(rng, 50), final=True)
    out.append(row_case("empty_blocks", {"empty_blocks"}, d))
    # stored blocks of 0, 1 and 65535 bytes, and one between two dynamic blocks whose matches reach across it
    d = D.Deflate()
    d.stored(bytes([2]) + bytes(rng.integers(0, 256, 65534, dtype=np.uint8)))
    d.stored(b"\x07")
    d.stored(b"")
    d.dynamic(lits(rng, 3000, 0, 64))
    d.stored(bytes(rng.integers(0, 256, 2000, dtype=np.uint8)))
    d.dynamic(lits(rng, 10, 0, 64) + [Match(40, 2500), Match(100, 4900), Match(258, 3100)] + lits(rng, 10, 0, 64), final=True)
    out.append(row_case("stored_sizes_and_reach_across", {"stored_between_dynamic"}, d))
    # HLIT 257 with HDIST 1 and a zero length (literal-only); the fewest code length codes a valid block can have (5: 16, 17, 18, 0, 8 --
    # 16, 17, 18 and 0 alone cannot give EOB a length): 256 symbols of 8 bits, literal 255 left out
    d = D.Deflate()
    d.dynamic([0] + lits(rng, 500, 0, 200), hdist=1)
    lit = [8] * 255 + [0] + [8]
    d.dynamic(lits(rng, 400, 0, 255), lit=lit, dist=[0])
    d.dynamic(lits(rng, 300, 0, 30) + [Match(3, 7)], hclen=19, hlit=286, final=True)   # a run of zeros from litlen 258 into distance 4
    out.append(row_case("literal_only_and_hclen", set(), d))
    # one distance codeword of length 1 (HDIST 1): matches at distance 1 only
    d = D.Deflate()
    d.dynamic([3] + lits(rng, 100) + [Match(50, 1), 9, Match(258, 1)] + lits(rng, 20) + [Match(7, 1)], final=True)
    out.append(row_case("hdist1_one_codeword", set(), d))
    # litlen codewords of every length 1..15 and distance codewords of 11..15 bits, all on the true walk; HLIT 286; a run of zero
    # lengths that crosses from the litlen lengths into the distance lengths
    syms = list(range(11)) + [256, 257, 266, 284, 285]
    lens = list(range(1, 15)) + [15, 15]
    order = [3, 0, 5, 1, 7, 9, 2, 11, 4, 13, 6, 15, 8, 10, 12, 14]
    lit = [0] * 286
    for s, k in zip(syms, order):
        lit[s] = lens[k]
    dist = [0] * 30
    dsyms = list(range(10, 26))
    for s, l in zip(dsyms, lens):
        dist[s] = l
    body = [0] + [int(v) % 11 for v in rng.integers(0, 11, 9000)]
    toks = list(body)
    for s in dsyms:
        for ln in (3, 13, 14, 230, 258):
            toks.append(Match(ln, D.DIST_BASE[s] + (s % 3)))
            toks += [s % 11, 10]
    toks += list(range(11)) * 2
    d = D.Deflate()
    d.dynamic(toks, lit=lit, dist=dist, hlit=286, final=True)
    out.append(row_case("every_codeword_length", set(), d))
    # length 258 as code 285 and as 284 + 31; distance 1, 32768 and both sides of every distance code's boundary
    d = D.Deflate()
    toks = [4] + lits(rng, 33000)
    for i in range(1, 30):
        toks += [Match(5, D.DIST_BASE[i] - 1), int(rng.integers(0, 256)), Match(4, D.DIST_BASE[i]), int(rng.integers(0, 256))]
    toks += [Match(258, 1), Match(258, 1, True), Match(258, 32768), Match(258, 32768, True), Match(3, 1)]
    d.dynamic(toks[:20000])
    d.dynamic(toks[20000:], final=True)
    out.append(row_case("lengths_and_distances", set(), d))
    return out


def huff_geometry_cases():
    """blocks whose EOB starts / ends one bit before, at and one bit after a lane-stretch boundary and a round boundary (64 and
    CSP_HUFF_WAVES * 64 lanes), tokens across round boundaries, blocks shorter than a stretch, hundreds of tiny blocks, and the image's
    last byte in the middle of a run of literals / of a match with blocks behind it, or with no final block at all"""
    g = geometry()
    sub, lanes = g["sub"], g["lanes"]
    rng = np.random.default_rng(11)
    out = []
    for tag, b in (("lane", 37 * sub), ("lane1", sub), ("round64", 64 * sub), ("round%d" % lanes, lanes * sub)):
        d = D.Deflate()
        first = 1
        for where in ("start", "end"):
            for delta in (-1, 0, 1):
                t = b + delta - (7 if where == "end" else 0)
                d.fixed(fill_fixed(rng, t, first))
                first = None
        d.fixed(lits(rng, 10), final=True)
        out.append(row_case("eob_at_%s" % tag, set(), d))
    for nl in sorted({64, lanes}):
        d = D.Deflate()
        d.fixed(fill_fixed(rng, nl * sub - 5, 2) + [Match(258, 1)] + lits(rng, 100))       # 13 bits from 5 bits in front of the boundary
        d.fixed(fill_fixed(rng, nl * sub - 4) + [200] + lits(rng, 100))                    # a 9-bit literal from 4 bits in front of it
        d.fixed(fill_fixed(rng, nl * sub - 20) + [Match(258, 2077)] + lits(rng, 20), final=True)   # 22 bits from 20 in front of it
        out.append(row_case("token_across_round%d" % nl, set(), d))
    # hundreds of tiny blocks of every type (some empty); each shorter than a stretch
    d = D.Deflate()
    d.fixed([0, 5])
    for k in range(400):
        kind = k % 7
        if kind in (0, 3):
            d.fixed(lits(rng, int(rng.integers(0, 4))))
        elif kind in (1, 4, 6):
            d.dynamic(lits(rng, int(rng.integers(1, 5))) + ([Match(3, 2)] if k % 2 else []))
        elif kind == 2:
            d.stored(bytes(rng.integers(0, 256, int(rng.integers(0, 3)), dtype=np.uint8)))
        else:
            d.fixed([Match(4, 1)])
    d.fixed(lits(rng, 3), final=True)
    out.append(row_case("tiny_blocks", set(), d))
    # the image's last byte in the middle of a run of literals / of a match, with more blocks behind it; with no final block at all
    d = D.Deflate()
    d.dynamic([1] + lits(rng, 5000, 0, 100) + [Match(100, 300)] + lits(rng, 400, 0, 100))
    d.fixed(lits(rng, 100))
    d.dynamic(lits(rng, 1000), final=True)
    out.append(row_case("last_byte_in_literals", set(), d, image_len=5000 + 1 + 100 + 200))
    d = D.Deflate()
    d.dynamic([1] + lits(rng, 5000, 0, 100) + [Match(258, 4000)] + lits(rng, 400, 0, 100))
    d.stored(b"abc")
    d.fixed(lits(rng, 10), final=True)
    out.append(row_case("last_byte_in_match", set(), d, image_len=5001 + 100))
    d = D.Deflate()
    d.dynamic([1] + lits(rng, 3000, 0, 50))
    d.fixed(lits(rng, 500) + [Match(30, 10)] + lits(rng, 30))
    out.append(row_case("no_final_block", set(), d, image_len=3001 + 200, adler=False))
    d = D.Deflate()
    d.fixed([1] + lits(rng, 3000) + [Match(258, 2)] + lits(rng, 50), eob=False)
    out.append(row_case("no_final_block_mid_match", set(), d, image_len=3001 + 100, adler=False))
    return out


def worst_convergence():
    """a stream where a walk entered at a wrong bit never falls into step: a literal-only block of 30000 x literal 255 whose code is
    1^11 (litlen lengths 1, 2, .., 10 and two of 11 bits, 255 the higher of the two): the stream is all ones, every misaligned walk
    reads 255 after 255, and every lane's first guess is off (352 g - 192 = 6 mod 11), so the corrections run through all lanes"""
    lit = [0] * 257
    for s, l in zip([0, 1, 2, 3, 4, 5, 6, 7, 8, 256], range(1, 11)):
        lit[s] = l
    lit[254] = lit[255] = 11
    d = D.Deflate()
    d.dynamic([0] + [255] * 30000, lit=lit, dist=[0], final=True)
    return row_case("worst_convergence", {"convergence_worst"}, d)


def lz77_cases():
    """distance-1 chains through whole 16 KiB pieces of k_png_lz77 (the ring wraps), 258-byte matches at and across piece boundaries,
    distance 32768 from the first and the last byte of a piece"""
    P = geometry()["piece"]
    rng = np.random.default_rng(13)
    out = []
    row = np.zeros((1, 70000), np.uint8) + 77
    raw = D.filter_rows(row, 1, [0])
    c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    out.append(Case("zlib_rle_constant_row", {"lz77_dist1_pieces"}, c.compress(raw) + c.flush(), raw, 70000, 1))
    d = D.Deflate()
    d.fixed([0, 9] + [Match(258, 1)] * ((5 * P) // 258) + [1, 2], final=True)
    out.append(row_case("dist1_chain_five_pieces", set(), d))
    toks = [3]

    def to(pos):
        toks.extend(lits(rng, pos - len(D.expand(toks))))
    to(P)
    toks.append(Match(258, 8))          # from the first byte of piece 1
    to(2 * P - 100)
    toks.append(Match(258, 300))        # across the boundary into piece 2
    to(3 * P)
    toks.append(Match(258, 1))          # a run from the first byte of piece 3
    to(4 * P - 50)
    toks.append(Match(258, 1))          # a run across into piece 4
    to(5 * P)
    toks.append(Match(100, 32768))      # distance 32768 from the first byte of piece 5
    to(6 * P - 1)
    toks += [Match(10, 32768)] + lits(rng, 50)   # from the last byte of piece 5, on into piece 6
    d = D.Deflate()
    d.dynamic(toks[:40000])
    d.dynamic(toks[40000:], final=True)
    out.append(row_case("matches_at_piece_edges", set(), d))
    return out


def tail_cases():
    """damage that lies only behind the image's last byte: accepted, as libpng (Pillow) accepts it"""
    rng = np.random.default_rng(17)
    out = []

    def base():
        d = D.Deflate()
        d.dynamic([1] + lits(rng, 2000, 0, 80))
        return d
    d = base()
    d.header(True, 3)
    d.w.bits(0x5A5A, 16)
    out.append(row_case("tail_btype3", {"tail_btype3"}, d, image_len=1991, adler=False))   # (libpng reads on to the block's end: damage right
    # behind the image's last byte with no bytes in between is an error there)
    d = base()
    d.header(True, 2)
    d.dynamic_header([1] * 200 + [1] * 57, [1])   # 257 codes of one bit
    out.append(row_case("tail_oversubscribed", {"tail_oversubscribed"}, d, image_len=1991, adler=False))
    d = D.Deflate()
    d.fixed([1] + lits(rng, 1500) + [Match(20, 30000)] + lits(rng, 10), final=True)
    out.append(row_case("tail_distance_too_far", {"tail_distance_too_far"}, d, image_len=1501, adler=False))
    d = base()
    d.fixed(lits(rng, 5), final=True)
    out.append(row_case("tail_after_trailer", {"tail_after_trailer"}, d, tail=b"\x00garbage behind the trailer"))
    d = base()
    d.fixed(lits(rng, 5), final=True)
    out.append(row_case("tail_no_trailer", {"tail_no_trailer"}, d, adler=False))
    d = base()
    d.fixed(lits(rng, 5000), final=True)
    out.append(row_case("tail_truncated", {"tail_truncated"}, d, image_len=2001 + 100, cut=2 + (d.toks[2001 + 120][0] >> 3)))
    return out


def valid_cases():
    return encoder_variety() + code_shapes() + huff_geometry_cases() + [worst_convergence()] + lz77_cases() + tail_cases()


# ---------------------------------------------------------------- invalid streams
def invalid_cases():
    """streams that zlib refuses before the image's last byte.  The Adler-32 trailer is always right for what the writer meant, so a
    decoder that refuses does so for the damage, not for the trailer"""
    rng = np.random.default_rng(19)
    out = []

    def bad(name, build, expect, extra=50, cut=None, **zkw):
        d = D.Deflate()
        d.fixed([1] + lits(rng, 300))
        build(d)
        n = len(d.data)
        d.fixed(lits(rng, extra), final=True)
        z = D.zlib_wrap(d.getvalue(), d.data, **zkw)
        if cut is not None:
            z = z[:2 + cut(d)]
        c = Case(name, {name}, z, d.data, len(d.data) - 1, 1, d=d, complete=False)
        c.expect = expect   # what zlib says (None: no error, the stream just ends)
        out.append(c)
        return n

    toks = lits(rng, 200, 0, 30) + [Match(10, 100), Match(20, 50)]
    lf, df = D.symbol_counts(toks)
    lit, dist = D.huffman_lengths(lf, 15), D.huffman_lengths(df, 15)

    def with_lit(change):
        def build(d):
            l2 = list(lit)
            change(l2)
            d.dynamic(toks, lit=l2, dist=dist)
        return build

    def with_dist(change):
        def build(d):
            d2 = list(dist)
            change(d2)
            d.dynamic(toks, lit=lit, dist=d2)
        return build
    bad("oversub_litlen", with_lit(lambda l: l.__setitem__(280, 1)), "invalid literal/lengths set")
    bad("oversub_dist", with_dist(lambda l: l.__setitem__(0, 1) or l.__setitem__(1, 1) or l.__setitem__(2, 1)), "invalid distances set")
    bad("incomplete_litlen", with_lit(lambda l: l.__setitem__(l.index(max(l)), max(l) + 1)), "invalid literal/lengths set")
    bad("incomplete_dist", with_dist(lambda l: l.__setitem__(l.index(max(l)), max(l) + 1)), "invalid distances set")
    # the code length code over-subscribed / incomplete with several codewords
    seq = D.rle_lengths(lit[:max(i for i, v in enumerate(lit) if v) + 1] + dist[:max(i for i, v in enumerate(dist) if v) + 1])
    cl = D.huffman_lengths([sum(1 for s, _ in seq if s == k) for k in range(19)], 7)
    bad("oversub_codelen", lambda d: d.dynamic(toks, lit=lit, dist=dist, cl=[1 if v else 0 for v in cl]), "invalid code lengths set")
    bad("incomplete_codelen", lambda d: d.dynamic(toks, lit=lit, dist=dist, cl=[v + 1 if v else 0 for v in cl]), "invalid code lengths set")
    # a single codeword of length 2 or more: litlen holding only EOB; distance code of one symbol
    for n in (2, 5):
        bad("single_litlen_len%d" % n, lambda d, n=n: d.dynamic([], lit=[0] * 256 + [n], dist=[0]), "invalid literal/lengths set")
    mt = lits(rng, 20, 0, 50) + [Match(30, 4), Match(5, 4)]
    mlf, _ = D.symbol_counts(mt)
    for n in (2, 3, 7):
        bad("single_dist_len%d" % n, lambda d, n=n: d.dynamic(mt, lit=D.huffman_lengths(mlf, 15), dist=[0, 0, 0, n]), "invalid distances set")
    for h in (287, 288):
        bad("hlit_%d" % h, lambda d, h=h: d.dynamic(toks, lit=lit + [0] * 10, dist=dist, hlit=h), "too many length or distance symbols")
    for h in (31, 32):
        bad("hdist_%d" % h, lambda d, h=h: d.dynamic(toks, lit=lit, dist=dist + [0] * 10, hdist=h), "too many length or distance symbols")
    cl_all = D.huffman_lengths([1] * 19, 7)   # a complete code over all 19 code length symbols
    lens_all = lit[:max(i for i, v in enumerate(lit) if v) + 1] + dist[:30]
    bad("code16_first", lambda d: d.dynamic(toks, lit=lit, dist=dist, hdist=30, seq=[(16, 0)] + D.rle_lengths(lens_all), cl=cl_all), "invalid bit length repeat")
    bad("repeat_past_end", lambda d: d.dynamic(toks, lit=lit, dist=dist, hdist=30, seq=D.rle_lengths(lens_all[:-3]) + [(18, 0)], cl=cl_all), "invalid bit length repeat")
    bad("eob_missing", lambda d: d.dynamic(toks[:200], lit=D.huffman_lengths(D.symbol_counts(toks[:200])[0][:256] + [0], 15), dist=[0]), "missing end-of-block")
    bad("hclen_4", lambda d: d.dynamic([], lit=[0] * 257, dist=[0], hclen=4, seq=[(18, 127), (18, 109)], cl=[0] * 17 + [1, 1]), "missing end-of-block")
    fl = D.canonical(D.FIXED_LIT)

    def fixed_raw(sym, dsym=None):
        def build(d):
            d.fixed(lits(rng, 20), eob=False)
            d.w.code(fl[sym], D.FIXED_LIT[sym])
            if dsym is not None:
                d.w.code(dsym, 5)
            d.data += bytes(10)   # what the image would have needed
            d.w.code(0, 7)        # EOB
        return build
    bad("fixed_litlen_286", fixed_raw(286), "invalid literal/length code")
    bad("fixed_litlen_287", fixed_raw(287), "invalid literal/length code")
    bad("fixed_dist_30", fixed_raw(257, 30), "invalid distance code")
    bad("fixed_dist_31", fixed_raw(257, 31), "invalid distance code")
    bad("dist_too_far", lambda d: d.fixed([Match(3, len(d.data) + 1)]), "invalid distance too far back")
    bad("stored_len_nlen", lambda d: d.stored(b"abcdefgh", nlen=0xFFF7 ^ 1), "invalid stored block lengths")
    bad("btype_3", lambda d: (d.header(False, 3), d.w.bits(0x1234, 16), d.data.extend(bytes(20))), "invalid block type")
    bad("zlib_fdict", lambda d: None, "Error 2 ", fdict=True)   # Z_NEED_DICT
    bad("zlib_cinfo_8", lambda d: None, "invalid window size", cinfo=8)

    # the one incomplete code that is accepted, a single codeword of length 1 ('0'), with the stream on its unassigned half ('1')
    def lit_bit1(d):
        d.dynamic([], lit=[0] * 256 + [1], dist=[0], eob=False)
        d.w.bits(1, 1)
        d.data += bytes(10)   # what the image would have needed
    bad("single_litlen_len1_bit1", lit_bit1, "invalid literal/length code")
    m1 = lits(rng, 20, 0, 50) + [Match(5, 1)]
    l1 = D.huffman_lengths(D.symbol_counts(m1)[0], 15)

    def dist_bit1(d):
        d.dynamic(m1, lit=l1, dist=[1], eob=False)
        d.w.code(D.canonical(l1)[259], l1[259])   # length 5, then distance code '1'
        d.w.bits(1, 1)
        d.data += bytes(10)
    bad("single_dist_len1_bit1", dist_bit1, "invalid distance code")
    bad("trunc_dynamic_header", lambda d: d.dynamic(toks, lit=lit, dist=dist), None, cut=lambda d: (d.blocks[1]["start"] - 40) >> 3)
    bad("trunc_stored_payload", lambda d: d.stored(bytes(rng.integers(0, 256, 1000, dtype=np.uint8))), None, cut=lambda d: (d.blocks[1]["start"] >> 3) + 4 + 500)
    bad("trunc_token", lambda d: d.dynamic(toks, lit=lit, dist=dist), None, cut=lambda d: (next(t for t in d.toks if t[5] and t[0] > d.blocks[1]["start"])[0] >> 3) + 1)
    return out


# ---------------------------------------------------------------- what the catalogue reaches
VALID_ITEMS = (
    ["zlib_level_%d" % k for k in range(10)] + ["strategy_" + s for s in ("default", "filtered", "huffman_only", "rle", "fixed")]
    + ["wbits_%d" % k for k in range(9, 16)] + ["memlevel_1", "memlevel_9"]
    + ["flush_%s_%s" % (f, e) for f in ("sync", "full", "partial", "block") for e in ("row", "rows")]
    + ["picture_ct%d_d%d" % p for p in PICTURES] + ["irreducible_ct2", "irreducible_ct6", "idat_split", "idat_split_in_zlib_header"]
    + ["empty_fixed", "empty_dynamic", "empty_stored", "stored_0", "stored_1", "stored_65535", "stored_between_dynamic",
       "hlit_257", "hlit_286", "hdist_1_zero", "hdist_1_len1", "hdist_30", "hclen_fewest", "hclen_19", "cl_run_crosses", "eob_only_len1"]
    + ["litlen_len_%d" % k for k in range(1, 16)] + ["dist_len_%d" % k for k in range(11, 16)]
    + ["len258_285", "len258_284_31", "dist_1", "dist_32768"] + ["dist_boundary_%d_%s" % (i, s) for i in range(1, 30) for s in ("below", "at")]
    + ["eob_%s_%s_%s" % (w, b, d) for w in ("start", "end") for b in ("lane", "round64", "roundN") for d in ("m1", "0", "p1")]
    + ["token_across_round64", "token_across_roundN", "block_shorter_than_stretch", "tiny_blocks_200",
       "last_byte_in_literals_more_blocks", "last_byte_in_match_more_blocks", "last_byte_no_final_block", "convergence_worst"]
    + ["lz77_dist1_pieces", "len258_at_piece_start", "len258_across_piece", "dist32768_piece_first", "dist32768_piece_last"]
    + ["tail_btype3", "tail_oversubscribed", "tail_distance_too_far", "tail_after_trailer", "tail_no_trailer", "tail_truncated"])

INVALID_ITEMS = (["oversub_litlen", "oversub_dist", "oversub_codelen", "incomplete_litlen", "incomplete_dist", "incomplete_codelen",
                  "single_litlen_len2", "single_litlen_len5", "single_dist_len2", "single_dist_len3", "single_dist_len7",
                  "single_litlen_len1_bit1", "single_dist_len1_bit1",
                  "hlit_287", "hlit_288", "hdist_31", "hdist_32", "code16_first", "repeat_past_end", "eob_missing", "hclen_4",
                  "fixed_litlen_286", "fixed_litlen_287", "fixed_dist_30", "fixed_dist_31", "dist_too_far", "stored_len_nlen", "btype_3",
                  "zlib_fdict", "zlib_cinfo_8", "trunc_dynamic_header", "trunc_stored_payload", "trunc_token"])


def facts(case):
    """what a case exercises: its labels, plus what the writer's record shows on the image's true walk"""
    f = set(case.items)
    f.add("picture_ct%d_d%d" % (case.ctype, case.depth))
    if case.irreducible:
        f.add("irreducible_ct%d" % case.ctype)
    at = case.png.index(b"IDAT")
    if case.png.count(b"IDAT") > 2 and int.from_bytes(case.png[at - 4:at], "big") < 2:
        f.add("idat_split_in_zlib_header")
    d = case.d
    if d is None:
        return f
    g = geometry()
    sub, P, n = g["sub"], g["piece"], len(case.raw)
    live = [t for t in d.toks if t[2] < n]   # tokens that start in front of the image's last byte
    for t in live:
        f.add("litlen_len_%d" % t[3])
        if t[5]:
            f.add("dist_len_%d" % t[4])
            if t[5] == 258:
                f.add("len258_284_31" if t[7] else "len258_285")
            if t[6] in (1, 32768):
                f.add("dist_%d" % t[6])
            for i in range(1, 30):
                if t[6] in (D.DIST_BASE[i] - 1, D.DIST_BASE[i]):
                    f.add("dist_boundary_%d_%s" % (i, "at" if t[6] == D.DIST_BASE[i] else "below"))
            if t[2] % P == 0 and t[5] == 258:
                f.add("len258_at_piece_start")
            if t[5] == 258 and t[2] // P != (t[2] + 257) // P:
                f.add("len258_across_piece")
            if t[6] == 32768 and t[2] % P == 0:
                f.add("dist32768_piece_first")
            if t[6] == 32768 and t[2] % P == P - 1 and t[5] > 1:
                f.add("dist32768_piece_last")
            if t[6] == 1 and t[2] + t[5] > 4 * P:
                run = [u for u in live if u[5] and u[6] == 1]
                if len(run) * 258 >= 4 * P:
                    f.add("lz77_dist1_pieces")
    blocks = [b for b in d.blocks if b.get("out", n) < n]
    ntiny = 0
    for b in blocks:
        if b["type"] == 0:
            f.add({0: "stored_0", 1: "stored_1", 65535: "stored_65535"}.get(b["stored"], "stored"))
            if b["stored"] == 0:
                f.add("empty_stored")
            continue
        if "start" not in b:
            continue
        toks = [t for t in d.toks if b["start"] <= t[0] < b["end"]]
        if not toks:
            f.add("empty_fixed" if b["type"] == 1 else "empty_dynamic")
        if b["end"] - b["start"] < sub:
            ntiny += 1
            if toks:
                f.add("block_shorter_than_stretch")
        if b["type"] == 2:
            f.add("hlit_%d" % b["hlit"]) if b["hlit"] in (257, 286) else None
            dl = b["dist"][:b["hdist"]] + [0] * max(0, b["hdist"] - len(b["dist"]))
            if b["hdist"] == 1:
                f.add("hdist_1_zero" if dl[0] == 0 else "hdist_1_len1" if dl[0] == 1 else "hdist_1")
            if b["hdist"] == 30:
                f.add("hdist_30")
            if b["hclen"] == 19:
                f.add("hclen_19")
            if b["hclen"] == 5:
                f.add("hclen_fewest")
            if sorted(l for l in b["lit"] if l) == [1] and b["lit"][256] == 1:
                f.add("eob_only_len1")
            at = 0
            for s, e in b["seq"]:
                k = 1 if s < 16 else (3 if s < 18 else 11) + e
                if s >= 16 and at < b["hlit"] < at + k:
                    f.add("cl_run_crosses")
                at += k
        if b.get("eob") is not None and b["eob"] is not None:
            for what, bit in (("start", b["eob"]), ("end", b["end"])):
                r = bit - b["start"]
                for delta, tag in ((-1, "m1"), (0, "0"), (1, "p1")):
                    q, m = divmod(r - delta, sub)
                    if m == 0 and 1 <= q < 64:
                        f.add("eob_%s_lane_%s" % (what, tag))
                    if m == 0 and q == 64:
                        f.add("eob_%s_round64_%s" % (what, tag))
                    if m == 0 and q == g["lanes"]:
                        f.add("eob_%s_roundN_%s" % (what, tag))
        for nl, tag in ((64, "round64"), (g["lanes"], "roundN")):
            edge = b["start"] + nl * sub
            if any(t[0] < edge < t[0] + t[1] for t in toks):
                f.add("token_across_" + tag)
    if ntiny >= 200:
        f.add("tiny_blocks_200")
    last = [t for t in d.toks if t[2] <= n - 1 < t[2] + max(1, t[5])]
    if last and n < len(case.data):
        t = last[0]
        more = any(b["at"] > t[0] and ("start" in b or b["type"] == 0) for b in d.blocks)
        i = d.toks.index(t)
        if t[5] and more:
            f.add("last_byte_in_match_more_blocks")
        if not t[5] and more and 0 < i < len(d.toks) - 1 and not d.toks[i - 1][5] and not d.toks[i + 1][5]:
            f.add("last_byte_in_literals_more_blocks")
        if not any(b["final"] for b in d.blocks):
            f.add("last_byte_no_final_block")
    return f


@functools.lru_cache(None)
def cached_valid():
    return valid_cases()


@functools.lru_cache(None)
def cached_invalid():
    return invalid_cases()
