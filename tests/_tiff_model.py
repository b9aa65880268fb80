"""A TIFF reader and the statement of the TIFF route's output rule, in plain Python from the TIFF 6.0 text (zlib for Deflate).  The reader takes a
file apart into pages, tags and segments and decodes the segments; recode() says, byte for byte, what the route must return for a file."""
import struct
import zlib

import _tiff_write as W

TYPE_SIZE = W.TYPE_SIZE
REWRITTEN = {259, 273, 278, 279, 317, 324, 325}
DROPPED = {270, 271, 272, 305, 306, 315, 700, 33432, 33723, 34377, 34665, 34853}
CODED = {1, 5, 8, 32946, 32773}


class BadTiff(Exception):
    pass


# ------------------------------------------------------------------------------------------------ the reader
def read_ifd(d, E, off):
    """-> ([(tag, type, count, value bytes)], next): BadTiff for anything outside the file, None in place of the entries for a field type that cannot be sized"""
    entries, nxt, sized = read_ifd_sized(d, E, off)
    return (entries if sized else None), nxt


def read_ifd_sized(d, E, off):
    """-> (the entries whose field type can be sized, next, whether that is all of them)"""
    if off + 2 > len(d):
        raise BadTiff("IFD offset outside the file")
    n = struct.unpack_from(E + "H", d, off)[0]
    if off + 2 + 12 * n + 4 > len(d):
        raise BadTiff("IFD ends behind the file")
    entries, sized = [], True
    for k in range(n):
        tag, typ, count = struct.unpack_from(E + "HHI", d, off + 2 + 12 * k)
        if typ not in TYPE_SIZE:
            sized = False
            continue
        size = count * TYPE_SIZE[typ]
        at = off + 2 + 12 * k + 8
        if size > 4:
            at = struct.unpack_from(E + "I", d, at)[0]
        if at + size > len(d):
            raise BadTiff("value outside the file")
        entries.append((tag, typ, count, bytes(d[at:at + size])))
    return entries, struct.unpack_from(E + "I", d, off + 2 + 12 * n)[0], sized


def numbers(E, entry):
    tag, typ, count, raw = entry
    fmt = {1: "B", 3: "H", 4: "I", 13: "I"}.get(typ)
    return list(struct.unpack(E + "%d%s" % (count, fmt), raw)) if fmt else [0] * count


def parse(d):
    """-> dict(big_endian, pages, why): why is None for a file the route codes, else the reason it is passed through.  A page: dict(entries, width, height, spp,
    bits, comp, pred (0 / 8 / 16: the input's), pred_ok (the depth the output may difference at, 0 for none), tiled, rowbytes, seg_rows (per segment), segs
    [(off, len)], tile, exif, gps)"""
    if len(d) < 8 or d[:2] not in (b"II", b"MM"):
        raise BadTiff("no header")
    big = d[:2] == b"MM"
    E = ">" if big else "<"
    if struct.unpack_from(E + "H", d, 2)[0] != 42:
        raise BadTiff("not a classic TIFF")
    off, seen, pages, why, total = struct.unpack_from(E + "I", d, 4)[0], set(), [], None, 0
    while off:
        if off in seen:
            raise BadTiff("the IFD chain loops")
        seen.add(off)
        if len(seen) > 65535:
            why = why or "pages"
            break
        entries, off, sized = read_ifd_sized(d, E, off)
        if not sized:
            why = why or "field type"
        tags = {e[0]: e for e in entries}

        def num(tag, default):
            return numbers(E, tags[tag])[0] if tag in tags and tags[tag][2] else default
        if 256 not in tags or 257 not in tags:
            raise BadTiff("no ImageWidth / ImageLength")
        w, h = num(256, 0), num(257, 0)
        if not w or not h:
            raise BadTiff("zero width or height")
        spp, comp = num(277, 1), num(259, 1)
        if not spp:
            raise BadTiff("SamplesPerPixel 0")
        if spp > 65535:   # (the tag is a SHORT by the text)
            why = why or "samples"
            pages.append(dict(entries=entries))
            continue
        b = numbers(E, tags[258]) if 258 in tags else [1]
        bits = [b[k] if len(b) == spp else b[0] for k in range(spp)]
        if 0 in bits:
            raise BadTiff("BitsPerSample 0")
        if sum(bits) > 1 << 20:
            why = why or "size"
            pages.append(dict(entries=entries))
            continue
        pred_ok = 0 if spp > 64 else 8 if all(x == 8 for x in bits) else 16 if all(x == 16 for x in bits) else 0
        predictor, pred = num(317, 1), 0
        if predictor == 2:
            pred = pred_ok
            if not pred_ok:
                why = why or "predictor depth"
        elif predictor != 1:
            why = why or "predictor"
        if comp not in CODED:
            why = why or "compression"
        if num(284, 1) == 2:
            why = why or "planar"
        if num(266, 1) == 2:
            why = why or "fill order"
        if 330 in tags:
            why = why or "SubIFDs"
        if num(262, 0) == 6 and (530 not in tags or tags[530][2] < 2 or numbers(E, tags[530])[:2] != [1, 1]):
            why = why or "YCbCr subsampling"
        tiled = any(t in tags for t in (322, 323, 324, 325))
        to, tc = (324, 325) if tiled else (273, 279)
        if to not in tags or tc not in tags or (tiled and (322 not in tags or 323 not in tags)):
            raise BadTiff("a required tag is missing")
        if tiled:
            tw, tl = num(322, 0), num(323, 0)
            if not tw or not tl:
                raise BadTiff("zero tile")
            nseg = -(-w // tw) * -(-h // tl)
            seg_rows, segw = [tl] * nseg, tw
        else:
            rps = min(num(278, 0xFFFFFFFF), h)
            if not rps:
                raise BadTiff("RowsPerStrip 0")
            nseg = -(-h // rps)
            seg_rows, segw, tw, tl = [min(rps, h - k * rps) for k in range(nseg)], w, 0, 0
        rowbytes = (segw * sum(bits) + 7) // 8
        p = dict(entries=entries, width=w, height=h, spp=spp, bits=bits, comp=comp, pred=pred, pred_ok=pred_ok, tiled=tiled, rowbytes=rowbytes, seg_rows=seg_rows, segs=[], tile=(tw, tl), exif=None, gps=None)
        rows = sum(seg_rows)
        if rowbytes > 1 << 31 or nseg > 1 << 20 or rows > 1 << 20 or rowbytes * rows > 1 << 31:
            why = why or "size"
            pages.append(p)
            continue
        if tags[to][2] != nseg or tags[tc][2] != nseg:
            raise BadTiff("offsets or byte counts of the wrong length")
        total += rowbytes * rows
        if why is None:
            for o, n in zip(numbers(E, tags[to]), numbers(E, tags[tc])):
                if o + n > len(d):
                    raise BadTiff("a segment outside the file")
                if comp == 5 and n >= 2 and d[o] == 0 and d[o + 1] & 1:
                    why = "old-style LZW"
                    break
                if comp in (8, 32946) and (n < 2 or d[o] & 15 != 8 or d[o] >> 4 > 7 or ((d[o] << 8) | d[o + 1]) % 31 or d[o + 1] & 0x20):
                    raise BadTiff("no zlib header")
                p["segs"].append((o, n))
        pages.append(p)
    if not pages and why is None:
        raise BadTiff("no IFD")
    if total > 1 << 31:
        why = why or "size"
    return dict(big_endian=big, pages=pages, why=why)


def lzw_decode(data, want):
    """TIFF 6.0 section 13, a code at a time; BadTiff("code") for a code beyond the next free entry, BadTiff("short") when EOI or the end comes too early"""
    table = [bytes([i]) for i in range(256)] + [b"", b""]
    out, pos, prev, total = bytearray(), 0, None, len(data) * 8
    while len(out) < want:
        width = min(12, (len(table) + 1).bit_length())
        if pos + width > total:
            break
        code = (int.from_bytes(data[pos >> 3:(pos >> 3) + 3].ljust(3, b"\0"), "big") >> (24 - (pos & 7) - width)) & ((1 << width) - 1)
        pos += width
        if code == 256:
            del table[258:]
            prev = None
            continue
        if code == 257:
            break
        if prev is None:
            if code > 257:
                raise BadTiff("code")
            s = table[code]
        else:
            if code < len(table):
                s = table[code]
            elif code == len(table) and len(table) < 4096:
                s = prev + prev[:1]
            else:
                raise BadTiff("code")
            if len(table) < 4096:
                table.append(prev + s[:1])
        out += s
        prev = s
    if len(out) < want:
        raise BadTiff("short")
    return bytes(out[:want])


def packbits_decode(data, want):
    out, pos = bytearray(), 0
    while len(out) < want:
        if pos >= len(data):
            raise BadTiff("short")
        h = data[pos]
        if h == 128:
            pos += 1
            continue
        n = h + 1 if h < 128 else 257 - h
        need = 1 + n if h < 128 else 2
        if pos + need > len(data):
            raise BadTiff("short")
        if len(out) + n > want:
            raise BadTiff("code")
        out += data[pos + 1:pos + 1 + n] if h < 128 else data[pos + 1:pos + 2] * n
        pos += need
    return bytes(out)


def unpredict(rows, spp, depth, big_endian):
    import numpy as np
    out = []
    for row in rows:
        a = np.frombuffer(row, dtype=np.uint8 if depth == 8 else (">u2" if big_endian else "<u2")).astype(np.int64).reshape(-1, spp)
        out.append((np.cumsum(a, axis=0) % (1 << depth)).astype(np.uint8 if depth == 8 else (">u2" if big_endian else "<u2")).tobytes())
    return out


def decode_segment(d, F, p, k):
    o, n = p["segs"][k]
    want = p["seg_rows"][k] * p["rowbytes"]
    data = d[o:o + n]
    if p["comp"] == 1:
        if n < want:
            raise BadTiff("short")
        raw = data[:want]
    elif p["comp"] == 5:
        raw = lzw_decode(data, want)
    elif p["comp"] == 32773:
        raw = packbits_decode(data, want)
    else:
        try:
            raw = zlib.decompressobj().decompress(data, want)
        except zlib.error:
            raise BadTiff("deflate")
        if len(raw) < want:
            raise BadTiff("short")
    if p["pred"]:
        rb = p["rowbytes"]
        raw = b"".join(unpredict([raw[y * rb:(y + 1) * rb] for y in range(p["seg_rows"][k])], p["spp"], p["pred"], F["big_endian"]))
    return raw


def decode_page(d, F, page):
    """the page's decoded bytes, predictor undone, the segments back to back"""
    p = F["pages"][page]
    return b"".join(decode_segment(d, F, p, k) for k in range(len(p["segs"])))


def picture(d, F, page):
    """the page as height rows of the picture's own row bytes (tiles put back in place; whole-byte pixels)"""
    p = F["pages"][page]
    raw = decode_page(d, F, page)
    if not p["tiled"]:
        return raw
    tw, tl = p["tile"]
    unit = sum(p["bits"])
    trb, across = p["rowbytes"], -(-p["width"] // tw)
    prb = (p["width"] * unit + 7) // 8
    rows = [bytearray() for _ in range(p["height"])]
    for k in range(len(p["segs"])):
        ty, tx = divmod(k, across)
        for y in range(tl):
            if ty * tl + y < p["height"]:
                rows[ty * tl + y] += raw[(k * tl + y) * trb:(k * tl + y + 1) * trb]
    return b"".join(bytes(r[:prb]) for r in rows)


# ------------------------------------------------------------------------------------------------ the output rule
def packbits_row(row):
    """a maximal run of at least 3 equal bytes: replicate packets of at most 128 (one left over: a literal of one); everything between such runs: literal packets of
    at most 128"""
    out, i, lit = bytearray(), 0, bytearray()

    def flush():
        for k in range(0, len(lit), 128):
            out.append(len(lit[k:k + 128]) - 1)
            out.extend(lit[k:k + 128])
        lit.clear()
    while i < len(row):
        j = i
        while j < len(row) and row[j] == row[i]:
            j += 1
        if j - i >= 3:
            flush()
            for k in range(i, j, 128):
                n = min(128, j - k)
                out.extend([(257 - n) & 255 if n > 1 else 0, row[i]])
        else:
            lit.extend(row[i:j])
        i = j
    flush()
    return bytes(out)


def strip_rows(p, strip_bytes):
    return max(1, min(p["height"], strip_bytes // p["rowbytes"]))


def recode(d, compression, strip_bytes=65536, keep_metadata=False, verdicts=None):
    """what the route returns for the file d: compression "none" / "lzw" / "packbits".  The input's bytes for a file that is passed through; BadTiff for a malformed one.
    Layout: the 8-byte header in the input's byte order; per page the segments, each at an even offset, then the out-of-line values in tag order at even offsets,
    then the IFD at an even offset; the last next-IFD pointer is 0.  verdicts: a list that takes, per page, whether Predictor 2 won (None where it was no candidate)"""
    F = parse(d)
    if F["why"]:
        return d
    big = F["big_endian"]
    E = ">" if big else "<"
    out = bytearray(d[:4] + b"\0\0\0\0")
    patch = 4

    def place(raw):
        if len(out) & 1:
            out.append(0)
        at = len(out)
        out.extend(raw)
        return at
    for k, p in enumerate(F["pages"]):
        raw = decode_page(d, F, k)
        rb = p["rowbytes"]
        R = p["tile"][1] if p["tiled"] else strip_rows(p, strip_bytes)
        rows = [raw[y * rb:(y + 1) * rb] for y in range(len(raw) // rb)]
        cut = [rows[y:y + R] for y in range(0, len(rows), R)]
        with_pred = False
        if compression == "none":
            segs = [b"".join(c) for c in cut]
        elif compression == "packbits":
            segs = [b"".join(packbits_row(r) for r in c) for c in cut]
        else:
            segs = [W.lzw_encode(b"".join(c)) for c in cut]
            if p["pred_ok"]:
                other = [W.lzw_encode(b"".join(W.predict(c, p["spp"], p["pred_ok"], big))) for c in cut]
                with_pred = sum(map(len, other)) < sum(map(len, segs))
                segs = other if with_pred else segs
        if verdicts is not None:
            verdicts.append(with_pred if compression == "lzw" and p["pred_ok"] else None)
        offs = [place(s) for s in segs]
        longs = lambda v: struct.pack(E + "%dI" % len(v), *v)
        shorts = lambda v: struct.pack(E + "%dH" % len(v), *v)
        ent = [e for e in p["entries"] if e[0] not in REWRITTEN and (keep_metadata or e[0] not in DROPPED)]
        subs = {}
        for tag in (34665, 34853):
            e = next((e for e in ent if e[0] == tag), None)
            if e is None:
                continue
            ent.remove(e)
            if e[2] == 1 and e[1] in (4, 13):   # a private IFD, copied one level deep without its interoperability pointer
                sub, _ = read_ifd(d, E, numbers(E, e)[0])
                if sub is None:
                    return d
                subs[tag] = [s for s in sub if s[0] != 40965]
                ent.append((tag, e[1], 1, None))
        ent.append((259, 3, 1, shorts([{"none": 1, "lzw": 5, "packbits": 32773}[compression]])))
        ent.append((324 if p["tiled"] else 273, 4, len(segs), longs(offs)))
        ent.append((325 if p["tiled"] else 279, 4, len(segs), longs([len(s) for s in segs])))
        if not p["tiled"]:
            ent.append((278, 4, 1, longs([R])))
        if with_pred:
            ent.append((317, 3, 1, shorts([2])))
        ent.sort(key=lambda e: e[0])

        def field(e, at):
            return struct.pack(E + "HHI", e[0], e[1], e[2]) + (e[3].ljust(4, b"\0") if at is None else struct.pack(E + "I", at))
        where = []
        for e in ent:
            if e[3] is None:
                at = [place(s[3]) if len(s[3]) > 4 else None for s in subs[e[0]]]
                where.append(place(struct.pack(E + "H", len(at)) + b"".join(field(s, a) for s, a in zip(subs[e[0]], at)) + b"\0\0\0\0"))
            else:
                where.append(place(e[3]) if len(e[3]) > 4 else None)
        ifd = place(struct.pack(E + "H", len(ent)) + b"".join(field(e if e[3] is not None else (e[0], e[1], e[2], b""), a) for e, a in zip(ent, where)) + b"\0\0\0\0")
        out[patch:patch + 4] = struct.pack(E + "I", ifd)
        patch = len(out) - 4
    return bytes(out)


def carried(F, page, keep_metadata=True):
    """the entries of a page that the route carries as they are: {tag: (type, count, value)}"""
    return {e[0]: e[1:] for e in F["pages"][page]["entries"] if e[0] not in REWRITTEN and e[0] not in (34665, 34853) and (keep_metadata or e[0] not in DROPPED)}
