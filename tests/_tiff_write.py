"""A TIFF writer for the tests of the TIFF route: classic TIFF in either byte order, strips or tiles, every compression the route decodes, with the stream shapes
real encoders never write (LZW without a leading Clear or without EOI, doubled Clears, Clears wherever asked, a table left to fill; PackBits with no-op headers
and packets that cross rows).  Written from the TIFF 6.0 text; tests/_tiff_model.py reads what this writes."""
import struct
import zlib

import numpy as np

BYTE, ASCII, SHORT, LONG, RATIONAL, UNDEFINED = 1, 2, 3, 4, 5, 7
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4}
NONE, LZW, DEFLATE, ADOBE_DEFLATE, PACKBITS = 1, 5, 8, 32946, 32773


class Bits:
    """codes packed from the high bit down"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def bytes(self):
        return bytes(self.out) + (bytes([(self.acc << (8 - self.n)) & 255]) if self.n else b"")


def lzw_codes(data, clears="spec", lead_clear=True, eoi=True, double=False):
    """[(code, width)] of TIFF LZW (section 13: Clear 256, EOI 257, first entry 258, the width one code early) over `data`, greedy longest match.  Code j behind a
    Clear is as wide as 258 + max(j, 1) is long, 12 at most, and adds entry 258 + j while that is below 4096.  clears: "spec" = a Clear right behind the code that
    adds entry 4094; an int N = a Clear behind every N codes; "never" = none: the table fills and the codes go on at 12 bits."""
    out, table, state = [], {}, {"j": 0, "since": 0}

    def width():
        return min(12, (258 + max(state["j"], 1)).bit_length())

    def clear():
        out.append((256, width()))
        state["j"] = 0
        if double:
            out.append((256, 9))
        table.clear()
        state["since"] = 0

    def emit(code, follow):
        out.append((code, width()))
        entry = 258 + state["j"]
        if follow is not None and entry < 4096:
            table[follow] = entry
        state["j"] += 1
        state["since"] += 1
        if (clears == "spec" and entry == 4094) or (isinstance(clears, int) and state["since"] >= clears):
            clear()

    if lead_clear:
        clear()
    cur = None
    for b in data:
        if cur is None:
            cur = b
        elif (cur, b) in table:
            cur = table[(cur, b)]
        else:
            emit(cur, (cur, b))
            cur = b
    if cur is not None:
        emit(cur, None)
    if eoi:
        out.append((257, width()))
    return out


def lzw_encode(data, **kw):
    bits = Bits()
    for code, width in lzw_codes(data, **kw):
        bits.put(code, width)
    return bits.bytes()


def packbits_encode(rows, noop=False, cross_rows=False):
    """rows: the segment's rows (bytes each).  Runs of 2 or more become replicate packets, the rest literal ones, 128 at most; cross_rows: the segment is coded as
    one row; noop: a 0x80 header in front of every packet"""
    out = bytearray()
    for row in ([b"".join(rows)] if cross_rows else rows):
        i = 0
        while i < len(row):
            run = 1
            while i + run < len(row) and run < 128 and row[i + run] == row[i]:
                run += 1
            if noop:
                out.append(0x80)
            if run >= 2:
                out += bytes([257 - run, row[i]])
                i += run
                continue
            j = i + 1
            while j < len(row) and j - i < 128 and not (j + 1 < len(row) and row[j] == row[j + 1]):
                j += 1
            out += bytes([j - i - 1]) + row[i:j]
            i = j
    return bytes(out)


def predict(rows, spp, depth, big_endian):
    """horizontal differencing (Predictor 2) of the rows of a segment: bytes at depth 8, 16-bit words in the file's byte order at depth 16"""
    out = []
    for row in rows:
        a = np.frombuffer(row, dtype=np.uint8 if depth == 8 else (">u2" if big_endian else "<u2")).astype(np.int64)
        d = a.copy()
        d[spp:] -= a[:-spp]
        out.append((d % (1 << depth)).astype(np.uint8 if depth == 8 else (">u2" if big_endian else "<u2")).tobytes())
    return out


def rowbytes_of(width, spp, bits):
    return (width * spp * bits + 7) // 8


def page(data, width, height, spp=1, bits=8, compression=NONE, rows_per_strip=None, tile=None, predictor=1, photometric=None, extra=(), exif=None, gps=None, lzw=None, packbits=None,
         zlevel=6, zstrategy=zlib.Z_DEFAULT_STRATEGY, planar=None, fillorder=None, surplus=b"", segments=None, drop=(), override=None):
    """one page: `data` is height rows of ceil(width * spp * bits / 8) bytes.  extra / exif / gps: [(tag, type, count, value bytes in the file's byte order)].
    segments: the coded segments as given, in place of what the codec would write; override: {tag: (type, count, value)} in place of what this writes; drop: tags left out"""
    if photometric is None:   # RGB for three samples and more (a fourth is written as unassociated alpha), else BlackIsZero
        photometric = 2 if spp >= 3 else 1
    return dict(data=bytes(data), width=width, height=height, spp=spp, bits=bits, compression=compression, rows_per_strip=rows_per_strip or height, tile=tile, predictor=predictor,
                photometric=photometric, extra=list(extra), exif=exif, gps=gps, lzw=lzw or {}, packbits=packbits or {}, zlevel=zlevel, zstrategy=zstrategy, planar=planar, fillorder=fillorder,
                surplus=surplus, segments=segments, drop=set(drop), override=override or {})


def segment_rows(p):
    """the rows of every segment: strips of rows_per_strip rows, or the tile grid, edge tiles padded with zeros"""
    rb = rowbytes_of(p["width"], p["spp"], p["bits"])
    rows = [p["data"][y * rb:(y + 1) * rb] for y in range(p["height"])]
    if not p["tile"]:
        r = p["rows_per_strip"]
        return [rows[y:y + r] for y in range(0, p["height"], r)]
    tw, tl = p["tile"]
    unit = p["spp"] * p["bits"]
    assert (tw * unit) % 8 == 0, "the test writer cuts tiles at byte boundaries"
    trb = tw * unit // 8
    out = []
    for y in range(0, p["height"], tl):
        for x in range(0, p["width"], tw):
            out.append([(rows[yy][x * unit // 8:x * unit // 8 + trb] if yy < p["height"] else b"").ljust(trb, b"\0") for yy in range(y, y + tl)])
    return out


def code_segment(p, rows, big_endian):
    if p["predictor"] == 2:
        rows = predict(rows, p["spp"], p["bits"], big_endian)
    c = p["compression"]
    if c == NONE:
        return b"".join(rows)
    if c == LZW:
        return lzw_encode(b"".join(rows), **p["lzw"])
    if c == PACKBITS:
        return packbits_encode(rows, **p["packbits"])
    z = zlib.compressobj(p["zlevel"], zlib.DEFLATED, 15, 8, p["zstrategy"])
    return z.compress(b"".join(rows)) + z.flush()


def tiff(pages, big_endian=False, first_ifd=None, next_of_last=0, type_sizes=None):
    """the file: header, then page by page the segments, the out-of-line values and the IFD.  next_of_last: the last IFD's next pointer ("first": the first IFD's offset, a loop);
    type_sizes: {field type: bytes} of field types TIFF does not know, for entries that carry one"""
    sizes = {**TYPE_SIZE, **(type_sizes or {})}
    E = ">" if big_endian else "<"
    out = bytearray((b"MM\0*" if big_endian else b"II*\0") + b"\0\0\0\0")
    patch, ifds = 4, []

    def value(tag, typ, count, raw):
        return (tag, typ, count, raw)

    def shorts(v):
        return struct.pack(E + "%dH" % len(v), *v)

    def longs(v):
        return struct.pack(E + "%dI" % len(v), *v)

    def place(raw):
        if len(out) & 1:
            out.append(0)
        at = len(out)
        out.extend(raw)
        return at

    def write_ifd(entries):
        """entries with their values; -> the IFD's offset (its next pointer is the last four bytes written)"""
        entries = sorted(entries, key=lambda e: e[0])
        fields = []
        for tag, typ, count, raw in entries:
            assert len(raw) == count * sizes[typ], (tag, typ, count, len(raw))
            fields.append(struct.pack(E + "HHI", tag, typ, count) + (raw.ljust(4, b"\0") if len(raw) <= 4 else struct.pack(E + "I", place(raw))))
        at = place(struct.pack(E + "H", len(fields)) + b"".join(fields) + b"\0\0\0\0")
        return at

    for p in pages:
        segs = p["segments"] if p["segments"] is not None else [code_segment(p, rows, big_endian) + p["surplus"] for rows in segment_rows(p)]
        offs = [place(s) for s in segs]
        ent = {256: value(256, LONG, 1, longs([p["width"]])), 257: value(257, LONG, 1, longs([p["height"]])), 258: value(258, SHORT, p["spp"], shorts([p["bits"]] * p["spp"])),
               259: value(259, SHORT, 1, shorts([p["compression"]])), 262: value(262, SHORT, 1, shorts([p["photometric"]])), 277: value(277, SHORT, 1, shorts([p["spp"]]))}
        if p["tile"]:
            ent[322] = value(322, SHORT, 1, shorts([p["tile"][0]])); ent[323] = value(323, SHORT, 1, shorts([p["tile"][1]]))
            ent[324] = value(324, LONG, len(segs), longs(offs)); ent[325] = value(325, LONG, len(segs), longs([len(s) for s in segs]))
        else:
            ent[273] = value(273, LONG, len(segs), longs(offs)); ent[278] = value(278, SHORT, 1, shorts([p["rows_per_strip"]])); ent[279] = value(279, LONG, len(segs), longs([len(s) for s in segs]))
        if p["photometric"] == 2 and p["spp"] == 4:
            ent[338] = value(338, SHORT, 1, shorts([2]))
        if p["predictor"] != 1:
            ent[317] = value(317, SHORT, 1, shorts([p["predictor"]]))
        if p["planar"] is not None:
            ent[284] = value(284, SHORT, 1, shorts([p["planar"]]))
        if p["fillorder"] is not None:
            ent[266] = value(266, SHORT, 1, shorts([p["fillorder"]]))
        for tag, typ, count, raw in p["extra"]:
            ent[tag] = value(tag, typ, count, raw)
        for tag, sub in ((34665, p["exif"]), (34853, p["gps"])):
            if sub is not None:
                ent[tag] = value(tag, LONG, 1, longs([write_ifd(sub)]))
        for tag, (typ, count, raw) in p["override"].items():
            ent[tag] = value(tag, typ, count, raw)
        for tag in p["drop"]:
            ent.pop(tag, None)
        at = write_ifd(list(ent.values()))
        ifds.append(at)
        out[patch:patch + 4] = struct.pack(E + "I", at)
        patch = len(out) - 4
    if first_ifd is not None:
        out[4:8] = struct.pack(E + "I", first_ifd)
    if next_of_last == "first":
        out[patch:patch + 4] = struct.pack(E + "I", ifds[0])
    return bytes(out)
