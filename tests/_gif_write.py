"""A GIF muxer and LZW writer with every choice exposed, for the GIF tests: code size, where clear codes go (on a full table, never -- the deferred-clear
form --, every N codes, doubled, absent in front), interlace, local tables, disposal, transparent index, sub-block sizes, extension blocks."""
import struct


class BitWriter:
    def __init__(self):
        self.acc = 0
        self.nb = 0
        self.out = bytearray()

    def put(self, code, width):
        self.acc |= code << self.nb
        self.nb += width
        while self.nb >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.nb -= 8

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.nb else b"")


def lzw_encode(px, mcs, clears="full", lead_clear=True, double=False, end=True):
    """greedy LZW over the indices px.  clears: "full" = a clear code when the table is full; "never" = the table stays full and the width stays 12
    (deferred clear); an int N = a clear code after every N codes (and none for a full table).  double: every clear code twice."""
    clear = 1 << mcs
    bw = BitWriter()
    st = {"table": {}, "next": clear + 2, "width": mcs + 1}

    def put_clear():
        for _ in range(2 if double else 1):
            bw.put(clear, st["width"])
            st["table"] = {}; st["next"] = clear + 2; st["width"] = mcs + 1

    def grow():
        st["next"] += 1
        if st["next"] > (1 << st["width"]) and st["width"] < 12:
            st["width"] += 1

    if lead_clear:
        put_clear()
    cur = int(px[0])
    ncodes = 0
    for b in px[1:]:
        b = int(b)
        if (cur, b) in st["table"]:
            cur = st["table"][(cur, b)]
            continue
        bw.put(cur, st["width"])
        ncodes += 1
        if st["next"] < 4096:
            st["table"][(cur, b)] = st["next"]
            grow()
        elif clears == "full":
            put_clear()
        if isinstance(clears, int) and ncodes % clears == 0:
            put_clear()
        cur = b
    bw.put(cur, st["width"])
    if st["next"] < 4096:
        grow()
    if end:
        bw.put(clear + 1, st["width"])
    return bw.bytes()


def sub_blocks(data, size=255):
    out = bytearray()
    for i in range(0, len(data), size):
        part = data[i:i + size]
        out.append(len(part))
        out += part
    out.append(0)
    return bytes(out)


def table_bytes(colours):
    """(r, g, b) tuples -> the table padded with black to a power of two (2 entries at least)"""
    n = 2
    while n < len(colours):
        n *= 2
    flat = bytearray()
    for c in list(colours) + [(0, 0, 0)] * (n - len(colours)):
        flat += bytes(c)
    return bytes(flat), n.bit_length() - 2   # the descriptor's three size bits


def interlace_rows(rows):
    h = len(rows)
    order = list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))
    return [rows[r] for r in order]


def extension(label, blocks):
    """an extension block: label, then data sub-blocks as given (a list of byte strings, each one block), the terminator"""
    out = bytearray([0x21, label])
    for b in blocks:
        out.append(len(b))
        out += b
    out.append(0)
    return bytes(out)


def loop_extension(count=0):
    return extension(0xFF, [b"NETSCAPE2.0", b"\x01" + struct.pack("<H", count)])


def frame(indices, x=0, y=0, lct=None, interlace=False, disposal=None, transparent=None, delay=0, mcs=None, sub=255, surplus=b"", data=None, before=b"", **lzw):
    """indices: rows of colour indices.  disposal / transparent / delay: a graphic control extension is written when any is given (delay: non-zero).
    mcs: the LZW minimum code size (default: from the largest index, 2 at least).  surplus: bytes behind the LZW stream, inside the sub-blocks.
    data: the LZW stream itself, instead of coding the indices.  before: blocks in front of the frame's own.  Other keywords go to lzw_encode."""
    rows = [list(map(int, r)) for r in indices]
    return dict(rows=rows, x=x, y=y, lct=lct, interlace=interlace, disposal=disposal, transparent=transparent, delay=delay, mcs=mcs, sub=sub, surplus=surplus, data=data, before=before, lzw=lzw)


def frame_bytes(f):
    rows = f["rows"]
    h, w = len(rows), len(rows[0])
    out = bytearray(f["before"])
    if f["disposal"] is not None or f["transparent"] is not None or f["delay"]:
        packed = ((f["disposal"] or 0) << 2) | (1 if f["transparent"] is not None else 0)
        out += bytes([0x21, 0xF9, 4, packed]) + struct.pack("<H", f["delay"]) + bytes([f["transparent"] or 0, 0])
    packed = 0x40 if f["interlace"] else 0
    lct = b""
    if f["lct"] is not None:
        lct, bits = table_bytes(f["lct"])
        packed |= 0x80 | bits
    out += b"\x2C" + struct.pack("<HHHH", f["x"], f["y"], w, h) + bytes([packed]) + lct
    px = [v for r in (interlace_rows(rows) if f["interlace"] else rows) for v in r]
    mcs = f["mcs"] if f["mcs"] is not None else max(2, max(px).bit_length())
    data = f["data"] if f["data"] is not None else lzw_encode(px, mcs, **f["lzw"])
    out += bytes([mcs]) + sub_blocks(data + f["surplus"], f["sub"])
    return bytes(out)


def gif(cw, ch, frames, gct=None, background=0, loop=None, version=b"GIF89a", extensions=(), trailer=True):
    """the file: header, screen descriptor, global table, loop extension (loop: a count, None for no extension), further extension blocks, the frames, the trailer"""
    out = bytearray(version)
    table, bits = table_bytes(gct) if gct is not None else (b"", 0)
    out += struct.pack("<HH", cw, ch) + bytes([(0x80 | 0x70 | bits) if gct is not None else 0x70, background, 0]) + table
    if loop is not None:
        out += loop_extension(loop)
    for e in extensions:
        out += e
    for f in frames:
        out += frame_bytes(f)
    if trailer:
        out += b"\x3B"
    return bytes(out)
