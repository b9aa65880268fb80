"""The GIF tests' model: a container walk, an LZW decoder and a composer written from the GIF89a text, and a Python statement of the optimiser's output rule
(DESIGN.md 8.3): rectangles, disposals, indices, the chunked LZW coder, the file -- byte for byte what the device route writes.
A canvas is [H][W] uint32, R | G << 8 | B << 16 | A << 24; 0 where nothing was painted."""
import struct

import numpy as np


class BadGif(Exception):
    pass


def _sub_blocks(d, i):
    out = bytearray()
    while True:
        if i >= len(d):
            raise BadGif("truncated sub-blocks")
        n = d[i]; i += 1
        if n == 0:
            return bytes(out), i
        if i + n > len(d):
            raise BadGif("truncated sub-block")
        out += d[i:i + n]; i += n


def parse(d):
    """-> dict(cw, ch, lsd, gct, loop, meta, frames, plain_text); a frame: x y w h interlace lct mcs data disposal delay transparent"""
    if len(d) < 13 or d[:6] not in (b"GIF87a", b"GIF89a"):
        raise BadGif("header")
    cw, ch = struct.unpack("<HH", d[6:10])
    g = dict(cw=cw, ch=ch, lsd=d[6:13], gct=b"", loop=b"", meta=[], frames=[], plain_text=False)
    i = 13
    if d[10] & 0x80:
        n = 3 << ((d[10] & 7) + 1)
        if i + n > len(d):
            raise BadGif("global table")
        g["gct"] = d[i:i + n]; i += n
    if not cw or not ch:
        raise BadGif("empty canvas")
    gce = dict(disposal=0, delay=0, transparent=None)
    while True:
        if i >= len(d):
            raise BadGif("no trailer")
        b = d[i]; i += 1
        if b == 0x3B:
            break
        if b == 0x21:
            if i >= len(d):
                raise BadGif("extension")
            start, label = i - 1, d[i]
            i += 1
            if label == 0xF9 and i + 5 <= len(d) and d[i] == 4:
                disposal = (d[i + 1] >> 2) & 7
                gce = dict(disposal=disposal if disposal <= 3 else 0, delay=d[i + 2] | (d[i + 3] << 8), transparent=d[i + 4] if d[i + 1] & 1 else None)
                _, i = _sub_blocks(d, i + 5)
                continue
            first = i
            _, i = _sub_blocks(d, i)
            if label == 0x01:
                g["plain_text"] = True
            elif label == 0xFF and d[first] == 11 and d[first + 1:first + 12] == b"NETSCAPE2.0":
                g["loop"] = g["loop"] or d[start:i]
            elif label in (0xFF, 0xFE):
                g["meta"].append(d[start:i])
            continue
        if b != 0x2C:
            raise BadGif("unknown block")
        if i + 9 > len(d):
            raise BadGif("image descriptor")
        x, y, w, h, packed = struct.unpack("<HHHHB", d[i:i + 9]); i += 9
        lct = b""
        if packed & 0x80:
            n = 3 << ((packed & 7) + 1)
            if i + n > len(d):
                raise BadGif("local table")
            lct = d[i:i + n]; i += n
        if i >= len(d):
            raise BadGif("image data")
        mcs = d[i]; i += 1
        data, i = _sub_blocks(d, i)
        if not w or not h or x + w > cw or y + h > ch:
            raise BadGif("rectangle")
        if not 2 <= mcs <= 8:
            raise BadGif("code size")
        if not lct and not g["gct"]:
            raise BadGif("no colour table")
        g["frames"].append(dict(x=x, y=y, w=w, h=h, interlace=bool(packed & 0x40), lct=lct, mcs=mcs, data=data, **gce))
        gce = dict(disposal=0, delay=0, transparent=None)
    if not g["frames"]:
        raise BadGif("no frame")
    return g


def lzw_decode(data, mcs, npx):
    """GIF89a appendix F: variable-width codes LSB first, clear and end codes, a table that stops growing at 4096 entries (deferred clear).
    -> npx indices; BadGif for a code beyond the next free entry or data that ends early; surplus data is ignored"""
    clear, end = 1 << mcs, (1 << mcs) + 1
    acc = nb = pos = 0
    out = []
    table = [[c] for c in range(clear)] + [None, None]
    width, prev = mcs + 1, None
    while len(out) < npx:
        while nb < width:
            if pos >= len(data):
                raise BadGif("data ends before the rectangle is full")
            acc |= data[pos] << nb; nb += 8; pos += 1
        code = acc & ((1 << width) - 1)
        acc >>= width; nb -= width
        if code == clear:
            table = table[:clear + 2]; width = mcs + 1; prev = None
            continue
        if code == end:
            raise BadGif("data ends before the rectangle is full")
        if prev is None:
            if code > end:
                raise BadGif("a code beyond the table")
            s = table[code]
        else:
            if code < len(table):
                s = table[code]
            elif code == len(table) and len(table) < 4096:
                s = prev + [prev[0]]
            else:
                raise BadGif("a code beyond the next free entry")
            if len(table) < 4096:
                table.append(prev + [s[0]])
                if len(table) == (1 << width) and width < 12:
                    width += 1
        out += s
        prev = s
    return out[:npx]


def deinterlace(rows):
    h = len(rows)
    order = list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))
    out = [None] * h
    for k, r in enumerate(order):
        out[r] = rows[k]
    return out


def frame_indices(f):
    """the frame's rectangle as [h][w] indices in row order"""
    a = np.array(lzw_decode(f["data"], f["mcs"], f["w"] * f["h"]), dtype=np.uint8).reshape(f["h"], f["w"])
    return np.array(deinterlace(list(a))) if f["interlace"] else a


def colour_table(g, f):
    """256 words: the frame's table (local, else global), opaque black behind its last entry"""
    raw = f["lct"] or g["gct"]
    t = np.full(256, 0xFF000000, dtype=np.uint32)
    for i in range(len(raw) // 3):
        t[i] = raw[3 * i] | (raw[3 * i + 1] << 8) | (raw[3 * i + 2] << 16) | 0xFF000000
    return t, len(raw) // 3


def compose(g):
    """every canvas of the file.  The canvas starts as 0; a pixel that is not the frame's transparent index is set to its colour, alpha 255; after the frame its
    rectangle is left (disposal 0 / 1), cleared to 0 -- not to the background colour: browsers do not use it -- (2) or put back (3)"""
    work = np.zeros((g["ch"], g["cw"]), dtype=np.uint32)
    canvases = []
    for f in g["frames"]:
        idx = frame_indices(f)
        table, _ = colour_table(g, f)
        cur = work.copy()
        view = cur[f["y"]:f["y"] + f["h"], f["x"]:f["x"] + f["w"]]
        mask = np.ones(idx.shape, dtype=bool) if f["transparent"] is None else idx != f["transparent"]
        view[mask] = table[idx][mask]
        canvases.append(cur)
        if f["disposal"] == 2:
            work = cur.copy()
            work[f["y"]:f["y"] + f["h"], f["x"]:f["x"] + f["w"]] = 0
        elif f["disposal"] != 3:
            work = cur
    return canvases


def canvases_rgba(blob):
    """[frames][H][W][4] uint8"""
    return np.stack([c.view(np.uint8).reshape(c.shape[0], c.shape[1], 4) for c in compose(parse(blob))])


# ------------------------------------------------------------------------------------------------ the output rule
def _bbox(mask):
    ys, xs = np.nonzero(mask)
    return None if not len(ys) else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def _unite(a, b):
    if a is None or b is None:
        return a or b
    return (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))


def rectangles(canvases):
    """-> ([R_k as x0 y0 x1 y1], [disp_out]).  Frame 0 is the whole canvas.  C_k: canvas k differs from canvas k - 1; U_k: canvas k - 1 opaque, canvas k not.
    disp_out[k - 1] = 2 if U_k is not empty, else 1; R_k = bbox(C_k + U_k+1), united with R_k-1 when that frame disposes; 1 x 1 at the origin when empty"""
    n = len(canvases)
    h, w = canvases[0].shape
    C = [None] + [_bbox(canvases[k] != canvases[k - 1]) for k in range(1, n)] + [None]
    U = [None] + [_bbox(((canvases[k - 1] >> 24) == 255) & ((canvases[k] >> 24) != 255)) for k in range(1, n)] + [None]
    disp = [2 if U[k + 1] is not None else 1 for k in range(n)]
    R = [(0, 0, w - 1, h - 1)]
    for k in range(1, n):
        r = _unite(C[k], U[k + 1])
        if disp[k - 1] == 2:
            r = _unite(r, R[k - 1])
        R.append(r or (0, 0, 0, 0))
    return R, disp


def encode_chunks(px, mcs, chunk):
    """the coder: the index stream cut into chunks of `chunk` pixels, each coded greedily from an empty table.  An entry is added behind every code while fewer
    than 4096 codes exist; the width grows when the next free code exceeds 2^width and stays at 12; a code sent with a full table is followed by a clear
    code.  The stream starts with a clear code; every chunk closes with the clear code the next one starts from, the last with the end code."""
    clear = 1 << mcs
    acc = nb = 0
    out = bytearray()

    def put(code, width):
        nonlocal acc, nb
        acc |= code << nb; nb += width
        while nb >= 8:
            out.append(acc & 255); acc >>= 8; nb -= 8

    put(clear, mcs + 1)
    nchunks = (len(px) + chunk - 1) // chunk
    for c in range(nchunks):
        part = px[c * chunk:(c + 1) * chunk]
        table, nxt, width = {}, clear + 2, mcs + 1
        cur = int(part[0])
        for b in list(part[1:]) + [None]:
            if b is not None and (cur, int(b)) in table:
                cur = table[(cur, int(b))]
                continue
            put(cur, width)
            if nxt < 4096:
                if b is not None:
                    table[(cur, int(b))] = nxt
                nxt += 1
                if nxt > (1 << width) and width < 12:
                    width += 1
            else:
                put(clear, width)
                table, nxt, width = {}, clear + 2, mcs + 1
            cur = None if b is None else int(b)
        put(clear + 1 if c == nchunks - 1 else clear, width)
    if nb:
        out.append(acc & 255)
    return bytes(out)


def _framed(data):
    out = bytearray()
    for i in range(0, len(data), 255):
        out.append(min(255, len(data) - i)); out += data[i:i + 255]
    return bytes(out) + b"\x00"


def optimise(blob, chunk, keep_metadata=False):
    """-> (the optimised file, None) or (None, "palette" / "hold" / "index") when the rule's fallback is raised; the caller applies the not-smaller rule"""
    g = parse(blob)
    for f in g["frames"]:
        # the output's code size follows the table's size alone; the extension may name any transparent index of 0..255, and one the output cannot code
        # leaves the file as it is
        if f["transparent"] is not None and f["transparent"] >= 1 << max(2, (len(f["lct"] or g["gct"]) // 3 - 1).bit_length()):
            return None, "index"
    canvases = compose(g)
    R, disp = rectangles(canvases)
    out = bytearray(b"GIF89a" + g["lsd"] + g["gct"] + g["loop"])
    if keep_metadata:
        for m in g["meta"]:
            out += m
    state = np.zeros_like(canvases[0])
    raised = None
    for k, f in enumerate(g["frames"]):
        table, n = colour_table(g, f)
        t = f["transparent"]
        lowest = {}
        for i in range(n - 1, -1, -1):
            if i != t:
                lowest[int(table[i])] = i
        if k > 0 and disp[k - 1] == 2:
            x0, y0, x1, y1 = R[k - 1]
            state[y0:y1 + 1, x0:x1 + 1] = 0
        x0, y0, x1, y1 = R[k]
        px = []
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                c, s = int(canvases[k][y, x]), int(state[y, x])
                if s == c and t is not None:
                    px.append(t)
                elif (c >> 24) != 255:
                    raised = raised or "hold"
                    px.append(0)
                else:
                    v = lowest.get(c)
                    if v is None:
                        raised = raised or ("hold" if s == c else "palette")
                        v = 0
                    state[y, x] = c
                    px.append(v)
        mcs = max(2, (n - 1).bit_length())
        out += bytes([0x21, 0xF9, 4, (disp[k] << 2) | (0 if t is None else 1)]) + struct.pack("<H", f["delay"]) + bytes([t or 0, 0])
        packed = (0x80 | ((len(f["lct"]) // 3).bit_length() - 2)) if f["lct"] else 0
        out += b"\x2C" + struct.pack("<HHHH", x0, y0, x1 - x0 + 1, y1 - y0 + 1) + bytes([packed]) + f["lct"] + bytes([mcs])
        out += _framed(encode_chunks(px, mcs, chunk))
    out += b"\x3B"
    return (None, raised) if raised else (bytes(out), None)
