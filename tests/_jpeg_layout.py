"""A small baseline JPEG writer for any component sampling layout (tests only).

Pillow/libjpeg-turbo writes 4:4:4, 4:2:2 and 4:2:0 only; the layout tests need 4:4:0, 4:1:1, 4:1:0, luma 3x1 / 1x4 and files whose Cb and Cr are
sampled differently.  This writer makes them from the seeded synthetic pictures of tools/gen_synth.py: JFIF YCbCr, each component point-sampled
to its own size (what the pixels are does not matter to a decoder test, only that they vary), an orthonormal float DCT, the Annex K quantisation
tables at a quality, and one fixed-length Huffman code per table class (every DC category 4 bits, every AC symbol 8 bits -- a valid DHT
that needs no statistics).  One interleaved sequential scan, with an optional restart interval -- or a list of scans (all components
interleaved, or one component each), every one with DRI segments of its own in front.  Progressive variants come from the oracle's
lossless transcode (oracle_lossless(src, progressive=1)), which keeps the layout.
"""
import numpy as np

from gen_synth import synth_rgb

# the layouts the tests use: name -> (h, v) of Y, Cb, Cr
LAYOUTS = {
    "440": ((1, 2), (1, 1), (1, 1)),
    "411": ((4, 1), (1, 1), (1, 1)),
    "410": ((4, 2), (1, 1), (1, 1)),
    "y31": ((3, 1), (1, 1), (1, 1)),
    "y14": ((1, 4), (1, 1), (1, 1)),
    "y22_cb11_cr22": ((2, 2), (1, 1), (2, 2)),
    "y21_cb12_cr11": ((2, 1), (1, 2), (1, 1)),
    "420": ((2, 2), (1, 1), (1, 1)),
}
# layouts libjpeg refuses: more than 10 blocks per MCU, and ratios that are not whole numbers
REFUSED = {
    "12_blocks": ((2, 2), (2, 2), (2, 2)),
    "11_blocks": ((4, 2), (2, 1), (1, 1)),
    "y31_cb21": ((3, 1), (2, 1), (1, 1)),
}

_ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# ITU T.81 Annex K.1, natural order
_QL = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
_QC = np.array([17, 18, 24, 47] + [99] * 4 + [18, 21, 26, 66] + [99] * 4 + [24, 26, 56] + [99] * 5 + [47, 66] + [99] * 38)
_AC_SYMS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]   # EOB, ZRL, run/size
_A = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def _qtable(base, quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * s + 50) // 100, 1, 255)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _category(v):
    return int(abs(int(v))).bit_length()


def _bits_of(v, size):
    return int(v) if v >= 0 else int(v) + (1 << size) - 1


def write_jpeg(rgb, layout, quality=85, restart_interval=0, scans=None):
    """(h, w, 3) uint8 RGB -> baseline JPEG bytes with the given ((h, v) x 3) sampling factors.
    scans: [(components, dri)] in file order; components (0, 1, 2) for an interleaved scan or (c,) for a scan of one component, whose
    restart interval counts the blocks of ceil(comp_w / 8) x ceil(comp_h / 8); dri None (no DRI segment: the interval in force stays),
    a value, or a tuple of values written as one DRI segment each in front of the SOS (0 switches restarts off)"""
    rgb = np.asarray(rgb, dtype=np.float64)
    H, W = rgb.shape[:2]
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    ycc = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128, 0.5 * r - 0.418688 * g - 0.081312 * b + 128]
    hmax, vmax = max(f[0] for f in layout), max(f[1] for f in layout)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    qt = [_qtable(_QL, quality), _qtable(_QC, quality)]
    comps = []
    for c, (h, v) in enumerate(layout):
        cw, ch = -(-W * h // hmax), -(-H * v // vmax)
        ys = np.minimum(np.arange(ch) * vmax // v, H - 1)
        xs = np.minimum(np.arange(cw) * hmax // h, W - 1)
        plane = np.clip(np.round(ycc[c][ys][:, xs]), 0, 255)
        bw, bh = mx * h, my * v
        plane = plane[np.minimum(np.arange(bh * 8), ch - 1)][:, np.minimum(np.arange(bw * 8), cw - 1)] - 128.0
        blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        coef = np.einsum("ux,abxy,vy->abuv", _A, blocks, _A).reshape(bh, bw, 64)
        q = np.round(coef / qt[min(c, 1)]).astype(np.int64)[:, :, _ZZ]
        q[:, :, 0] = np.clip(q[:, :, 0], -1023, 1023)
        q[:, :, 1:] = np.clip(q[:, :, 1:], -1023, 1023)
        comps.append((h, v, q, -(-cw // 8), -(-ch // 8)))

    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload

    out = bytearray(b"\xff\xd8")
    out += seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += seg(0xDB, bytes([t]) + bytes(int(x) for x in qt[t][_ZZ]))
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3])
    for c, (h, v) in enumerate(layout):
        sof += bytes([c + 1, (h << 4) | v, min(c, 1)])
    out += seg(0xC0, sof)
    for t in range(2):   # DC class: categories 0..11, 4 bits each; AC class: 162 symbols, 8 bits each
        out += seg(0xC4, bytes([t]) + bytes([0, 0, 0, 12] + [0] * 12) + bytes(range(12)))
        out += seg(0xC4, bytes([0x10 | t]) + bytes([0] * 7 + [len(_AC_SYMS)] + [0] * 8) + bytes(_AC_SYMS))
    ac_code = {s: i for i, s in enumerate(_AC_SYMS)}
    if scans is None:
        scans = [((0, 1, 2), restart_interval or None)]
    for group, dri in scans:
        assert len(group) == 1 or tuple(group) == (0, 1, 2), "an interleaved scan takes every component"
        for value in (() if dri is None else dri if isinstance(dri, tuple) else (dri,)):
            out += seg(0xDD, value.to_bytes(2, "big"))
            restart_interval = value
        out += seg(0xDA, bytes([len(group)]) + b"".join(bytes([c + 1, 0x11 if c else 0x00]) for c in group) + bytes([0, 63, 0]))
        bits = _Bits()
        pred = [0, 0, 0]

        def code_block(c, blk):
            d = int(blk[0]) - pred[c]
            pred[c] = int(blk[0])
            s = _category(d)
            bits.put(s, 4)
            if s:
                bits.put(_bits_of(d, s), s)
            run = 0
            nz = np.flatnonzero(blk[1:]) + 1
            last = 0
            for k in nz:
                run = k - last - 1
                while run > 15:
                    bits.put(ac_code[0xF0], 8)
                    run -= 16
                s = _category(blk[k])
                bits.put(ac_code[(run << 4) | s], 8)
                bits.put(_bits_of(blk[k], s), s)
                last = k
            if last != 63:
                bits.put(ac_code[0x00], 8)

        one = len(group) == 1
        across = comps[group[0]][3] if one else mx
        nunit, rst = across * (comps[group[0]][4] if one else my), 0
        for m in range(nunit):
            if restart_interval and m and m % restart_interval == 0:
                bits.flush()
                bits.out += bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) & 7
                pred = [0, 0, 0]
            mby, mbx = divmod(m, across)
            if one:
                code_block(group[0], comps[group[0]][2][mby, mbx])
                continue
            for c, (h, v, q, _, _) in enumerate(comps):
                for yy in range(v):
                    for xx in range(h):
                        code_block(c, q[mby * v + yy, mbx * h + xx])
        bits.flush()
        out += bits.out
    out += b"\xff\xd9"
    return bytes(out)


def layout_jpeg(seed, w, h, layout, quality=85, restart_interval=0):
    """a seeded synthetic picture (gen_synth.synth_rgb) in the layout, by name (LAYOUTS / REFUSED) or as ((h, v) x 3)"""
    if isinstance(layout, str):
        layout = LAYOUTS.get(layout) or REFUSED[layout]
    return write_jpeg(synth_rgb(seed, w, h, texture=6.0), layout, quality, restart_interval)
