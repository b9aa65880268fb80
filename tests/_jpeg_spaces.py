"""JPEG files in the colour spaces beside YCbCr and grey (tests only): Adobe CMYK and YCCK with four components, RGB with three.

Pillow / libjpeg-turbo writes CMYK files (Adobe transform 0, ids C M Y K) and, with keep_rgb, RGB files (ids R G B); it reads YCCK but does not
write it.  write_file() is a baseline writer from COEFFICIENTS: 1, 3 or 4 components with chosen ids, sampling factors, table slots and an optional
APP14 / JFIF segment, one interleaved scan, the fixed-length Huffman code of tests/_jpeg_layout.py.  The same planes can so be stored as a
CMYK / YCCK / RGB file and as grey or YCbCr files that hold identical coefficients -- which is how a component of such a file is compared with what
the oracle (which codes grey and YCbCr only) makes of it.
"""
import functools
import io

import numpy as np

from _jpeg_layout import _A, _AC_SYMS, _QC, _QL, _ZZ, _Bits, _bits_of, _category, _qtable
from _jpeg_markers import seg, walk
from gen_synth import synth_rgb

CMYK, CMYK_PLAIN, RGB, YCCK = "cmyk", "cmyk without APP14", "rgb", "ycck"


def adobe(transform):
    return seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform]))


JFIF = seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")


def plane_coefs(plane, bw, bh, qt):
    """(h, w) samples -> (bh, bw, 64) quantised coefficients in zig-zag order: the plane's edges replicated to the block grid, an orthonormal float DCT, `qt` (natural order)"""
    plane = np.asarray(plane, dtype=np.float64)
    ch, cw = plane.shape
    plane = plane[np.minimum(np.arange(bh * 8), ch - 1)][:, np.minimum(np.arange(bw * 8), cw - 1)] - 128.0
    blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    coef = np.einsum("ux,abxy,vy->abuv", _A, blocks, _A).reshape(bh, bw, 64)
    return np.clip(np.round(coef / qt).astype(np.int64)[:, :, _ZZ], -1023, 1023)


def write_file(width, height, comps, qtables, segments=(), restart_interval=0):
    """comps: [dict(id, h, v, tq, coef)] with coef (bh, bw, 64) zig-zag over the MCU-padded block grid (or larger); qtables: {slot: 64 values, natural order};
    segments: marker segments that go behind SOI (JFIF, adobe(t)).  One interleaved baseline scan, every component on Huffman tables 0."""
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    out = bytearray(b"\xff\xd8")
    for s in segments:
        out += s
    for slot, qt in sorted(qtables.items()):
        out += seg(0xDB, bytes([slot]) + bytes(int(x) for x in np.asarray(qt)[_ZZ]))
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([len(comps)])
    for c in comps:
        sof += bytes([c["id"], (c["h"] << 4) | c["v"], c["tq"]])
    out += seg(0xC0, sof)
    out += seg(0xC4, bytes([0x00]) + bytes([0, 0, 0, 12] + [0] * 12) + bytes(range(12)))                      # DC: categories 0..11, 4 bits each
    out += seg(0xC4, bytes([0x10]) + bytes([0] * 7 + [len(_AC_SYMS)] + [0] * 8) + bytes(_AC_SYMS))             # AC: 162 symbols, 8 bits each
    if restart_interval:
        out += seg(0xDD, restart_interval.to_bytes(2, "big"))
    out += seg(0xDA, bytes([len(comps)]) + b"".join(bytes([c["id"], 0x00]) for c in comps) + bytes([0, 63, 0]))
    ac_code = {s: i for i, s in enumerate(_AC_SYMS)}
    bits, pred, rst = _Bits(), [0] * len(comps), 0

    def code_block(ci, blk):
        d = int(blk[0]) - pred[ci]
        pred[ci] = int(blk[0])
        s = _category(d)
        bits.put(s, 4)
        if s:
            bits.put(_bits_of(d, s), s)
        last = 0
        for k in np.flatnonzero(blk[1:]) + 1:
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

    for m in range(mx * my):
        if restart_interval and m and m % restart_interval == 0:
            bits.flush()
            bits.out += bytes([0xFF, 0xD0 + rst])
            rst = (rst + 1) & 7
            pred = [0] * len(comps)
        mby, mbx = divmod(m, mx)
        for ci, c in enumerate(comps):
            for yy in range(c["v"]):
                for xx in range(c["h"]):
                    code_block(ci, c["coef"][mby * c["v"] + yy, mbx * c["h"] + xx])
    bits.flush()
    return bytes(out + bits.out + b"\xff\xd9")


def frame(data):
    """-> dict(sof marker, width, height, comps [(id, h, v, tq)], adobe (transform or None), jfif (bool), sof (offset of the SOF marker))"""
    f = dict(adobe=None, jfif=False)
    for m, a, b in walk(data):
        if m in (0xC0, 0xC1, 0xC2):
            n = data[a + 9]
            f.update(marker=m, sof=a, height=int.from_bytes(data[a + 5:a + 7], "big"), width=int.from_bytes(data[a + 7:a + 9], "big"),
                     comps=[(data[a + 10 + 3 * c], data[a + 11 + 3 * c] >> 4, data[a + 11 + 3 * c] & 15, data[a + 12 + 3 * c]) for c in range(n)])
        elif m == 0xEE and data[a + 4:a + 9] == b"Adobe":
            assert f["adobe"] is None, "two Adobe segments"
            f["adobe"] = data[a + 15]
        elif m == 0xE0 and data[a + 4:a + 9] == b"JFIF\0":
            f["jfif"] = True
    return f


def general_script(n):
    """libjpeg's all-purpose progression (jcparam.c jpeg_simple_progression) for n components: 2 + 4 n scans"""
    every = tuple(range(n))
    each = lambda ss, se, ah, al: [((c,), ss, se, ah, al) for c in range(n)]
    return [(every, 0, 0, 0, 1)] + each(1, 5, 0, 2) + each(6, 63, 0, 2) + each(1, 63, 2, 1) + [(every, 0, 0, 1, 0)] + each(1, 63, 1, 0)


def without_app14(data):
    for m, a, b in walk(data):
        if m == 0xEE:
            return data[:a] + data[b:]
    raise AssertionError("no APP14")


def _four_planes(seed, w, h):
    rgb = synth_rgb(seed, w, h, texture=6.0)
    k = synth_rgb(seed + 100, w, h, texture=3.0)[:, :, 1]
    return np.dstack([rgb, 255 - k // 2])


def pillow_cmyk(seed, w, h, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(_four_planes(seed, w, h), "CMYK").save(b, "JPEG", quality=88, **kw)
    return b.getvalue()


def pillow_rgb(seed, w, h, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(synth_rgb(seed, w, h, texture=6.0), "RGB").save(b, "JPEG", quality=88, keep_rgb=True, **kw)
    return b.getvalue()


def ycck_comps(seed, w, h, layout, quality=88):
    """the four components of a YCCK picture (Y, Cb, Cr of a synthetic picture, K of another; each point-sampled to its own size) as write_file wants them"""
    px = _four_planes(seed, w, h).astype(np.float64)
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    full = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128, 0.5 * r - 0.418688 * g - 0.081312 * b + 128, px[..., 3]]
    hmax, vmax = max(f[0] for f in layout), max(f[1] for f in layout)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    qts = {0: _qtable(_QL, quality), 1: _qtable(_QC, quality)}
    comps = []
    for c, (ch_, cv_) in enumerate(layout):
        cw, ch = -(-w * ch_ // hmax), -(-h * cv_ // vmax)
        ys, xs = np.minimum(np.arange(ch) * vmax // cv_, h - 1), np.minimum(np.arange(cw) * hmax // ch_, w - 1)
        tq = 1 if c in (1, 2) else 0
        comps.append(dict(id=c + 1, h=ch_, v=cv_, tq=tq, coef=plane_coefs(np.clip(np.round(full[c][ys][:, xs]), 0, 255), mx * ch_, my * cv_, qts[tq])))
    return comps, qts


def ycck_file(seed, w, h, layout, restart_interval=0):
    comps, qts = ycck_comps(seed, w, h, layout)
    return write_file(w, h, comps, qts, [adobe(2)], restart_interval)


L111 = ((1, 1),) * 4
L2112 = ((2, 2), (1, 1), (1, 1), (2, 2))


@functools.lru_cache(maxsize=None)
def sources():
    """-> [(name, file bytes, kind)]: every kind of source at every size the issue names (8x8, 17x9, 97x61 with partial 16x16 MCUs, 200x150 with 475 blocks a component)"""
    cases = [
        ("cmyk_base_97x61", pillow_cmyk(1, 97, 61), CMYK),
        ("cmyk_prog_200x150", pillow_cmyk(2, 200, 150, progressive=True, optimize=True), CMYK),
        ("cmyk_prog_8x8", pillow_cmyk(3, 8, 8, progressive=True, optimize=True), CMYK),
        ("cmyk_base_dri5_97x61", pillow_cmyk(4, 97, 61, restart_marker_blocks=5), CMYK),
        ("cmyk_plain_17x9", without_app14(pillow_cmyk(5, 17, 9)), CMYK_PLAIN),
        ("rgb_base_17x9", pillow_rgb(6, 17, 9), RGB),
        ("rgb_prog_97x61", pillow_rgb(7, 97, 61, progressive=True, optimize=True), RGB),
        ("rgb_base_200x150", pillow_rgb(8, 200, 150), RGB),
        ("ycck_111_97x61", ycck_file(9, 97, 61, L111), YCCK),
        ("ycck_2112_200x150", ycck_file(10, 200, 150, L2112), YCCK),
        ("ycck_2112_17x9", ycck_file(11, 17, 9, L2112), YCCK),
        ("ycck_2112_dri3_97x61", ycck_file(12, 97, 61, L2112, restart_interval=3), YCCK),
    ]
    for name, data, kind in cases:   # each file is what its name says
        f = frame(data)
        assert len(f["comps"]) == (3 if kind == RGB else 4), name
        assert f["adobe"] == {CMYK: 0, CMYK_PLAIN: None, RGB: f["adobe"], YCCK: 2}[kind] and not f["jfif"], (name, f)
        if kind == RGB:
            assert bytes(c[0] for c in f["comps"]) == b"RGB", name
        if kind in (CMYK, CMYK_PLAIN):
            assert bytes(c[0] for c in f["comps"]) == b"CMYK", name
        assert ("prog" in name) == (f["marker"] == 0xC2), name
        assert ("dri" in name) == any(m == 0xDD for m, _, _ in walk(data)), name
    return cases


def grey_of(data, c):
    """a grey JFIF file (baseline, this module's writer) holding the coefficients of component c of `data` at the component's own size"""
    from oracle import oracle as O
    img = O.decode(data)
    k = img.im.comp[c]
    coef = img.coefs(c)[:, :, _ZZ].astype(np.int64)
    return write_file(k.comp_w, k.comp_h, [dict(id=1, h=1, v=1, tq=0, coef=coef)], {0: img_table(img, c)}, [JFIF])


def ycc_of(data):
    """a YCbCr JFIF file holding the coefficients of components 0..2 of a four-component file at their sampling factors.  (The fourth component must
    not carry the largest factors alone: the first three then keep their sizes.)"""
    from oracle import oracle as O
    img = O.decode(data)
    im = img.im
    assert max(im.comp[c].h for c in range(3)) == im.hmax and max(im.comp[c].v for c in range(3)) == im.vmax
    comps = [dict(id=c + 1, h=im.comp[c].h, v=im.comp[c].v, tq=min(c, 1), coef=img.coefs(c)[:, :, _ZZ].astype(np.int64)) for c in range(3)]
    return write_file(im.width, im.height, comps, {0: img_table(img, 0), 1: img_table(img, 1)}, [JFIF])


def img_table(img, c):
    """the quantisation table component c of an oracle decode was coded with, natural order"""
    return np.array(img.im.qt[img.im.comp[c].tq], dtype=np.int64)


def real_blocks(img, c):
    k = img.im.comp[c]
    return img.coefs(c)[:k.real_bh, :k.real_bw]
