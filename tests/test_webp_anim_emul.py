"""Animated WebP inputs: the container, the canvas reconstruction (blend and dispose) and the change search between canvases, here through the
emulation build.  The judge is libwebp's AnimDecoder through Pillow: every canvas the device composes must equal Pillow's seek(k) sample for
sample; what is written again must decode (in Pillow) to the same canvases (lossless) or carry exactly the rectangles, flags, timing and coded
bytes the fixed output rule predicts from Pillow's canvases.  Inputs are Pillow's own save_all animations and files muxed by hand from Pillow
still frames with every offset and flag chosen here."""
import functools
import io
import json
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

from _util import ROOT, emul_api, package

CS_ERR_UNSUPPORTED, CS_ERR_BAD_WEBP = 10201, 40100
EMUL_CLI = os.path.join(ROOT, "tests", "emul", "caesiumclt_emul")


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


# ------------------------------------------------------------------------------------------------ RIFF
def chunks(blob, start=12, end=None):
    """[(fourcc, payload, offset of the payload)] of a chunk list"""
    out = []
    end = len(blob) if end is None else end
    i = start
    while i + 8 <= end:
        n = struct.unpack_from("<I", blob, i + 4)[0]
        out.append((blob[i:i + 4], blob[i + 8:i + 8 + n], i + 8))
        i += 8 + n + (n & 1)
    return out


def u24(b, i):
    return b[i] | (b[i + 1] << 8) | (b[i + 2] << 16)


def p24(v):
    return bytes((v & 255, (v >> 8) & 255, (v >> 16) & 255))


def chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def anim_layout(blob):
    """what the container says: canvas, VP8X flags, background, loops, and per ANMF its rectangle, duration, flag bits and sub-chunks"""
    top = chunks(blob)
    vp8x = [p for f, p, _ in top if f == b"VP8X"][0]
    anim = [p for f, p, _ in top if f == b"ANIM"][0]
    frames = []
    for f, p, _ in top:
        if f == b"ANMF":
            frames.append(dict(x=2 * u24(p, 0), y=2 * u24(p, 3), w=u24(p, 6) + 1, h=u24(p, 9) + 1, duration=u24(p, 12), no_blend=bool(p[15] & 2), dispose=bool(p[15] & 1),
                               sub={sf: sp for sf, sp, _ in chunks(p, 16)}))
    return dict(w=u24(vp8x, 4) + 1, h=u24(vp8x, 7) + 1, flags=vp8x[0], background=anim[:4], loops=anim[4] | (anim[5] << 8), frames=frames, order=[f for f, _, _ in top])


def still_chunks(arr, lossy=False):
    """a Pillow still of an RGBA array, as the chunks an ANMF takes: VP8L (lossless, exact) or ALPH + VP8"""
    b = io.BytesIO()
    if lossy:
        Image.fromarray(arr, "RGBA").save(b, format="WEBP", quality=75, method=4, exact=True)
    else:
        Image.fromarray(arr, "RGBA").save(b, format="WEBP", lossless=True, exact=True)
    return b"".join(chunk(f, p) for f, p, _ in chunks(b.getvalue()) if f in (b"ALPH", b"VP8 ", b"VP8L"))


def mux(cw, ch, frames, background=b"\x10\x20\x30\x40", loops=0, extra_front=b"", extra_back=b"", flags=0):
    """frames: dicts of arr ([h][w][4]), x, y (even), duration, blend, dispose, lossy, junk (an unknown chunk behind the bitstream: libwebp takes none in front of it)"""
    body = chunk(b"VP8X", bytes([0x12 | flags, 0, 0, 0]) + p24(cw - 1) + p24(ch - 1)) + extra_front + chunk(b"ANIM", background + struct.pack("<H", loops))
    for f in frames:
        h, w = f["arr"].shape[:2]
        head = p24(f["x"] // 2) + p24(f["y"] // 2) + p24(w - 1) + p24(h - 1) + p24(f.get("duration", 100)) + bytes([(0 if f.get("blend", True) else 2) | (1 if f.get("dispose") else 0)])
        body += chunk(b"ANMF", head + still_chunks(f["arr"], f.get("lossy", False)) + (chunk(b"JUNK", b"abc") if f.get("junk") else b""))
    body += extra_back
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body


def rgba(rng, w, h, alpha="mixed"):
    """random colours; alpha: 'opaque', or 'mixed' = blocks of 0, of 255 and of everything in between"""
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha == "opaque":
        a[..., 3] = 255
    else:
        pick = rng.integers(0, 3, (h, w))
        a[..., 3] = np.where(pick == 0, 0, np.where(pick == 1, 255, a[..., 3]))
    return a


def hand_muxed():
    rng = np.random.default_rng(2024)
    out = {}
    # blend over a partly transparent canvas, source alpha 0 / 255 / in between; a 1 x 1 frame in the bottom right corner of an odd canvas; a frame that
    # touches the right and the bottom edge
    out["blend"] = mux(33, 21, [dict(arr=rgba(rng, 33, 21), x=0, y=0, duration=30), dict(arr=rgba(rng, 20, 10), x=4, y=2, duration=40, junk=True),
                                dict(arr=rgba(rng, 1, 1), x=32, y=20, duration=50), dict(arr=rgba(rng, 13, 9), x=20, y=12, duration=60),
                                dict(arr=rgba(rng, 7, 5, "opaque"), x=2, y=6, duration=70)], loops=7)
    # dispose to background, then a blended frame across the cleared rectangle's edge; a frame that changes nothing (all of it transparent)
    out["dispose"] = mux(40, 30, [dict(arr=rgba(rng, 40, 30, "opaque"), x=0, y=0), dict(arr=rgba(rng, 16, 12), x=6, y=4, dispose=True, duration=0),
                                  dict(arr=rgba(rng, 20, 14), x=10, y=8), dict(arr=np.zeros((8, 8, 4), np.uint8), x=0, y=0, duration=0xFFFFFF),
                                  dict(arr=rgba(rng, 9, 9), x=30, y=20, blend=False, dispose=True), dict(arr=rgba(rng, 12, 10), x=26, y=18)])
    # a small first frame that disposes: the frame behind it is a key frame too, and so is the one behind that if it disposes as well
    out["inherit"] = mux(30, 20, [dict(arr=rgba(rng, 10, 8), x=4, y=4, dispose=True), dict(arr=rgba(rng, 20, 12), x=2, y=2, dispose=True),
                                  dict(arr=rgba(rng, 14, 10), x=8, y=6), dict(arr=rgba(rng, 6, 6), x=0, y=0)])
    # whole-canvas frames in mid-sequence: one that does not blend (a key frame), one that does (not one)
    out["full"] = mux(24, 18, [dict(arr=rgba(rng, 24, 18), x=0, y=0), dict(arr=rgba(rng, 8, 8), x=6, y=4), dict(arr=rgba(rng, 24, 18), x=0, y=0, blend=False),
                               dict(arr=rgba(rng, 24, 18), x=0, y=0), dict(arr=rgba(rng, 24, 18, "opaque"), x=0, y=0, dispose=True), dict(arr=rgba(rng, 5, 7), x=18, y=10)])
    out["single"] = mux(17, 13, [dict(arr=rgba(rng, 9, 7), x=2, y=2, duration=123)], loops=1)
    out["1x1"] = mux(1, 1, [dict(arr=rgba(rng, 1, 1), x=0, y=0), dict(arr=rgba(rng, 1, 1, "opaque"), x=0, y=0), dict(arr=rgba(rng, 1, 1), x=0, y=0, blend=False)])
    # opaque content that changes in a corner: the blend form of the lossless output
    base = rgba(rng, 51, 37, "opaque")
    moving = [dict(arr=base, x=0, y=0)]
    for k in range(4):
        patch = rgba(rng, 6, 6, "opaque")
        x, y = 8 + 4 * k, 10 + 2 * (k & 1)
        patch[2:4, 2:4] = base[y + 2:y + 4, x + 2:x + 4]   # part of it equal to what is under it
        moving.append(dict(arr=patch, x=x, y=y, duration=20 + k))
    out["opaque"] = mux(51, 37, moving)
    # more frames than a wave has lanes
    many = [dict(arr=rgba(rng, 16, 16), x=0, y=0, duration=1)]
    for k in range(69):
        w, h = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        many.append(dict(arr=rgba(rng, w, h, "opaque" if k % 3 == 0 else "mixed"), x=2 * int(rng.integers(0, (16 - w) // 2 + 1)), y=2 * int(rng.integers(0, (16 - h) // 2 + 1)), duration=k,
                         blend=bool(rng.integers(0, 2)), dispose=bool(rng.integers(0, 4) == 0)))
    out["many"] = mux(16, 16, many)
    # lossy frames with an ALPH chunk, and one without
    out["alph"] = mux(48, 32, [dict(arr=rgba(rng, 48, 32), x=0, y=0, lossy=True), dict(arr=rgba(rng, 20, 16), x=10, y=8, lossy=True, dispose=True),
                               dict(arr=rgba(rng, 30, 20, "opaque"), x=4, y=4, lossy=True), dict(arr=rgba(rng, 17, 11), x=30, y=20)])
    return out


def pillow_made():
    rng = np.random.default_rng(99)
    out = {}

    def frames(w, h, n, alpha):
        base = rgba(rng, w, h, "opaque")
        yy, xx = np.mgrid[0:h, 0:w]
        base[..., 0] = (xx * 3 + yy) & 255; base[..., 1] = (yy * 5) & 255   # smooth enough for the lossy coder, with some noise in blue
        fr = []
        for k in range(n):
            a = base.copy()
            a[4 + 3 * k:14 + 3 * k, 6 + 5 * k:22 + 5 * k, :3] = rng.integers(0, 256, 3, dtype=np.uint8)
            if alpha:
                a[..., 3] = np.clip(xx * 6 + k * 10, 0, 255).astype(np.uint8)
                a[:5, :5, 3] = 0
            fr.append(Image.fromarray(a, "RGBA" ) if alpha else Image.fromarray(a[..., :3].copy(), "RGB"))
        return fr

    def save(fr, **kw):
        b = io.BytesIO()
        fr[0].save(b, format="WEBP", save_all=True, append_images=fr[1:], duration=[30 + 7 * k for k in range(len(fr))], loop=kw.pop("loop", 0), **kw)
        return b.getvalue()
    out["p_lossless"] = save(frames(64, 48, 5, False), lossless=True, loop=2)
    out["p_lossless_alpha"] = save(frames(61, 45, 4, True), lossless=True, background=(1, 2, 3, 4))
    out["p_lossy"] = save(frames(64, 48, 5, False), quality=70)
    out["p_lossy_alpha"] = save(frames(70, 50, 4, True), quality=50, method=2)
    out["p_mixed"] = save(frames(64, 48, 6, True), allow_mixed=True, quality=60)
    out["p_minimize"] = save(frames(57, 33, 6, False), lossless=True, minimize_size=True)
    out["p_kminmax"] = save(frames(64, 48, 8, True), quality=80, kmin=2, kmax=3)
    return out


@functools.lru_cache(maxsize=None)
def inputs():
    d = hand_muxed()
    d.update(pillow_made())
    return d


@functools.lru_cache(maxsize=None)
def judged(name):
    """Pillow's canvases of an input: [frames][h][w][4]"""
    return pillow_canvases(inputs()[name])


def pillow_canvases(blob):
    im = Image.open(io.BytesIO(blob))
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append(np.asarray(im.convert("RGBA")).copy())
    return np.stack(out)


def predicted(canv, lossless):
    """section 3 of the output rule, from the judge's canvases: per frame (x, y, w, h, no_blend, pixels of the rectangle as they are coded)"""
    out = []
    for k in range(len(canv)):
        cur = canv[k]
        if k == 0:
            out.append((0, 0, cur.shape[1], cur.shape[0], True, cur))
            continue
        changed = (cur != canv[k - 1]).any(axis=2)
        if not changed.any():
            x = y = 0; w = h = 1
        else:
            ys, xs = np.nonzero(changed)
            x, y = int(xs.min()) & ~1, int(ys.min()) & ~1
            w, h = int(xs.max()) + 1 - x, int(ys.max()) + 1 - y
        rect, ch = cur[y:y + h, x:x + w], changed[y:y + h, x:x + w]
        holes = lossless and bool((rect[ch][:, 3] == 255).all()) and not ch.all()
        if holes:
            rect = np.where(ch[..., None], rect, 0).astype(np.uint8)
        out.append((x, y, w, h, not holes, rect))
    return out


def check_structure(name, out, lossless):
    src, got = anim_layout(inputs()[name]), anim_layout(out)
    canv = judged(name)
    want = predicted(canv, lossless)
    assert (got["w"], got["h"], got["loops"], got["background"]) == (src["w"], src["h"], src["loops"], src["background"]), name
    assert [f["duration"] for f in got["frames"]] == [f["duration"] for f in src["frames"]], name
    assert len(got["frames"]) == len(canv)
    assert got["order"] == [b"VP8X", b"ANIM"] + [b"ANMF"] * len(canv), name
    carries = False
    for k, (f, (x, y, w, h, no_blend, rect)) in enumerate(zip(got["frames"], want)):
        assert (f["x"], f["y"], f["w"], f["h"], f["no_blend"], f["dispose"]) == (x, y, w, h, no_blend, False), (name, k)
        assert set(f["sub"]) == ({b"VP8L"} if lossless else ({b"ALPH", b"VP8 "} if (rect[..., 3] < 255).any() else {b"VP8 "})), (name, k)
        carries |= bool((rect[..., 3] < 255).any())
    assert got["flags"] == (0x02 | (0x10 if carries else 0)), name
    return want


# ------------------------------------------------------------------------------------------------ the tests
def test_emul_canvases_equal_libwebp(api):
    names = list(inputs())
    for name, got in zip(names, api.webp_anim_canvases([inputs()[n] for n in names])):
        assert not isinstance(got, Exception), (name, got)
        want = judged(name)
        assert got.shape == want.shape, name
        for k in range(len(want)):
            assert np.array_equal(got[k], want[k]), (name, k)


def test_emul_lossless_run_keeps_canvases_and_follows_the_rule(api):
    names = list(inputs())
    outs = api.cs_batch_compress([inputs()[n] for n in names], params(webp_lossless=True))
    for name, out in zip(names, outs):
        assert not isinstance(out, Exception), (name, out)
        check_structure(name, out, True)
        assert np.array_equal(pillow_canvases(out), judged(name)), name
    # the device decoder reads its own muxer's files: the same canvases again
    for name, got in zip(names, api.webp_anim_canvases(outs)):
        assert np.array_equal(got, judged(name)), name


@pytest.mark.parametrize("quality", [35, 85])
def test_emul_lossy_run_follows_the_rule_and_codes_like_the_still_path(api, quality):
    names = list(inputs())
    p = params(webp_quality=quality)
    outs = api.cs_batch_compress([inputs()[n] for n in names], p)
    stills, where = [], []
    for name, out in zip(names, outs):
        assert not isinstance(out, Exception), (name, out)
        want = check_structure(name, out, False)
        assert np.array_equal(pillow_canvases(out)[..., 3], judged(name)[..., 3]), name   # the alpha plane is coded losslessly
        for k, (x, y, w, h, _, rect) in enumerate(want):   # the rectangle as a still picture of its own, through the path still pictures take
            b = io.BytesIO()
            Image.fromarray(rect, "RGBA").save(b, format="WEBP", lossless=True, exact=True)
            stills.append(b.getvalue()); where.append((name, k, anim_layout(out)["frames"][k]["sub"]))
    for (name, k, sub), still in zip(where, api.cs_batch_compress(stills, p)):
        assert not isinstance(still, Exception), (name, k, still)
        assert {f: pl for f, pl, _ in chunks(still) if f in (b"ALPH", b"VP8 ")} == sub, (name, k)


def damaged():
    good = inputs()["p_lossy"]
    lay = [(f, p, o) for f, p, o in chunks(good) if f == b"ANMF"]
    cut = good[:lay[-1][2] + len(lay[-1][1]) // 2]                               # the last ANMF ends with the file, in the middle of its bitstream
    outside = bytearray(inputs()["blend"]); o = [o for f, _, o in chunks(bytes(outside)) if f == b"ANMF"][1]
    outside[o:o + 3] = p24(8)                                                     # x = 16, width 20 on a canvas of 33
    broken = bytearray(good); o = lay[1][2] + 16
    sub = [(f, so) for f, _, so in chunks(bytes(broken), o, lay[1][2] + len(lay[1][1])) if f == b"VP8 "][0][1]
    broken[sub] |= 0xE0; broken[sub + 1] = broken[sub + 2] = 0xFF                 # a first partition longer than the frame: the size bytes behind it stay as they are
    return [cut, bytes(outside), bytes(broken)]


def test_emul_damaged_animations_fail_alone(api):
    still_a, still_b = io.BytesIO(), io.BytesIO()
    rng = np.random.default_rng(3)
    Image.fromarray(rgba(rng, 40, 30, "opaque")[..., :3].copy(), "RGB").save(still_a, format="WEBP", quality=80)
    Image.fromarray(rgba(rng, 21, 17), "RGBA").save(still_b, format="WEBP", lossless=True, exact=True)
    bad = damaged()
    batch = [still_a.getvalue(), inputs()["dispose"], bad[0], inputs()["alph"], bad[1], still_b.getvalue(), bad[2], inputs()["p_mixed"]]
    for p in (params(webp_quality=70), params(webp_lossless=True)):
        outs = api.cs_batch_compress(batch, p)
        for i, (blob, out) in enumerate(zip(batch, outs)):
            if i in (2, 4, 6):
                assert isinstance(out, Exception) and out.code == CS_ERR_BAD_WEBP, (i, out)
            else:
                assert not isinstance(out, Exception), (i, out)
                assert out == api.cs_batch_compress([blob], p)[0], i
    for out in api.webp_anim_canvases(bad):
        assert isinstance(out, Exception) and out.code == CS_ERR_BAD_WEBP
    # an animation whose frames alone exceed what one device batch may reserve (twenty ANMF headers of 16384 x 16384 each): refused alone, before anything is reserved
    huge = b"".join(chunk(b"ANMF", p24(0) + p24(0) + p24(16383) + p24(16383) + p24(10) + b"\0" + chunk(b"VP8L", b"\x2f")) for _ in range(20))
    body = chunk(b"VP8X", bytes([0x12, 0, 0, 0]) + p24(16383) + p24(16383)) + chunk(b"ANIM", bytes(6)) + huge
    outs = api.cs_batch_compress([inputs()["single"], b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body, still_a.getvalue()], params(webp_quality=70))
    assert isinstance(outs[1], Exception) and outs[1].code == CS_ERR_UNSUPPORTED and "animated" in str(outs[1]), outs[1]
    assert outs[0] == api.cs_batch_compress([inputs()["single"]], params(webp_quality=70))[0] and not isinstance(outs[2], Exception)
    # what stays refused says so
    for kw in (dict(width=20), dict(height=10), dict(width=20, height=10)):
        out = api.cs_batch_compress([inputs()["blend"], still_a.getvalue()], params(webp_quality=70, **kw))
        assert isinstance(out[0], Exception) and out[0].code == CS_ERR_UNSUPPORTED and "animated" in str(out[0]) and not isinstance(out[1], Exception)
    for fmt in (0, 1):
        out = api.batch_convert([inputs()["blend"], still_a.getvalue()], params(), fmt)
        assert isinstance(out[0], Exception) and out[0].code == CS_ERR_UNSUPPORTED and "animated" in str(out[0]) and not isinstance(out[1], Exception)


def test_emul_metadata_is_carried_under_keep_metadata(api):
    icc, exif, xmp = b"profile-bytes-odd", b"Exif\0\0II*\0\x08\0\0\0\0\0", b"<x:xmpmeta/>"
    rng = np.random.default_rng(8)
    fr = [dict(arr=rgba(rng, 20, 14), x=0, y=0), dict(arr=rgba(rng, 6, 4), x=4, y=2)]
    src = mux(20, 14, fr, extra_front=chunk(b"ICCP", icc), extra_back=chunk(b"EXIF", exif) + chunk(b"XMP ", xmp), flags=0x2C)
    want = pillow_canvases(src)
    for lossless in (False, True):
        kept, dropped = api.cs_batch_compress([src], params(webp_lossless=lossless, keep_metadata=True))[0], api.cs_batch_compress([src], params(webp_lossless=lossless))[0]
        lay = anim_layout(kept)
        assert lay["order"] == [b"VP8X", b"ICCP", b"ANIM", b"ANMF", b"ANMF", b"EXIF"] and lay["flags"] == 0x02 | 0x10 | 0x20 | 0x08
        got = dict((f, p) for f, p, _ in chunks(kept))
        assert got[b"ICCP"] == icc and got[b"EXIF"] == exif
        assert anim_layout(dropped)["order"] == [b"VP8X", b"ANIM", b"ANMF", b"ANMF"] and anim_layout(dropped)["flags"] == 0x02 | 0x10
        assert struct.unpack_from("<I", kept, 4)[0] == len(kept) - 8
        if lossless:
            assert np.array_equal(pillow_canvases(kept), want)


def test_emul_compress_to_size_on_an_animation(api):
    name = "p_lossy_alpha"
    full = api.cs_batch_compress([inputs()[name]], params(webp_quality=80))[0]
    small = api.cs_batch_compress([inputs()[name]], params(webp_quality=1))[0]
    target = (len(full) + len(small)) // 2
    out = api.batch_compress_to_size([inputs()[name], inputs()["single"]], params(), target)
    assert not isinstance(out[0], Exception), out[0]
    assert len(small) <= len(out[0]) <= target
    check_structure(name, out[0], False)
    assert not isinstance(out[1], Exception) and len(out[1]) <= target


def test_emul_lossless_run_with_the_far_coder(api, monkeypatch):
    names = ["opaque", "p_lossless_alpha", "many"]
    plain = api.cs_batch_compress([inputs()[n] for n in names], params(webp_lossless=True))
    monkeypatch.setenv("CSH_VP8L", "far")
    outs = api.cs_batch_compress([inputs()[n] for n in names], params(webp_lossless=True))
    for name, out, ref in zip(names, outs, plain):
        assert not isinstance(out, Exception), (name, out)
        check_structure(name, out, True)
        assert np.array_equal(pillow_canvases(out), judged(name)), name
        assert len(out) <= len(ref), name   # per picture the far coder is never larger than the plain one
    assert sum(map(len, outs)) < sum(map(len, plain))


def run_cli_over_a_tree(binary, tmp_path):
    root = tmp_path / "in"
    root.mkdir()
    (root / "a_anim.webp").write_bytes(inputs()["p_lossy"])
    b = io.BytesIO()
    Image.fromarray(rgba(np.random.default_rng(4), 40, 30, "opaque")[..., :3].copy(), "RGB").save(b, format="WEBP", quality=95)
    (root / "b_still.webp").write_bytes(b.getvalue())
    r = subprocess.run([binary, "-q", "60", "-o", str(tmp_path / "out"), "-R", "--json", str(root)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = json.loads(r.stdout)["files"]
    assert sorted(os.path.basename(f["original_path"]) for f in files) == ["a_anim.webp", "b_still.webp"]
    assert [f["status"] for f in files] == ["success", "success"], files
    out = (tmp_path / "out" / "a_anim.webp").read_bytes()
    check_structure("p_lossy", out, False)
    assert Image.open(io.BytesIO(out)).n_frames == len(judged("p_lossy"))


def test_emul_cli_takes_a_tree_with_an_animation(api, tmp_path):
    run_cli_over_a_tree(EMUL_CLI, tmp_path)
