"""The mixed batches of test_routes_emul.py and test_zzz_routes_gpu.py: one small file per kind of input, kinds interleaved, and per file what each entry point must
answer -- stated with the oracle helper the route's own test file uses (_util.oracle_*, and the libwebp-pinned checks of test_webp_decode_emul.py /
test_webp_anim_emul.py).  No picture is larger than 64 x 48."""
import functools
import io

import numpy as np
from PIL import Image

JPEG, PNG, WEBP = 0, 1, 3
UNKNOWN_TYPE, UNSUPPORTED, SAME_FORMAT, TOO_BIG = 10200, 10201, 10407, 10500


@functools.lru_cache(maxsize=None)
def files():
    """[(name, kind, bytes)], kinds interleaved: jpeg / png / webp (opaque still) / webp_alpha / webp_anim / pass (GIF, TIFF) / garbage"""
    import test_webp_anim_emul as WA
    import test_webp_decode_emul as WD
    from gen_synth import synth_jpeg, synth_png, synth_rgb
    yy, xx = np.mgrid[0:17, 0:33]
    rgba = np.dstack([synth_rgb(300, 33, 17, texture=10.0), ((xx * 255) // 32).astype(np.uint8)])

    def webp(arr, mode, **kw):
        b = io.BytesIO()
        Image.fromarray(arr, mode).save(b, format="WEBP", **kw)
        return b.getvalue()

    def other(fmt):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(5, 20, 14), "RGB").save(b, format=fmt)
        return b.getvalue()
    jpegs = [("jpeg_baseline", synth_jpeg(0, 64, 48, texture=10.0)), ("jpeg_progressive", synth_jpeg(1, 56, 40, progressive=True, subsampling=1, texture=20.0)),
             ("jpeg_restarts", synth_jpeg(2, 48, 32, restart_rows=1, texture=5.0))]
    pngs = [("png_" + m, synth_png(10 + k, 47, 31, m, texture=2.0 + k)) for k, m in enumerate(["RGB", "RGBA", "L", "LA", "P", "1", "I;16"])]
    webps = [("webp_lossy", "webp", WD.webp_of(30, 64, 48, 80)), ("webp_lossless", "webp", WD.lossless_of(synth_rgb(60, 40, 30, texture=10.0))),
             ("webp_lossy_alpha", "webp_alpha", webp(rgba, "RGBA", quality=80)), ("webp_lossless_alpha", "webp_alpha", webp(rgba, "RGBA", lossless=True)),
             ("single", "webp_anim", WA.inputs()["single"])]   # (an animation's name is its name in test_webp_anim_emul.inputs())
    rest = [("gif", "pass", other("GIF")), ("tiff", "pass", other("TIFF")), ("garbage", "garbage", bytes(range(7, 200)))]
    groups = [[(n, "jpeg", b) for n, b in jpegs], [(n, "png", b) for n, b in pngs], webps, rest]
    return [g[k] for k in range(max(len(g) for g in groups)) for g in groups if k < len(g)]


def riff_chunks(blob):
    from test_png_webp_emul import riff_chunks as chunks
    return chunks(blob)


def webp_rgba(blob):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(blob)).convert("RGBA")))


def failed(out, code):
    assert isinstance(out, Exception) and out.code == code, out


def check_webp_alpha_lossy(out, src, quality):
    """VP8X + ALPH + VP8: the frame is the oracle's frame of the colour libwebp reads from the source, the plane comes back exactly (libwebp is the judge)"""
    from oracle import oracle as O
    want = webp_rgba(src)
    chunks = riff_chunks(out)
    assert [c[0] for c in chunks] == [b"VP8X", b"ALPH", b"VP8 "]
    assert chunks[2][1] == riff_chunks(O.webp_encode_rgb(np.ascontiguousarray(want[:, :, :3]), quality))[0][1]
    assert np.array_equal(webp_rgba(out)[:, :, 3], want[:, :, 3])


def check_compress(name, kind, src, out, p):
    """cs_batch_compress's answer for one file under the parameters p (no size)"""
    import test_webp_anim_emul as WA
    from _util import oracle_lossless, oracle_lossy, oracle_png, oracle_png_lossy
    from oracle import oracle as O
    from test_webp_lossless_emul import check_vp8l
    if kind == "garbage":
        return failed(out, UNKNOWN_TYPE)
    assert isinstance(out, bytes), (name, out)
    if kind == "pass":
        assert out == src
    elif kind == "jpeg":
        assert out == (oracle_lossless(src) if p.jpeg_optimize else oracle_lossy(src, p.jpeg_quality))
    elif kind == "png":
        assert out == (oracle_png(src, p.png_optimization_level) if p.png_optimize else oracle_png_lossy(src, p.png_optimization_level, quality=p.png_quality))
    elif kind == "webp_anim":
        WA.check_structure(name, out, bool(p.webp_lossless))
        if p.webp_lossless:
            assert np.array_equal(WA.pillow_canvases(out), WA.judged(name))
    elif p.webp_lossless:
        if kind == "webp":
            check_vp8l(out, webp_rgba(src)[:, :, :3])
        else:
            assert out[8:16] == b"WEBPVP8L" and np.array_equal(webp_rgba(out), webp_rgba(src))
    elif kind == "webp":
        assert out == O.webp_encode_rgb(np.ascontiguousarray(webp_rgba(src)[:, :, :3]), p.webp_quality)
    else:
        check_webp_alpha_lossy(out, src, p.webp_quality)


def check_convert(name, kind, src, out, p, fmt):
    """cs_batch_convert's answer for one file towards fmt under p (no size)"""
    from _util import device_quantiser, device_scan_script, oracle_jpeg_to_png, oracle_jpeg_to_webp, oracle_png_to_jpeg, raw_png
    from oracle import oracle as O
    from test_png_webp_emul import check as check_png_to_webp
    from test_webp_lossless_emul import check_vp8l, oracle_vp8l
    source ={"jpeg": JPEG, "png": PNG, "webp": WEBP, "webp_alpha": WEBP, "webp_anim": WEBP}.get(kind)
    if kind == "garbage":
        return failed(out, UNKNOWN_TYPE)
    if source == fmt:
        return failed(out, SAME_FORMAT)
    if kind in ("pass", "webp_anim"):
        return failed(out, UNSUPPORTED)
    if kind == "png" and fmt == WEBP and not p.webp_lossless:   # (its own check: transparency and 16-bit samples have rules of their own there)
        return check_png_to_webp(_Single(out), [(name, src)], p.webp_quality)   # (a picture it has no path for must fail with the oracle's code)
    assert isinstance(out, bytes), (name, out)
    if kind == "jpeg" and fmt == WEBP and not p.webp_lossless:
        assert out == oracle_jpeg_to_webp(src, p.webp_quality)
    elif kind == "jpeg":   # to PNG, or to lossless WebP: exactly the pixels of the PNG the oracle makes of the same decode
        want = oracle_jpeg_to_png(src, bool(p.png_optimize), p.png_optimization_level, quality=p.png_quality)
        if fmt == PNG:
            assert out == want
        else:
            check_vp8l(out, np.asarray(Image.open(io.BytesIO(oracle_jpeg_to_png(src, True, 1))).convert("RGB")))
    elif kind == "png" and fmt == JPEG:
        assert out == oracle_png_to_jpeg(src, p.jpeg_quality)
    elif kind == "png":   # lossless WebP: what libpng reads, alpha included; 16-bit samples narrowed as image-rs does (the lossy PNG -> WebP path pins the rule)
        want = np.asarray(Image.open(io.BytesIO(src)))
        want = np.asarray(Image.fromarray(((want.astype(np.uint32) + 128) // 257).astype(np.uint8), "L").convert("RGBA")) if name == "png_I;16" else np.asarray(Image.open(io.BytesIO(src)).convert("RGBA"))
        assert out[8:16] == b"WEBPVP8L" and np.array_equal(webp_rgba(out), want) and out == oracle_vp8l(out)
    elif fmt == JPEG:   # a WebP file: the plane, if any, is dropped
        assert out == O.pixels_to_jpeg(np.ascontiguousarray(webp_rgba(src)[:, :, :3]), O.params(quality=p.jpeg_quality, progressive=1, subsampling=420, qtable_profile=3, marker_style=1,
                                                                                                scan_script=device_scan_script(), **device_quantiser()), 0, 0)
    else:   # to PNG: the PNG path over a PNG file of the pixels libwebp reads (RGBA where the picture has transparency), as for a JPEG source
        px = webp_rgba(src)
        png = raw_png(px if kind == "webp_alpha" else np.ascontiguousarray(px[:, :, :3]), 6 if kind == "webp_alpha" else 2)
        assert out == (O.png_optimize(png, p.png_optimization_level)[0] if p.png_optimize else O.png_lossy(png, p.png_optimization_level, False, p.png_quality))


class _Single:
    """test_png_webp_emul.check asks an api for the output of its one file: this one hands it the answer the mixed batch gave"""

    def __init__(self, out):
        self.out = out

    def batch_convert(self, blobs, p, fmt):
        return [self.out]

    def convert_in_memory(self, src, p, fmt):
        return self.out
