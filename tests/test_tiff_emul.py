"""TIFF inputs with CSH_TIFF set, on the emulation build: the decoders' tap against a reader written from the TIFF 6.0 text, byte for byte, over
every stream shape the codecs allow; the output against a Python statement of its rule, byte for byte, and against what it must decode to (Pillow / libtiff as a
witness where it is there); metadata, fallbacks, errors, routing and the CLI.  tests/test_zzz_tiff_gpu.py runs the same checks on the device.
Every test but the unset-variable one and the model's check of itself fails without the route: CSH_TIFF is unknown there and the cst_* symbols do not exist."""
import ctypes
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import _lzw_probe as L
import _tiff_model as M
import _tiff_write as W
from _util import ROOT, emul_api, package

CW, CH = 48, 40
BAD_TIFF, UNSUPPORTED, TOO_BIG = 60100, 10201, 10500
EMUL_CLI = os.path.join(ROOT, "tests", "emul", "caesiumclt_emul")


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


def noise(n, seed, high=256):
    return np.random.default_rng(seed).integers(0, high, n).astype(np.uint8).tobytes()


def gradient(w, h, spp):
    """a smooth picture: horizontal differencing leaves runs of equal small bytes"""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(2 * x + 3 * y + 40 * c) % 256 for c in range(spp)], axis=2).astype(np.uint8).tobytes()


def dithered(w, h):
    """four colours in an ordered dither: the bytes repeat with a short period, their differences do not compress better"""
    y, x = np.mgrid[0:h, 0:w]
    pal = np.array([[0, 0, 0], [255, 255, 255], [200, 30, 30], [30, 30, 200]], np.uint8)
    return pal[((x * 7 + y * 3) % 5 + (x // 3 + y // 2) % 3) % 4].tobytes()


def has_libtiff():
    try:
        from PIL import features
        return bool(features.check("libtiff"))
    except Exception:
        return False


def pillow_tiff(arr, compression, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "TIFF", compression=compression, **kw)
    return b.getvalue()


# ------------------------------------------------------------------------------------------------ the decoders
def switch_strips():
    """one-row pictures of noise whose LZW code count puts each width switch (the 255th, 767th and 1791st code behind the Clear is the first of its width) at the
    last data code, one code before it and one behind it"""
    data = noise(2000, 30)
    counts = {}
    for n in range(200, 2000):
        counts.setdefault(len(W.lzw_codes(data[:n])) - 2, n)   # (without the Clear in front and EOI)
    return [("lzw %d codes" % c, W.tiff([W.page(data[:counts[c]], counts[c], 1, compression=W.LZW)])) for k in (254, 766, 1790) for c in (k - 1, k, k + 1)]


def decoder_cases():
    """[(name, file)]"""
    c = []
    for spp in (1, 3, 4):
        c.append(("lzw noise spp %d" % spp, W.tiff([W.page(noise(CW * CH * spp, spp), CW, CH, spp=spp, compression=W.LZW, rows_per_strip=7)])))
    c.append(("lzw flat (KwKwK)", W.tiff([W.page(bytes([9]) * (CW * CH), CW, CH, compression=W.LZW)])))
    big = noise(70 * 70 * 3, 7)   # 14 700 bytes, more than 4094 codes: the table fills
    c.append(("lzw full table, Clear by the text", W.tiff([W.page(big, 70, 70, spp=3, compression=W.LZW)])))
    c.append(("lzw full table, never cleared", W.tiff([W.page(big, 70, 70, spp=3, compression=W.LZW, lzw=dict(clears="never"))])))
    c.append(("lzw Clear every 50 codes, doubled", W.tiff([W.page(noise(CW * CH, 8, 16), CW, CH, compression=W.LZW, lzw=dict(clears=50, double=True))])))
    c.append(("lzw no Clear in front", W.tiff([W.page(noise(CW * CH, 9, 16), CW, CH, compression=W.LZW, rows_per_strip=9, lzw=dict(lead_clear=False))])))
    c.append(("lzw no EOI", W.tiff([W.page(noise(CW * CH, 10, 16), CW, CH, compression=W.LZW, rows_per_strip=9, lzw=dict(eoi=False))])))
    c.append(("lzw no EOI, surplus bytes that read as codes beyond the table", W.tiff([W.page(noise(CW * CH, 24, 16), CW, CH, compression=W.LZW, rows_per_strip=9, lzw=dict(eoi=False), surplus=b"\xff" * 9)])))
    c.append(("lzw surplus bytes", W.tiff([W.page(noise(CW * CH, 11, 16), CW, CH, compression=W.LZW, rows_per_strip=16, surplus=b"\x55" * 7)])))
    c += switch_strips()
    # the encoder's dictionary look-up in its second step of 64 slots (tests/_lzw_probe.py; the replay proves each string does it): one row, one segment at any CSH_TIFF_STRIP
    for name, home, wraps in (("lzw encoder's second probe step", L.FIRST, False), ("lzw encoder's second probe step across the table's end", L.WRAPPING, True)):
        L.check(L.probe_string(home), 4094, wraps)
        c.append((name, W.tiff([W.page(L.probe_string(home), len(L.probe_string(home)), 1, compression=W.LZW)])))
    c.append(("1 x 1", W.tiff([W.page(b"\x7f", 1, 1, compression=W.LZW)])))
    c.append(("one-row strips", W.tiff([W.page(noise(CW * 5, 12), CW, 5, compression=W.LZW, rows_per_strip=1)], big_endian=True)))
    c.append(("a last strip of one row", W.tiff([W.page(noise(CW * 41, 13), CW, 41, compression=W.PACKBITS, rows_per_strip=8)])))
    runs = b"".join(bytes([k + 1]) * n + bytes([200 + k, 100 + k]) for k, n in enumerate((2, 3, 128, 129, 300)))
    runs = runs.ljust(CW * -(-len(runs) // CW), b"\7")
    c.append(("packbits literal only", W.tiff([W.page(bytes(range(240)) * 8, CW, CH, compression=W.PACKBITS, rows_per_strip=11)])))
    c.append(("packbits runs of 2 3 128 129 300", W.tiff([W.page(runs, CW, len(runs) // CW, compression=W.PACKBITS, packbits=dict(cross_rows=True))])))
    c.append(("packbits no-op headers", W.tiff([W.page(runs, CW, len(runs) // CW, compression=W.PACKBITS, rows_per_strip=5, packbits=dict(noop=True))])))
    for name, kw in (("stored", dict(zlevel=0)), ("level 1", dict(zlevel=1)), ("level 9", dict(zlevel=9)), ("fixed", dict(zstrategy=zlib.Z_FIXED))):
        c.append(("deflate " + name, W.tiff([W.page(gradient(CW, CH, 3), CW, CH, spp=3, compression=W.DEFLATE if name != "level 9" else W.ADOBE_DEFLATE, rows_per_strip=13, **kw)])))
    c.append(("deflate noise", W.tiff([W.page(noise(CW * CH * 3, 14), CW, CH, spp=3, compression=W.ADOBE_DEFLATE, rows_per_strip=17)])))
    c.append(("uncompressed", W.tiff([W.page(noise(CW * CH * 3, 15), CW, CH, spp=3, rows_per_strip=6)], big_endian=True)))
    for spp in (1, 3, 4):
        c.append(("predictor 8-bit spp %d" % spp, W.tiff([W.page(gradient(CW, CH, spp), CW, CH, spp=spp, compression=W.LZW, predictor=2, rows_per_strip=9)])))
    for big in (False, True):
        d16 = np.random.default_rng(16).integers(0, 65536, CW * CH * 3).astype(">u2" if big else "<u2").tobytes()
        c.append(("predictor 16-bit " + ("MM" if big else "II"), W.tiff([W.page(d16, CW, CH, spp=3, bits=16, compression=W.ADOBE_DEFLATE if big else W.LZW, predictor=2, rows_per_strip=10)], big_endian=big)))
    c.append(("predictor on a 70-sample row, uncompressed", W.tiff([W.page(noise(70 * 3 * 4, 17), 70, 4, spp=3, predictor=2)])))
    c.append(("tiles 16 x 16 on 48 x 40", W.tiff([W.page(noise(CW * CH * 3, 18), CW, CH, spp=3, compression=W.LZW, tile=(16, 16))])))
    c.append(("tiles 16 x 16 on 50 x 41", W.tiff([W.page(gradient(50, 41, 3), 50, 41, spp=3, compression=W.PACKBITS, tile=(16, 16))], big_endian=True)))
    c.append(("tiles 16 x 16 on 50 x 41, predictor 2", W.tiff([W.page(gradient(50, 41, 1), 50, 41, compression=W.LZW, predictor=2, tile=(16, 16))])))
    c.append(("two pages, two compressions", W.tiff([W.page(noise(CW * CH, 19), CW, CH, compression=W.LZW, rows_per_strip=8), W.page(gradient(30, 20, 3), 30, 20, spp=3, compression=W.PACKBITS)])))
    c.append(("1-bit rows", W.tiff([W.page(noise(7 * CH, 20), 50, CH, bits=1, compression=W.PACKBITS, rows_per_strip=16, photometric=0)])))
    c.append(("4-bit rows", W.tiff([W.page(noise(25 * CH, 21), 49, CH, bits=4, compression=W.LZW, rows_per_strip=16)])))
    cmap = struct.pack("<768H", *[int(v) * 257 for v in np.random.default_rng(22).integers(0, 256, 768)])
    c.append(("palette", W.tiff([W.page(noise(CW * CH, 23), CW, CH, compression=W.LZW, photometric=3, extra=[(320, W.SHORT, 768, cmap)])])))
    return c


def check_decoder(api, cases=None):
    cases = cases or decoder_cases()
    b = api.tiff_batch([c[1] for c in cases])
    try:
        t = b.run()
        assert (t.n_failed, t.n_passed) == (0, 0)
        for i, (name, blob) in enumerate(cases):
            F = M.parse(blob)
            assert F["why"] is None, name
            assert b.pages(i) == len(F["pages"]), name
            for k, p in enumerate(F["pages"]):
                info = b.page_info(i, k)
                assert (info["width"], info["height"], info["rowbytes"], info["nsegments"], info["tiled"]) == (p["width"], p["height"], p["rowbytes"], len(p["segs"]), p["tiled"]), name
                assert b.decoded(i, k) == M.decode_page(blob, F, k), name
    finally:
        b.close()


def test_the_model_reads_what_the_writer_wrote():
    data = noise(CW * CH * 3, 1)
    for kw in (dict(compression=W.LZW, rows_per_strip=7), dict(compression=W.PACKBITS), dict(compression=W.DEFLATE, predictor=2), dict(compression=W.LZW, tile=(16, 16), lzw=dict(clears="never"))):
        blob = W.tiff([W.page(data, CW, CH, spp=3, **kw)])
        assert M.picture(blob, M.parse(blob), 0) == data, kw
    for rows in (bytes([5]) * 300, bytes(range(200)), b"\1\1\2\2\2" + bytes([9]) * 129 + b"\3\3"):
        assert M.packbits_decode(M.packbits_row(rows), len(rows)) == rows and M.packbits_decode(W.packbits_encode([rows]), len(rows)) == rows
    assert M.packbits_row(b"\1\1\2\2\2" + bytes([9]) * 129 + b"\3\3") == b"\1\1\1" + b"\xfe\2" + b"\x81\x09" + b"\0\x09" + b"\1\3\3"


def test_emul_decoder_tap_equals_the_model(api):
    check_decoder(api)


# ------------------------------------------------------------------------------------------------ the output
def output_cases():
    """[(name, file, what Predictor 2 must do on the LZW route: True wins, False loses, None not asked)]"""
    pick = ("lzw noise spp 3", "lzw full table, Clear by the text", "one-row strips", "a last strip of one row", "packbits runs of 2 3 128 129 300", "deflate level 9", "uncompressed", "predictor 16-bit MM",
            "tiles 16 x 16 on 50 x 41, predictor 2", "two pages, two compressions", "1-bit rows", "palette", "1 x 1", "lzw encoder's second probe step", "lzw encoder's second probe step across the table's end")
    c = [(n, b, None) for n, b in decoder_cases() if n in pick]
    assert len(c) == len(pick)
    c.append(("smooth gradient", W.tiff([W.page(gradient(CW, CH, 3), CW, CH, spp=3, photometric=2)]), True))
    c.append(("dithered four colours", W.tiff([W.page(dithered(CW, CH), CW, CH, spp=3, photometric=2, compression=W.PACKBITS)]), False))
    return c


NOT_FOR_PILLOW = {"predictor 16-bit MM"}   # Pillow has no mode for three 16-bit samples a pixel: it opens neither the input nor the output


def run_batch(api, blobs, compression, **kw):
    b = api.tiff_batch(blobs, params(**kw), compression)
    try:
        t = b.run()
        return b.fetch(), t
    finally:
        b.close()


def check_outputs(api, monkeypatch, cases=None):
    cases = cases or output_cases()
    blobs = [c[1] for c in cases]
    counts = {}
    for strip in ("512", "65536"):
        monkeypatch.setenv("CSH_TIFF_STRIP", strip)
        for compression in ("lzw", "packbits", "none"):
            outs, t = run_batch(api, blobs, compression)
            assert t.strip_bytes == int(strip) and (t.n_failed, t.n_passed) == (0, 0)
            won = lost = 0
            for (name, blob, pred), out in zip(cases, outs):
                what = (name, compression, strip)
                verdicts = []
                want = M.recode(blob, compression, int(strip), verdicts=verdicts)
                if compression == "lzw" and pred is not None:
                    assert verdicts == [pred], what   # the case means what it says
                won += verdicts.count(True); lost += verdicts.count(False)
                assert not isinstance(out, Exception), (what, out)
                assert out == want, what
                F, G = M.parse(blob), M.parse(out)
                assert G["why"] is None and len(G["pages"]) == len(F["pages"]), what
                for k in range(len(F["pages"])):
                    assert M.picture(out, G, k) == M.picture(blob, F, k), what
                    assert M.carried(G, k, False) == M.carried(F, k, False), what
                    assert G["pages"][k]["comp"] == {"lzw": 5, "packbits": 32773, "none": 1}[compression], what
                counts[(name, strip)] = len(G["pages"][0]["segs"])
                if has_libtiff() and name not in NOT_FOR_PILLOW:   # the witness: libtiff reads the output to the input's samples
                    from PIL import Image
                    im, src = Image.open(io.BytesIO(out)), Image.open(io.BytesIO(blob))
                    for k in range(len(F["pages"])):
                        im.seek(k); src.seek(k)
                        assert im.size == src.size and im.mode == src.mode and im.tobytes() == src.tobytes(), what
            assert (t.n_pred_won, t.n_pred_lost) == (won, lost), (compression, strip)
    if ("lzw noise spp 3", "512") in counts:   # 144-byte rows: three to a 512-byte strip
        assert counts[("lzw noise spp 3", "512")] == 14 and counts[("lzw noise spp 3", "65536")] == 1


def test_emul_outputs_equal_the_model_and_decode_to_the_input(api, monkeypatch):
    check_outputs(api, monkeypatch)


def check_pillow_files(api):
    """the decoder tap on files libtiff wrote, every compression; conditional on Pillow having libtiff (the model checks above never are)"""
    if not has_libtiff():
        return
    arr = np.frombuffer(gradient(CW, CH, 3), np.uint8).reshape(CH, CW, 3) ^ np.frombuffer(noise(CW * CH * 3, 40, 4), np.uint8).reshape(CH, CW, 3)
    grey = arr[:, :, 0].copy()
    blobs = [pillow_tiff(a, c) for a in (arr, grey) for c in ("raw", "tiff_lzw", "tiff_adobe_deflate", "tiff_deflate", "packbits")]
    blobs.append(pillow_tiff(arr, "tiff_lzw", tiffinfo={317: 2}))
    b = api.tiff_batch(blobs)
    try:
        b.run()
        for i, blob in enumerate(blobs):
            want = (arr if i < 5 or i == 10 else grey).tobytes()
            assert b.decoded(i, 0) == want == M.picture(blob, M.parse(blob), 0), i
    finally:
        b.close()


def test_emul_decoder_reads_what_libtiff_writes(api):
    check_pillow_files(api)


# ------------------------------------------------------------------------------------------------ metadata
def rich_file(big_endian=False):
    E = ">" if big_endian else "<"
    asc = lambda s: (W.ASCII, len(s) + 1, s.encode() + b"\0")
    extra = [(270,) + asc("a description longer than four bytes"), (271,) + asc("mk"), (305,) + asc("the software"), (315,) + asc("artist"), (33432,) + asc("(c) somebody"),
             (282, W.RATIONAL, 1, struct.pack(E + "II", 300, 1)), (283, W.RATIONAL, 1, struct.pack(E + "II", 300, 1)), (296, W.SHORT, 1, struct.pack(E + "H", 2)),
             (34675, W.UNDEFINED, 40, bytes(range(40))), (700, W.BYTE, 9, b"<x:xmp/> ")]
    exif = [(33434, W.RATIONAL, 1, struct.pack(E + "II", 1, 125)), (36867,) + asc("2020:01:02 03:04:05"), (37500, W.UNDEFINED, 11, b"maker\0note!"), (40962, W.LONG, 1, struct.pack(E + "I", CW)),
            (40965, W.LONG, 1, struct.pack(E + "I", 8))]
    gps = [(1,) + asc("N"), (2, W.RATIONAL, 3, struct.pack(E + "6I", 48, 1, 8, 1, 30, 1))]
    return W.tiff([W.page(gradient(CW, CH, 3), CW, CH, spp=3, photometric=2, compression=W.PACKBITS, extra=extra, exif=exif, gps=gps)], big_endian=big_endian)


def check_metadata(api):
    for big in (False, True):
        blob = rich_file(big)
        F = M.parse(blob)
        E = ">" if big else "<"
        for keep in (False, True):
            (out,), t = run_batch(api, [blob], "lzw", keep_metadata=keep)
            assert out == M.recode(blob, "lzw", keep_metadata=keep), (big, keep)
            G = M.parse(out)
            tags = {e[0]: e for e in G["pages"][0]["entries"]}
            assert M.carried(G, 0) == M.carried(F, 0, keep) and 34675 in tags and tags[34675][3] == bytes(range(40))
            assert [e[0] for e in G["pages"][0]["entries"]] == sorted(tags)
            had = {e[0] for e in F["pages"][0]["entries"]} & M.DROPPED
            assert had == {270, 271, 305, 315, 700, 33432, 34665, 34853} and all((tag in tags) == keep for tag in had), (big, keep)
            if keep:   # the private IFDs read back entry for entry, out-of-line values included, without the interoperability pointer
                for tag, src in ((34665, 34665), (34853, 34853)):
                    got, nxt = M.read_ifd(out, E, M.numbers(E, tags[tag])[0])
                    want, _ = M.read_ifd(blob, E, M.numbers(E, {e[0]: e for e in F["pages"][0]["entries"]}[src])[0])
                    assert nxt == 0 and got == [e for e in want if e[0] != 40965] and len(got) >= 2
            assert M.picture(out, G, 0) == M.picture(blob, F, 0)


def test_emul_metadata_is_kept_under_keep_metadata_only(api):
    check_metadata(api)


# ------------------------------------------------------------------------------------------------ fallbacks and errors
def good_file(seed=50):
    return W.tiff([W.page(gradient(CW, CH, 3), CW, CH, spp=3, photometric=2, rows_per_strip=8)])


def many_pages(n):
    """n pages of 1 x 1 one-bit pixels that share one strip, written by hand: the test writer would take seconds over 65536 of them"""
    body = struct.pack("<H", 4) + b"".join(struct.pack("<HHII", tag, W.LONG, 1, v) for tag, v in ((256, 1), (257, 1), (273, 8), (279, 1)))
    return b"II*\0" + struct.pack("<I", 10) + b"\x80\0" + b"".join(body + struct.pack("<I", 10 + 54 * (k + 1) if k + 1 < n else 0) for k in range(n))


def fallback_cases():
    data = noise(CW * CH * 3, 51)
    rgb = dict(spp=3, photometric=2)
    old = bytes([0, 1]) + noise(100, 52)   # old-style LZW: libtiff's test on the first two bytes
    return {"JPEG compression": W.tiff([W.page(data, CW, CH, compression=7, segments=[noise(64, 53)], **rgb)]),
            "CCITT compression": W.tiff([W.page(noise(6 * CH, 54), CW, CH, bits=1, compression=4, segments=[noise(64, 55)])]),
            "separate planes": W.tiff([W.page(data, CW, CH, planar=2, **rgb)]),
            "floating-point predictor": W.tiff([W.page(data, CW, CH, predictor=3, **rgb)]),
            "predictor 2 at 4 bits": W.tiff([W.page(b"", CW, CH, bits=4, predictor=2, compression=W.LZW, segments=[W.lzw_encode(noise(24 * CH, 56))])]),
            "fill order 2": W.tiff([W.page(data, CW, CH, fillorder=2, **rgb)]),
            "SubIFDs": W.tiff([W.page(data, CW, CH, extra=[(330, W.LONG, 1, struct.pack("<I", 8))], **rgb)]),
            "YCbCr 2 x 2": W.tiff([W.page(data, CW, CH, spp=3, photometric=6)]),
            "old-style LZW": W.tiff([W.page(data, CW, CH, compression=W.LZW, segments=[old], **rgb)]),
            "more than 2^31 decoded bytes": W.tiff([W.page(b"", 40000, 20000, compression=W.LZW, segments=[noise(64, 57)], **rgb)]),
            "more than 65535 pages": many_pages(65536),
            "a field type that cannot be sized": W.tiff([W.page(data, CW, CH, extra=[(65000, 99, 1, b"\1\0\0\0")], **rgb)], type_sizes={99: 4}),
            "predictor 2 on 65 samples a pixel": W.tiff([W.page(noise(4 * 4 * 65, 59), 4, 4, spp=65, predictor=2, compression=W.LZW)]),
            "more than 65535 samples a pixel": W.tiff([W.page(data, CW, CH, override={277: (W.LONG, 1, struct.pack("<I", 70000))}, **rgb)]),
            "more than 2^20 bits a pixel": W.tiff([W.page(data, CW, CH, override={258: (W.LONG, 3, struct.pack("<3I", 1 << 19, 1 << 19, 8))}, **rgb)]),
            "more than 2^20 rows in a page": W.tiff([W.page(b"", 1, (1 << 20) + 1, compression=W.LZW, rows_per_strip=1, override={278: (W.LONG, 1, struct.pack("<I", (1 << 20) + 1))}, segments=[noise(64, 61)])]),
            "more than 2^20 segments in a page": W.tiff([W.page(b"", 1 << 11, 1 << 11, compression=W.LZW, tile=(1, 1), override={324: (W.LONG, 1, struct.pack("<I", 8)), 325: (W.LONG, 1, struct.pack("<I", 8))}, segments=[b""])])}


def check_fallbacks(api):
    cases = fallback_cases()
    good = good_file()
    blobs = [good]
    for name, blob in cases.items():
        assert M.recode(blob, "lzw") == blob, name   # (the model returns the input for a file it has a reason to pass through, and for no other)
        blobs += [blob, good]
    outs, t = run_batch(api, blobs, "lzw")
    want = M.recode(good, "lzw")
    for i, name in enumerate(cases):
        assert outs[1 + 2 * i] == blobs[1 + 2 * i], name
    assert all(o == want for o in outs[0::2]) and want != good
    assert (t.n_passed, t.n_failed, t.n_files) == (len(cases), 0, len(blobs))
    ycc = W.tiff([W.page(noise(CW * CH * 3, 58), CW, CH, spp=3, photometric=6, extra=[(530, W.SHORT, 2, struct.pack("<HH", 1, 1))])])   # YCbCr without subsampling is coded
    (out,), t = run_batch(api, [ycc], "packbits")
    assert out == M.recode(ycc, "packbits") != ycc and t.n_passed == 0


def test_emul_fallbacks_return_the_input(api):
    check_fallbacks(api)


def malformed_cases():
    data = noise(CW * CH, 60, 16)
    good = W.tiff([W.page(data, CW, CH, compression=W.LZW)])
    ifd = struct.unpack_from("<I", good, 4)[0]
    bits = W.Bits()
    for code, width in ((256, 9), (5, 9), (259, 9)):   # Clear, 5, 259: the next free entry is 258
        bits.put(code, width)
    lzw = W.lzw_encode(data)
    pb = W.packbits_encode([data[:CW * CH - 1]]) + b"\xfd\x07"   # the last packet holds four bytes where one is left
    z = zlib.compress(data)
    return {"truncated IFD": good[:ifd + 20], "IFD offset past the end": W.tiff([W.page(data, CW, CH)], first_ifd=1 << 20),
            "strip offset past the end": W.tiff([W.page(data, CW, CH, override={273: (W.LONG, 1, struct.pack("<I", 1 << 20))})]),
            "IFD loop": W.tiff([W.page(data, CW, CH), W.page(data, CW, CH)], next_of_last="first"),
            "strip arrays of the wrong length": W.tiff([W.page(data, CW, CH, rows_per_strip=8, override={279: (W.LONG, 4, struct.pack("<4I", 1, 1, 1, 1))})]),
            "zero width": W.tiff([W.page(data, CW, CH, override={256: (W.LONG, 1, struct.pack("<I", 0))})]),
            "no byte counts": W.tiff([W.page(data, CW, CH, drop=[279])]),
            "LZW code beyond the table": W.tiff([W.page(data, CW, CH, compression=W.LZW, segments=[bits.bytes()])]),
            "LZW first code beyond the bytes": W.tiff([W.page(data, CW, CH, compression=W.LZW, segments=[b"\x80\x40\x80" + lzw])]),
            "LZW data one byte short": W.tiff([W.page(data, CW, CH, compression=W.LZW, segments=[W.lzw_encode(data, eoi=False)[:-1]])]),
            "LZW EOI too early": W.tiff([W.page(data, CW, CH, compression=W.LZW, segments=[W.lzw_encode(data[:900])])]),
            "uncompressed data short": W.tiff([W.page(data, CW, CH, segments=[data[:-1]])]),
            "PackBits packet overruns the segment": W.tiff([W.page(data, CW, CH, compression=W.PACKBITS, segments=[pb])]),
            "PackBits data short": W.tiff([W.page(data, CW, CH, compression=W.PACKBITS, segments=[W.packbits_encode([data])[:-3]])]),
            "Deflate without a zlib header": W.tiff([W.page(data, CW, CH, compression=W.DEFLATE, segments=[z[2:]])]),
            "Deflate stream short": W.tiff([W.page(data, CW, CH, compression=W.DEFLATE, segments=[zlib.compress(data[:1000])])]),
            "Deflate stream broken": W.tiff([W.page(data, CW, CH, compression=W.DEFLATE, segments=[z[:2] + b"\x07" + z[3:]])])}


def check_malformed(api):
    good = good_file()
    cases = malformed_cases()
    blobs = [good]
    for name, bad in cases.items():
        with pytest.raises(M.BadTiff):
            M.recode(bad, "lzw")
        blobs += [bad, good]
    outs, t = run_batch(api, blobs, "lzw")
    want = M.recode(good, "lzw")
    for i, name in enumerate(cases):
        assert isinstance(outs[1 + 2 * i], Exception) and outs[1 + 2 * i].code == BAD_TIFF, (name, outs[1 + 2 * i])
    assert all(o == want for o in outs[0::2]) and t.n_failed == len(cases)


def test_emul_malformed_files_fail_alone(api):
    check_malformed(api)


# ------------------------------------------------------------------------------------------------ routing
def mixed_call():
    from gen_synth import synth_jpeg, synth_png
    return [synth_jpeg(0, 64, 48, texture=20), good_file(), synth_png(2, 40, 30, "RGB", compress_level=1), rich_file(True)]


def comp_of(blob):
    return M.parse(blob)["pages"][0]["comp"]


def check_routing(api, monkeypatch):
    blobs = mixed_call()
    tif = blobs[1]
    monkeypatch.delenv("CSH_TIFF", raising=False)
    monkeypatch.delenv("CSH_TIFF_STRIP", raising=False)
    plain = api.cs_batch_compress(blobs, params())
    assert plain[1] == tif and plain[3] == blobs[3]
    monkeypatch.setenv("CSH_TIFF", "pass")
    assert api.cs_batch_compress(blobs, params()) == plain
    monkeypatch.setenv("CSH_TIFF", "device")
    for number, name, tag in ((0, "none", 1), (1, "lzw", 5), (3, "packbits", 32773), (7, "none", 1)):
        dev = api.cs_batch_compress(blobs, params(tiff_compression=number))   # a mixed call keeps the order of its inputs
        assert [dev[0], dev[2]] == [plain[0], plain[2]] and dev[1] == M.recode(tif, name) and dev[3] == M.recode(blobs[3], name) and comp_of(dev[1]) == tag, number
    dev = api.cs_batch_compress(blobs, params(tiff_compression=2))
    assert [dev[0], dev[2]] == [plain[0], plain[2]]
    for k in (1, 3):
        assert isinstance(dev[k], Exception) and dev[k].code == UNSUPPORTED and "Deflate coder is not built" in str(dev[k])
    for name, tag in (("lzw", 5), ("packbits", 32773), ("none", 1)):   # the value overrides the parameter
        monkeypatch.setenv("CSH_TIFF", name)
        for number in (0, 1, 2, 3):
            assert api.compress_in_memory(tif, params(tiff_compression=number)) == M.recode(tif, name)
    monkeypatch.setenv("CSH_TIFF", "bogus")
    bogus = api.cs_batch_compress(blobs, params())
    assert [bogus[0], bogus[2]] == [plain[0], plain[2]]
    for k in (1, 3):
        assert isinstance(bogus[k], Exception) and bogus[k].code == UNSUPPORTED and "CSH_TIFF" in str(bogus[k]) and "packbits" in str(bogus[k])
    monkeypatch.setenv("CSH_TIFF", "lzw")
    want = M.recode(tif, "lzw")
    with pytest.raises(Exception) as e:   # a resize of a TIFF file is refused as before
        api.compress_in_memory(tif, params(width=24))
    assert e.value.code == UNSUPPORTED and "resizing a GIF / TIFF" in str(e.value)
    with pytest.raises(Exception) as e:   # ... and so is a conversion from or to TIFF
        api.convert_in_memory(tif, params(), 1)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(Exception) as e:
        api.convert_in_memory(blobs[0], params(), 4)
    assert e.value.code == UNSUPPORTED
    # the size walk: one run, then the target rule on the coded size
    assert api.batch_compress_to_size([tif], params(), len(want), return_smallest=False) == [want]
    r = api.batch_compress_to_size([tif], params(), len(want) - 1, return_smallest=False)[0]
    assert isinstance(r, Exception) and r.code == TOO_BIG and "no quality to walk" in str(r)
    assert api.batch_compress_to_size([tif], params(), len(want) - 1, return_smallest=True) == [want]
    # the coded file is returned even when it is larger than the input
    small = W.tiff([W.page(noise(CW * CH, 70), CW, CH, compression=W.PACKBITS)])
    assert len(api.compress_in_memory(small, params())) > len(small)


def test_emul_routing_under_each_setting(api, monkeypatch):
    check_routing(api, monkeypatch)


@pytest.mark.parametrize("value", [None, "", "pass"])
def test_emul_tiff_is_passed_through_without_the_variable(api, monkeypatch, value):
    """passes on the code before the route too, on purpose: the variable is opt-in"""
    if value is None:
        monkeypatch.delenv("CSH_TIFF", raising=False)
    else:
        monkeypatch.setenv("CSH_TIFF", value)
    blobs = mixed_call()
    outs = api.cs_batch_compress(blobs, params(tiff_compression=1))
    assert outs[1] == blobs[1] and outs[3] == blobs[3] and not isinstance(outs[0], Exception) and not isinstance(outs[2], Exception)


def run_cli_over_tiffs(binary, tmp_path):
    data = gradient(CW, CH, 3)
    tif = W.tiff([W.page(data, CW, CH, spp=3, photometric=2, rows_per_strip=8)])
    src, out = tmp_path / "in", tmp_path / "out"
    (src / "deep").mkdir(parents=True)
    (src / "a.tif").write_bytes(tif)
    (src / "deep" / "b.tiff").write_bytes(tif)
    env = dict(os.environ, CSH_TIFF="lzw")
    env.pop("CSH_TIFF_STRIP", None)
    r = subprocess.run([binary, "-q", "80", "-R", "-S", "-o", str(out), str(src)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    single = tmp_path / "single"
    r = subprocess.run([binary, "-q", "80", "-o", str(single), str(src / "a.tif")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    for got in (out / "a.tif", out / "deep" / "b.tiff", single / "a.tif"):
        blob = got.read_bytes()
        assert len(blob) < len(tif) and blob == M.recode(tif, "lzw") and M.picture(blob, M.parse(blob), 0) == data, got
    env.pop("CSH_TIFF")   # without the variable the scanner is the reference's: it knows no TIFF file
    r = subprocess.run([binary, "-q", "80", "-R", "-S", "-o", str(tmp_path / "none"), str(src)], capture_output=True, text=True, env=env)
    assert not (tmp_path / "none" / "a.tif").exists() and not (tmp_path / "none" / "deep" / "b.tiff").exists(), r.stdout


def test_emul_cli_compresses_tiff_files_under_the_variable_only(api, tmp_path):
    run_cli_over_tiffs(EMUL_CLI, tmp_path)


# ------------------------------------------------------------------------------------------------ order independence, the interface
def test_emul_outputs_do_not_depend_on_the_launch_order(api, monkeypatch):
    fn = api.L.csh_emul_set_reverse
    fn.argtypes = [ctypes.c_int]
    fn(1)
    try:
        check_decoder(api, decoder_cases()[:12])
        check_outputs(api, monkeypatch, output_cases()[-6:])
    finally:
        fn(0)


def test_header_binding_and_libraries_agree_on_the_tiff_entry_points(api):
    import re
    hdr = open(os.path.join(ROOT, "include", "caesium_hip.h")).read()
    declared = set(re.findall(r"\b(cst_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(package().binding.TIFF_EXPORTS) and "CS_ERR_BAD_TIFF = 60100" in hdr
    for lib in (api.L, ctypes.CDLL(package().library_path())):
        for name in sorted(declared):
            assert hasattr(lib, name), name
    assert api.tiff_kernel_names() == ["tiff_lzw_decode", "tiff_packbits_decode", "tiff_place", "tiff_inflate", "tiff_unpredict", "tiff_predict", "tiff_lzw_encode", "tiff_packbits_encode",
                                       "tiff_layout", "tiff_gather", "tiff_patch"]
