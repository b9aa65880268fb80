"""Output pools that overflow and grow, on every route.  A batch sizes its output pools from an estimate; a file that does not fit is reported by the kernels, the
host makes the pool four times larger and runs the batch again, three times at the most.  Here that loop runs for the pools the other tests never fill:

* the lossy WebP encoder's reservation (4096 + macroblocks x (768 + 2) bytes a file), which CSH_TEST_POOL_SHIFT divides at the start: shift 4 begins at 48 bytes a
  macroblock (192, then 768 after the retries), shift 16 at 0, which no retry makes larger -- the files above the flat part fail alone with CS_ERR_POOL_OVERFLOW;
* the JPEG coder's raw-scan / output pool, which an ordinary call overflows: a small noise JPEG enlarged at quality 100.

Every file is compared byte for byte with the oracle the route's own tests use, and n_pool_retries (csh_timing / csp_timing; csh_last_pool_retries() for the
one-call entries) says that the retries happened: a hook that is silently ignored fails here.  Which pictures overflow is asserted from the oracle's files.
The same bodies run on the device in test_zzz_pool_growth_gpu.py."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from _util import ROOT, emul_api, oracle_jpeg_to_webp, oracle_lossy, oracle_resized, package
from gen_synth import synth_jpeg, synth_rgb

Image = pytest.importorskip("PIL.Image")
WEBP = 3
POOL_OVERFLOW = 20200


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


def set_env(monkeypatch, **kw):
    for k, v in kw.items():
        if v is None: monkeypatch.delenv(k, raising=False)
        else: monkeypatch.setenv(k, str(v))


# ------------------------------------------------------------------------------------------------ the pictures
def macroblocks(w, h):
    return ((w + 15) // 16) * ((h + 15) // 16)


def save(arr, mode, fmt, **kw):
    b = io.BytesIO()
    Image.fromarray(arr, mode).save(b, fmt, **kw)
    return b.getvalue()


def busy_rgb():
    return synth_rgb(9, 200, 150, texture=90)


def busy_jpeg():
    return synth_jpeg(9, 200, 150, texture=90)        # test_webp_emul.py's busy_200x150: 130 macroblocks


def flat_jpeg():
    return synth_jpeg(3, 64, 48)                      # flat_64x48: 80 bytes of WebP


def mid_jpeg():
    return synth_jpeg(1, 160, 96, texture=10)         # 420_160x96: 60 macroblocks


def noise_png_1bit():
    bits = np.random.default_rng(2).integers(0, 2, (96, 160), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(bits * 255, "L").convert("1").save(b, "PNG")
    return b.getvalue()


def busy_rgba_png():
    rgb = busy_rgb()
    yy, xx = np.mgrid[0:150, 0:200]
    alpha = ((xx * 255) // 199).astype(np.uint8)
    alpha[(yy // 10) % 3 == 0] = 255
    return save(np.dstack([rgb, alpha]), "RGBA", "PNG")


def busy_webp():
    return save(busy_rgb(), "RGB", "WEBP", quality=90)


def libwebp_rgb(blob):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(blob)).convert("RGB")))


def noise_jpeg_64x48(subsampling=2):
    """the raw pool's natural trigger: 64 x 48 of white noise at quality 30, about 1.5 KB as 4:2:0 (2.3 KB as 4:4:4, subsampling=0) -- the pools are sized from
    that, the output from the call's width"""
    return save(np.random.default_rng(5).integers(0, 256, (48, 64, 3), dtype=np.uint8), "RGB", "JPEG", quality=30, subsampling=subsampling)


def small_jpeg():
    return synth_jpeg(3, 64, 48)                      # flat: small at any size


# ------------------------------------------------------------------------------------------------ what has to overflow, from the oracle's file
def vp8_chunk(blob):
    at = 12
    while at < len(blob):
        n = int.from_bytes(blob[at + 4:at + 8], "little")
        if blob[at:at + 4] == b"VP8 ":
            return blob[at + 8:at + 8 + n]
        at += 8 + n + (n & 1)
    raise AssertionError("no VP8 chunk")


def webp_room(nmb, mb_bytes):
    """a file's region and its two halves for a reservation of mb_bytes a macroblock: (file, first partition, token partition).  The region is 4096 + macroblocks
    x (mb_bytes + 2); a sixteenth of what is above the flat 4096, plus 2048, holds the first partition, the rest less 128 the token partition (k_webp.hip)"""
    cap = 4096 + nmb * (mb_bytes + 2)
    first = 2048 + ((cap - 4096) >> 4)
    return cap, first, cap - 128 - first


def growths(want, nmb, shift=4):
    """how many times the reservation has to grow for the oracle's file `want` (a plain VP8 file, or the extended form around one), from the file alone.  Asserts what
    the cases rest on: a picture meant to overflow is LARGER than the region (so it cannot fit whatever the split), and one meant to fit after a growth fits both
    halves with room to spare (64 bytes: the model of the split is not tested to the byte here)"""
    frame = vp8_chunk(want)
    p0 = int.from_bytes(frame[:3], "little") >> 5
    p1 = len(frame) - 10 - p0
    total = 20 + len(frame) + (len(frame) & 1)
    for n in range(4):
        cap, first, rest = webp_room(nmb, (768 >> shift) << (2 * n))
        if total > cap:
            continue
        assert total + 64 <= cap and p0 + 64 <= first and p1 + 64 <= rest, ("too close to a reservation to say how often it grows", total, p0, p1, cap, first, rest)
        return n
    return 4


def check_growths(name, want, nmb, expect):
    """the precondition of a case, from the oracle's file alone: above 4096 + mb x (48 + 2) for one growth, above 4096 + mb x (192 + 2) for two"""
    total = 20 + len(vp8_chunk(want)) + (len(vp8_chunk(want)) & 1)
    if expect >= 1: assert total > 4096 + nmb * (48 + 2), (name, total)
    if expect >= 2: assert total > 4096 + nmb * (192 + 2), (name, total)
    assert growths(want, nmb) == expect, (name, total, growths(want, nmb))


# ------------------------------------------------------------------------------------------------ WebP, shift 4, every route that ends in the VP8 encoder
def check_jpeg_to_webp_grows(api, monkeypatch, width=0, nmb=130):
    """JPEG -> WebP through the batch object (csh_timing) and through cs_batch_convert (the last-call reader): busy_200x150 needs one growth at quality 85, two at 100"""
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=4)
    src = busy_jpeg()
    seen = []
    for q, expect in ((85, 1), (100, 2)):
        want = oracle_jpeg_to_webp(src, q, width, 0)
        check_growths(("jpeg", q, width), want, nmb, expect)
        b = api.webp_batch([src], params(webp_quality=q, width=width))
        try:
            t = b.run()
            assert b.fetch() == [want], q
        finally:
            b.close()
        assert t.n_pool_retries == expect, (q, t.n_pool_retries)
        api.last_pool_retries()
        assert api.batch_convert([src], params(webp_quality=q, width=width), WEBP) == [want]
        assert api.last_pool_retries() == expect
        seen.append(int(t.n_pool_retries))
    return seen


def test_jpeg_to_webp_grows_once_and_twice(api, monkeypatch):
    assert check_jpeg_to_webp_grows(api, monkeypatch) == [1, 2]


def test_jpeg_to_webp_with_a_width_grows(api, monkeypatch):
    """the resize branch in front: 200 x 150 -> 260 x 195, 221 macroblocks"""
    assert check_jpeg_to_webp_grows(api, monkeypatch, width=260, nmb=macroblocks(260, 195)) == [1, 2]


def check_png_to_webp_grows(api, monkeypatch):
    """opaque PNG -> WebP through the PNG batch object (csp_timing): the busy picture once at quality 85 and twice at 100, 1-bit noise of 160 x 96 twice at 100"""
    from oracle import oracle as O
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=4)
    busy, noise = save(busy_rgb(), "RGB", "PNG"), noise_png_1bit()
    seen = []
    for name, src, nmb, q, expect in (("busy", busy, 130, 85, 1), ("busy", busy, 130, 100, 2), ("noise_1bit_160x96", noise, 60, 100, 2)):
        want = O.png_to_webp(src, q)
        check_growths((name, q), want, nmb, expect)
        b = api.png_webp_batch([src], params(webp_quality=q))
        try:
            t = b.run()
            assert b.fetch() == [want], (name, q)
            t2 = b.run()                                 # the reservation that grew stays with the batch object
            assert b.fetch() == [want] and t2.n_pool_retries == 0, (name, q)
        finally:
            b.close()
        assert t.n_pool_retries == expect, (name, q, t.n_pool_retries)
        seen.append(int(t.n_pool_retries))
    return seen


def test_png_to_webp_grows_once_and_twice(api, monkeypatch):
    assert check_png_to_webp_grows(api, monkeypatch) == [1, 2, 2]


def check_png_with_alpha_grows(api, monkeypatch):
    """a PNG with transparency -> VP8X / ALPH / VP8: the colour samples' frame is the oracle's, the alpha comes back exactly (test_png_webp_emul.check_alpha), and the
    frame went through the growths its size asks for"""
    import test_png_webp_emul as PW
    from _util import png_expand8
    from oracle import oracle as O
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=4)
    src = busy_rgba_png()
    pix, _ = png_expand8(O.png_decode(src))
    seen = []
    for q, expect in ((85, 1), (100, 2)):
        check_growths(("alpha", q), O.webp_encode_rgb(np.ascontiguousarray(pix[:, :, :3]), q), 130, expect)
        api.last_pool_retries()
        PW.check_alpha(api, f"busy_rgba q{q}", src, q)
        seen.append(api.last_pool_retries())
    return seen


def test_png_with_alpha_grows_once_and_twice(api, monkeypatch):
    assert check_png_with_alpha_grows(api, monkeypatch) == [1, 2]


def check_webp_to_webp_grows(api, monkeypatch):
    """a WebP file coded again at webp.quality (cs_batch_compress): decoded on the device, the RGB through the same encoder"""
    from oracle import oracle as O
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=4)
    src = busy_webp()
    rgb = libwebp_rgb(src)
    seen = []
    for q, expect in ((85, 1), (100, 2)):
        want = O.webp_encode_rgb(rgb, q)
        check_growths(("webp", q), want, 130, expect)
        api.last_pool_retries()
        assert api.cs_batch_compress([src], params(webp_quality=q)) == [want], q
        seen.append(api.last_pool_retries())
    return seen


def test_webp_to_webp_grows_once_and_twice(api, monkeypatch):
    assert check_webp_to_webp_grows(api, monkeypatch) == [1, 2]


# ------------------------------------------------------------------------------------------------ mixed batches
def codes(outs):
    return [getattr(o, "code", 0) if isinstance(o, Exception) else 0 for o in outs]


def damaged_jpeg():
    """the first file of test_pipeline_emul.fuzzed_blobs that the oracle refuses"""
    from test_pipeline_emul import fuzzed_blobs
    for blob in fuzzed_blobs(11, 24, True):
        try:
            oracle_lossy(blob)
        except Exception:   # noqa: BLE001 - that is the one
            return blob
    raise AssertionError("no damaged file in the set")


def check_mixed_jpeg_batch(api, monkeypatch):
    """one call: a picture that fits the first reservation, one that needs a growth, one that needs two, junk, a damaged JPEG.  The good files are the oracle's, the
    failures carry the codes they carry without the hook, and the same batch object run again gives the same with no retry.  (Both failures are the host's: the
    JPEG decoder on the device refuses nothing, it decodes what libjpeg decodes.  A failure that lives in the status words, which are zeroed in front of every
    attempt, is in check_mixed_png_batch)"""
    q = 100
    srcs = [flat_jpeg(), mid_jpeg(), busy_jpeg(), b"junk", damaged_jpeg()]
    want = [oracle_jpeg_to_webp(s, q) for s in srcs[:3]]
    assert len(want[0]) < 4096
    check_growths("mid", want[1], 60, 1)
    check_growths("busy", want[2], 130, 2)
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=None)
    plain = api.batch_convert(srcs, params(webp_quality=q), WEBP)
    assert plain[:3] == want and codes(plain)[:3] == [0, 0, 0] and codes(plain)[3] == 10200 and codes(plain)[4] != 0
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=4)
    b = api.webp_batch(srcs, params(webp_quality=q))
    try:
        t = b.run()
        outs = b.fetch()
        assert outs[:3] == want and codes(outs) == codes(plain)
        assert t.n_pool_retries == 2, t.n_pool_retries
        t2 = b.run()
        again = b.fetch()
        assert again[:3] == want and codes(again) == codes(plain) and t2.n_pool_retries == 0
    finally:
        b.close()
    return int(t.n_pool_retries)


def test_mixed_jpeg_batch_keeps_files_and_failures(api, monkeypatch):
    assert check_mixed_jpeg_batch(api, monkeypatch) == 2


def damaged_pngs():
    """test_png_emul's injured files; check_mixed_png_batch picks the ones whose injury only the device's inflate sees (the chunk walk accepts them, their status
    word says malformed)"""
    from test_png_emul import damaged_pngs as make
    return make(23, 40)


def check_mixed_png_batch(api, monkeypatch):
    """the PNG batch keeps the decode's status words apart from the encoder's (zeroed in front of every attempt): a PNG whose stream the device refuses keeps its code
    through the growths the others need"""
    from oracle import oracle as O
    q = 100
    good = [save(synth_rgb(3, 64, 48), "RGB", "PNG"), save(busy_rgb(), "RGB", "PNG")]
    want = [O.png_to_webp(s, q) for s in good]
    assert len(want[0]) < 4096
    check_growths("busy png", want[1], 130, 2)
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=None)
    pool = damaged_pngs()
    first = api.batch_convert(pool, params(webp_quality=q), WEBP)
    bad = [s for s, o in zip(pool, first) if isinstance(o, Exception) and "malformed PNG data" in str(o)][:2]
    assert bad, "no damaged PNG that fails on the device"
    srcs = [good[0], bad[0], good[1], b"junk"] + bad[1:]
    plain = api.batch_convert(srcs, params(webp_quality=q), WEBP)
    assert plain[0] == want[0] and plain[2] == want[1] and codes(plain)[1] != 0 and codes(plain)[3] == 10200
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=4)
    api.last_pool_retries()
    outs = api.batch_convert(srcs, params(webp_quality=q), WEBP)
    n = api.last_pool_retries()
    assert outs[0] == want[0] and outs[2] == want[1] and codes(outs) == codes(plain)
    assert [str(o) for o in outs if isinstance(o, Exception)] == [str(o) for o in plain if isinstance(o, Exception)]
    assert n == 2, n
    return n


def test_mixed_png_batch_keeps_files_and_failures(api, monkeypatch):
    assert check_mixed_png_batch(api, monkeypatch) == 2


# ------------------------------------------------------------------------------------------------ exhaustion
def check_exhaustion(api, monkeypatch):
    """shift 16: the reservation starts at 0 bytes a macroblock and four times nothing is nothing, so a file above the flat 4096 + 2 x macroblocks bytes never fits.
    It fails ALONE with CS_ERR_POOL_OVERFLOW after the three retries: every WebP file has a region of its own, so the small files beside it are whole in every
    attempt and come back as the oracle's (no group is tried again in halves for this: the batch itself answers per file).  A later call without the hook is as ever"""
    from oracle import oracle as O
    q = 85
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=16)
    small, large = flat_jpeg(), busy_jpeg()
    ws, wl = oracle_jpeg_to_webp(small, q), oracle_jpeg_to_webp(large, q)
    assert len(ws) < 4096 + 2 * 12 and len(wl) > 4096 + 2 * 130
    api.last_pool_retries()
    outs = api.batch_convert([small, large, small], params(webp_quality=q), WEBP)
    assert outs[0] == ws and outs[2] == ws and codes(outs) == [0, POOL_OVERFLOW, 0], outs[1]
    assert api.last_pool_retries() == 3
    # PNG sources: the PNG batch's own loop
    psmall, plarge = save(synth_rgb(3, 64, 48), "RGB", "PNG"), save(busy_rgb(), "RGB", "PNG")
    pws, pwl = O.png_to_webp(psmall, q), O.png_to_webp(plarge, q)
    assert len(pws) < 4096 + 2 * 12 and len(pwl) > 4096 + 2 * 130
    outs = api.batch_convert([psmall, plarge, psmall], params(webp_quality=q), WEBP)
    assert outs[0] == pws and outs[2] == pws and codes(outs) == [0, POOL_OVERFLOW, 0], outs[1]
    assert api.last_pool_retries() == 3
    # WebP sources: the decoded pictures go through the JPEG batch object's WebP tail
    wsmall, wlarge = save(synth_rgb(3, 64, 48), "RGB", "WEBP", quality=90), busy_webp()
    wws, wwl = O.webp_encode_rgb(libwebp_rgb(wsmall), q), O.webp_encode_rgb(libwebp_rgb(wlarge), q)
    assert len(wws) < 4096 + 2 * 12 and len(wwl) > 4096 + 2 * 130
    outs = api.cs_batch_compress([wsmall, wlarge, wsmall], params(webp_quality=q))
    assert outs[0] == wws and outs[2] == wws and codes(outs) == [0, POOL_OVERFLOW, 0], outs[1]
    assert api.last_pool_retries() == 3
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=None)
    assert api.batch_convert([small, large, small], params(webp_quality=q), WEBP) == [ws, wl, ws]
    assert api.batch_convert([plarge], params(webp_quality=q), WEBP) == [pwl]
    assert api.last_pool_retries() == 0


def test_exhaustion_fails_the_large_file_alone(api, monkeypatch):
    check_exhaustion(api, monkeypatch)


# ------------------------------------------------------------------------------------------------ the boolean coder in pieces under overflow
def check_bool_pieces_under_overflow(api, monkeypatch):
    """CSH_TEST_BOOL_SEG: pieces of 3 and of 61 decisions.  A piece that completes no byte runs out of room at its first one: the 0xff bytes it held back overflow in
    settle(), not in emit()"""
    src, mid = busy_jpeg(), mid_jpeg()
    seen = []
    for seg in ("3", "61"):
        set_env(monkeypatch, CSH_TEST_POOL_SHIFT=4, CSH_TEST_BOOL_SEG=seg)
        for q, expect in ((85, 1), (100, 2)):
            want = [oracle_jpeg_to_webp(src, q), oracle_jpeg_to_webp(mid, q)]
            check_growths(("busy", q), want[0], 130, expect)
            b = api.webp_batch([src, mid], params(webp_quality=q))
            try:
                t = b.run()
                assert b.fetch() == want, (seg, q)
            finally:
                b.close()
            assert t.n_pool_retries == expect, (seg, q, t.n_pool_retries)
            seen.append(int(t.n_pool_retries))
    set_env(monkeypatch, CSH_TEST_BOOL_SEG=None)
    return seen


def test_boolean_coder_in_pieces_under_overflow(api, monkeypatch):
    assert check_bool_pieces_under_overflow(api, monkeypatch) == [1, 2, 1, 2]


# ------------------------------------------------------------------------------------------------ the JPEG raw-scan / output pool: a natural trigger, no hook
def raw_pool_bytes(srcs, profile):
    """what the batch reserves for its scans and files: per file 2 x input + 64 KiB, 8 x input + 256 KiB where the scan search's candidates need room (batch_plan.cpp)"""
    return sum((2 * len(s) + 64 * 1024) if profile == "plain" else (8 * len(s) + 256 * 1024) for s in srcs)


def check_raw_pool(api, monkeypatch, profile, width, subsampling=2, beside=True):
    """a noise JPEG of 64 x 48 enlarged to `width` at quality 100, beside a flat file that stays small: the enlarged file alone is larger than the whole pool (asserted
    from the oracle's size), so the batch has to run again.  -> the retries seen"""
    set_env(monkeypatch, CSH_PROFILE=profile, CSH_TEST_POOL_SHIFT=None)
    srcs = [noise_jpeg_64x48(subsampling)] + ([small_jpeg()] if beside else [])
    want = [oracle_resized(s, width, 0, quality=100) for s in srcs]
    assert len(want[0]) > raw_pool_bytes(srcs, profile), (len(want[0]), raw_pool_bytes(srcs, profile))
    assert not beside or len(want[1]) < 64 * 1024
    b = api.batch(srcs, params(jpeg_quality=100, width=width))
    try:
        t = b.run()
        outs = b.fetch()
    finally:
        b.close()
    assert outs[0] == want[0], (profile, width)
    assert outs[1:] == want[1:], (profile, width)
    assert t.n_pool_retries >= 1, t.n_pool_retries
    return int(t.n_pool_retries)


def test_jpeg_raw_pool_grows_default_profile(api, monkeypatch):
    """2400 x 1800 from 64 x 48, 794 K wanted of a pool of 536 K.  The token / list pools, estimated from the 1.5 KB input, are too small as well and the run needs
    all three retries; every retry makes the raw pool four times larger too, and the token pools' overflow cuts the scans of the early attempts short -- with this
    4:2:0 source the raw pool is never the one that reports (CSH_TRACE names the pools of every attempt)"""
    assert check_raw_pool(api, monkeypatch, None, 2400) >= 1


def test_jpeg_raw_pool_reports_for_itself(api, monkeypatch):
    """the same from a 4:4:4 source (2.3 KB, 1.18 MB out): the first attempt fills the raw pool as well -- k_scan_place reports it and the packers leave the scans
    without room alone (k_list_pack, k_list_refine_pack).  All three retries are needed: check_raw_and_token_pools_together rests on that"""
    assert check_raw_pool(api, monkeypatch, None, 2400, subsampling=0, beside=False) == 3


def test_jpeg_raw_pool_grows_plain_profile(api, monkeypatch):
    """CSH_PROFILE=plain reserves 2 x input + 64 KiB a file: 650 wide is the first multiple of 50 at which the enlarged file alone exceeds the two files' pool.  At 2400
    wide from the 4:4:4 source (1.6 MB out, 70 KB reserved) the raw pool itself gives out in every attempt but the last, under k_pack"""
    set_env(monkeypatch, CSH_PROFILE="plain")
    srcs = [noise_jpeg_64x48(), small_jpeg()]
    sizes = {w: len(oracle_resized(srcs[0], w, 0, quality=100)) for w in (600, 650)}
    assert sizes[600] <= raw_pool_bytes(srcs, "plain") < sizes[650], sizes
    assert check_raw_pool(api, monkeypatch, "plain", 650) >= 1
    assert check_raw_pool(api, monkeypatch, "plain", 2400, subsampling=0, beside=False) >= 1


def check_raw_and_token_pools_together(api, monkeypatch):
    """CSH_TEST_POOL_SHIFT=4 on top of the natural trigger (default profile, the 4:4:4 source at 2400 wide: token / list pools and the raw pool report in the same run).
    Without the hook this call needs all three retries -- pools 64 times their estimate (asserted: test_jpeg_raw_pool_reports_for_itself).  With it the pools
    start at a sixteenth and end at 4 times the estimate: they cannot reach what the picture needs, so what the code promises is the clean end, not the file:
    csh_batch_run answers CS_ERR_POOL_OVERFLOW after its three retries, and the batch object is still good for its destroy"""
    set_env(monkeypatch, CSH_PROFILE=None, CSH_TEST_POOL_SHIFT=4)
    src = noise_jpeg_64x48(0)
    assert len(oracle_resized(src, 2400, 0, quality=100)) > raw_pool_bytes([src], None)
    api.last_pool_retries()
    b = api.batch([src], params(jpeg_quality=100, width=2400))
    try:
        with pytest.raises(package().CaesiumError) as e:
            b.run()
    finally:
        b.close()
    assert e.value.code == POOL_OVERFLOW
    assert api.last_pool_retries() == 3


def test_jpeg_raw_pool_and_token_pools_overflow_together(api, monkeypatch):
    check_raw_and_token_pools_together(api, monkeypatch)


def check_jpeg_exhaustion_halves_the_group(api, monkeypatch):
    """the JPEG coder's pools are the batch's, not a file's: a group that exhausts its retries fails as a whole and the route tries the same files again in halves
    (route_jpeg.cpp; csh_device_count() is 1 in the emulation too).  Shift 4 and the enlarged noise file between two flat ones: the noise file alone comes back as
    CS_ERR_POOL_OVERFLOW, the flat files are the oracle's; the same call without the hook gives all three"""
    set_env(monkeypatch, CSH_PROFILE=None, CSH_TEST_POOL_SHIFT=4)
    srcs = [small_jpeg(), noise_jpeg_64x48(), small_jpeg()]
    want = [oracle_resized(s, 600, 0, quality=100) for s in srcs]
    outs = api.cs_batch_compress(srcs, params(jpeg_quality=100, width=600))
    assert codes(outs) == [0, POOL_OVERFLOW, 0] and outs[0] == want[0] and outs[2] == want[2]
    set_env(monkeypatch, CSH_TEST_POOL_SHIFT=None)
    assert api.cs_batch_compress(srcs, params(jpeg_quality=100, width=600)) == want


def test_jpeg_exhaustion_halves_the_group(api, monkeypatch):
    check_jpeg_exhaustion_halves_the_group(api, monkeypatch)


def check_size_walk(api, monkeypatch):
    """size targeting on the enlarged file (1200 wide, default profile): libcaesium's walk starts at quality 80 and climbs to 100 for a target of the quality-100
    file's size -- 80, 90, 95, 98, 99, 100.  The result is reference_size_walk's.  Which tries grow the pools is read from the same walk made by hand on a batch
    object that retains its DCT (it is printed): the first try already grows them, twice (the token / list pools are estimated from the 1.5 KB input, whatever the
    quality), so no target puts a fitting try in front of an overflowing one; 90, 95 and 98 fit what the first try left, the re-run at 99 grows the pools once
    more, and 100 fits again -- retries per try 2, 0, 0, 0, 1, 0.  The re-runs start from the decoded coefficients (the profile derings), and every one is the
    oracle's file at its quality: the retained state survives the retries"""
    from test_pipeline_emul import reference_size_walk
    set_env(monkeypatch, CSH_PROFILE=None, CSH_TEST_POOL_SHIFT=None)
    src, width = noise_jpeg_64x48(), 1200
    top = oracle_resized(src, width, 0, quality=100)
    assert len(top) > raw_pool_bytes([src], None) > len(oracle_resized(src, width, 0, quality=80))
    target = len(top) + 1
    seq, want = reference_size_walk(src, target, encode=lambda s, q: oracle_resized(s, width, 0, quality=q))
    assert seq[0] == 80 and seq[-1] == 100 and want == top
    api.last_pool_retries()
    assert api.batch_compress_to_size([src], params(width=width), target) == [want]
    total = api.last_pool_retries()
    assert total >= 1
    b = api.batch([src], params(jpeg_quality=80, width=width))
    grew = []
    try:
        b.retain_dct()
        for k, q in enumerate(seq):
            if k: b.set_quality([q])
            t = b.rerun_encode() if k else b.run()
            assert b.fetch() == [oracle_resized(src, width, 0, quality=q)], q
            grew.append(int(t.n_pool_retries))
    finally:
        b.close()
    assert sum(grew) == total and sum(grew) >= 1, (grew, total)
    print("size walk", seq, "retries per try", grew)
    return seq, grew


def test_size_walk_over_a_growing_pool(api, monkeypatch):
    check_size_walk(api, monkeypatch)


# ------------------------------------------------------------------------------------------------ back to front (the emulation only)
def test_back_to_front(api, monkeypatch):
    """every launch's workgroups in reverse order (test_order_emul.py): no retry may lean on the order in which the first attempt's workgroups gave up"""
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    api.L.csh_emul_set_reverse(1)
    try:
        assert check_jpeg_to_webp_grows(api, monkeypatch) == [1, 2]
        assert check_raw_pool(api, monkeypatch, None, 2400) >= 1
    finally:
        api.L.csh_emul_set_reverse(0)


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_and_binding_agree_on_the_timing_structs(api):
    """n_pool_retries is the LAST member of csh_timing and of csp_timing (no earlier offset moved), the binding's structures list the header's members in the
    header's order, and both libraries export the last-call reader"""
    hdr = open(os.path.join(ROOT, "include", "caesium_hip.h")).read()
    B = package().binding

    def members(struct):
        body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + struct + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                out += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
        return out
    for struct, cls in (("csh_timing", B.Timing), ("csp_timing", B.PngTiming)):
        names = members(struct)
        assert names == [f[0] for f in cls._fields_], struct
        assert names[-1] == "n_pool_retries"
    assert ctypes.sizeof(B.Timing) == 304 and ctypes.sizeof(B.PngTiming) == 120   # csp_timing: the new word took the struct's tail padding
    assert "csh_last_pool_retries" in B.EXPORTS and "uint32_t csh_last_pool_retries(void);" in hdr
    for lib in (api.L, ctypes.CDLL(package().library_path())):
        assert hasattr(lib, "csh_last_pool_retries")
    api.last_pool_retries()
    assert api.last_pool_retries() == 0   # read and reset
