"""The Lanczos3 resize kernels against the float64 model of image-rs (tests/_lanczos_model.py), read through outputs that keep the resized
samples exactly: JPEG -> PNG and PNG -> PNG lossless (k_planes_to_rgb + k_lanczos_*, k_png_lanczos_*), and lossless WebP from PNG sources
(the pixel-source JPEG batch).  Every output sample must pass the acceptance rule of _lanczos_model.check, and every file must still equal
the oracle's byte for byte.  Kernel sources compiled for the CPU; test_zzz_resize_model_gpu.py runs the same cases on the device.

The battery asserts its own edges: source rows at each side of every LDS cap (k_resize.hip CSH_RZ_CAP_S / _L, k_png_resize.hip
CSP_RZ_CAP), row lengths of each residue mod 4, the two-pass kernels both forced (CSH_RESIZE_TWO_PASS) and chosen by a wide row, a batch
of one wide picture and small ones, extreme ratios and identity on one axis or both.

Not pinned: how image-rs treats alpha (resampled here like any channel, as the oracle does) and libcaesium's exact compute_dimensions."""
import io
import os
from contextlib import contextmanager

import numpy as np
import pytest

import _lanczos_model as M
from _util import emul_api, oracle_jpeg_to_png, oracle_png_resized, package

PIL = pytest.importorskip("PIL.Image")

CAP_S, CAP_L, CAP_PNG = 6144, 16128, 16128   # floats of LDS per source row: k_resize.hip CSH_RZ_CAP_S / CSH_RZ_CAP_L, k_png_resize.hip CSP_RZ_CAP
FMT_PNG, FMT_WEBP = 1, 3


@pytest.fixture(scope="module")
def api():
    return emul_api()


@contextmanager
def two_pass(on=True):
    """CSH_RESIZE_TWO_PASS: the vertical and horizontal kernels with the f32 image between them, whatever the row length"""
    if not on:
        yield
        return
    os.environ["CSH_RESIZE_TWO_PASS"] = "1"
    try:
        yield
    finally:
        del os.environ["CSH_RESIZE_TWO_PASS"]


def pattern(seed, h, w, nc, maxval):
    """noise with hard 0 / M edges: full-height bars, a saturated corner and single-sample spikes, where ringing clamps"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, maxval + 1, (h, w, nc), dtype=np.int64)
    b = max(1, w // 7)
    a[:, w // 3:w // 3 + b] = maxval
    a[:, 2 * w // 3:2 * w // 3 + b] = 0
    a[h // 2:, :max(1, w // 5)] = maxval
    a[::3, ::11] = 0
    return a


def expand_rgba(a, maxval):
    """(h, w, c) -> (h, w, 4): grey repeated, a missing alpha opaque -- the common layout device output and model are compared in"""
    a = np.asarray(a, np.float64)
    c = a.shape[2]
    col = a[:, :, :3] if c >= 3 else np.repeat(a[:, :, :1], 3, axis=2)
    alpha = a[:, :, c - 1:c] if c in (2, 4) else np.full(a.shape[:2] + (1,), float(maxval))
    return np.concatenate([col, alpha], axis=2)


def decode_png(data):
    """a PNG file's samples as they are meant: -> (h, w, c) array, bit depth.  Palette, sub-byte grey and tRNS are expanded (png_expand8);
    16-bit colour keys become a 0 / 65535 alpha"""
    from _util import png_expand8
    from oracle import oracle as O
    P = O.png_decode(data)
    im = P.im
    if im.depth != 16:
        return png_expand8(P)[0].astype(np.int64), 8
    import ctypes as C
    pix = P.rows().view(">u2").astype(np.int64).reshape(im.height, im.width, im.channels)
    chunks, pos = C.string_at(im.chunks, im.chunks_len), 0
    while pos + 12 <= len(chunks):
        ln = int.from_bytes(chunks[pos:pos + 4], "big")
        if chunks[pos + 4:pos + 8] == b"tRNS":
            key = np.frombuffer(chunks[pos + 8:pos + 8 + ln], ">u2").astype(np.int64)
            pix = np.concatenate([pix, np.where((pix == key).all(axis=2), 0, 65535)[:, :, None]], axis=2)
        pos += 12 + ln
    return pix, 16


def check_resized(name, got, depth_got, src, nw, nh, maxval, ties):
    """got (the device's resized samples, any layout the lossless coder chose) against the model of src resized to nw x nh"""
    assert got.shape[:2] == (nh, nw), (name, got.shape, nw, nh)
    if depth_got == 8 and maxval == 65535:
        got = got * 257   # the coder narrowed 16-bit samples whose two bytes are equal
    v, delta = M.resize(src, nw, nh, maxval)
    if (nw, nh) == src.shape[1::-1]:
        assert np.array_equal(expand_rgba(got, maxval), expand_rgba(src, maxval)), name   # unchanged size: a copy
        return
    ties[name] = ties.get(name, 0) + M.assert_rule(expand_rgba(got, maxval), expand_rgba(v, maxval), delta, name)


# ---------------------------------------------------------------- JPEG sources
def jpeg_of(seed, w, h, ss=2, grey=False):
    """a JPEG of a noise-and-edges picture (Pillow subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)"""
    a = pattern(seed, h, w, 1 if grey else 3, 255).astype(np.uint8)
    b = io.BytesIO()
    if grey:
        PIL.fromarray(a[:, :, 0], "L").save(b, "JPEG", quality=90)
    else:
        PIL.fromarray(a, "RGB").save(b, "JPEG", quality=90, subsampling=ss)
    return b.getvalue()


def jpeg_pixels(src):
    """the pre-resize pixels: the oracle's decode and cso_ycc_to_rgb (as _util.oracle_jpeg_to_png; existing tests pin these to the device's
    unresized conversion)"""
    from oracle import oracle as O
    pix = O.decode(src).pixels()
    return (O.ycc_to_rgb(pix) if pix.shape[2] == 3 else pix).astype(np.int64)


def run_jpeg_cases(api, cases, width, height, ties, parity=True):
    """cases: [(name, jpeg)] in one batch_convert to lossless PNG"""
    outs = api.batch_convert([c[1] for c in cases], package().default_parameters(png_optimize=True, png_optimization_level=1, width=width, height=height), FMT_PNG)
    for (name, src), out in zip(cases, outs):
        assert not isinstance(out, Exception), (name, out)
        if parity:
            assert out == oracle_jpeg_to_png(src, True, 1, width, height), name
        pix = jpeg_pixels(src)
        nw, nh = M.compute_dimensions(pix.shape[1], pix.shape[0], width, height)
        got, depth = decode_png(out)
        check_resized(name, got, depth, pix, nw, nh, 255, ties)


def report(ties):
    print("tie band:", ", ".join(f"{k} {v}" for k, v in ties.items()))


# row lengths (samples per source row) around the caps: RGB 2048 / 2049 px (CAP_S), 5376 / 5377 (CAP_L), grey 6144 / 6145, 16128 / 16129
JPEG_CAP_CASES = [("rgb420_2048", 2048, 3, 2), ("rgb422_2049", 2049, 3, 1), ("rgb444_5376", 5376, 3, 0), ("rgb420_5377", 5377, 3, 2),
                  ("grey_6144", 6144, 1, None), ("grey_6145", 6145, 1, None), ("grey_16128", 16128, 1, None), ("grey_16129", 16129, 1, None)]


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
@pytest.mark.parametrize("case", JPEG_CAP_CASES, ids=[c[0] for c in JPEG_CAP_CASES])
def test_jpeg_rows_at_the_lds_caps(api, case, forced):
    name, w, nc, ss = case
    row = w * nc
    assert row in (CAP_S, CAP_S + 1, CAP_S + 3, CAP_L, CAP_L + 1, CAP_L + 3)   # each side of a cap (RGB steps by 3)
    src = jpeg_of(w, w, 6, ss if ss is not None else 2, grey=nc == 1)
    ties = {}
    with two_pass(forced):
        run_jpeg_cases(api, [(name, src)], w * 2 // 3 + 1, 0, ties)   # 6 rows -> 4, and a ratio off the integers
        run_jpeg_cases(api, [(name + "_up_h", src)], w, 11, ties)      # width kept, height enlarged
    report(ties)


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
def test_jpeg_shapes_and_ratios(api, forced):
    """every subsampling and grey, row lengths of each residue mod 4, enlarging and reducing, identity on one axis"""
    cases = []
    for k, (w, ss) in enumerate([(99, 2), (98, 1), (97, 0), (100, 2)]):     # 297, 294, 291, 300 samples a row
        cases.append((f"rgb{['444', '422', '420'][ss]}_{w}", jpeg_of(30 + k, w, 37, ss)))
    for k, w in enumerate([101, 102, 103]):
        cases.append((f"grey_{w}", jpeg_of(40 + k, w, 29, grey=True)))
    assert {(w * 3) % 4 for w in (99, 98, 97)} == {1, 2, 3} and {w % 4 for w in (101, 102, 103)} == {1, 2, 3}
    ties = {}
    with two_pass(forced):
        for (w, h) in [(45, 0), (0, 50), (150, 61), (203, 13)]:
            run_jpeg_cases(api, cases, w, h, ties)
        run_jpeg_cases(api, cases[:1] + cases[4:5], 99, 80, ties)    # width unchanged for rgb_99, changed for grey_101
        run_jpeg_cases(api, cases[:1], 99, 37, ties)                  # both unchanged: the bytes of the source
    report(ties)


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
def test_jpeg_extreme_ratios(api, forced):
    ties = {}
    with two_pass(forced):
        run_jpeg_cases(api, [("rgb_3000x2", jpeg_of(50, 3000, 2))], 1, 1, ties)            # 3000 taps for one output
        run_jpeg_cases(api, [("grey_1x300", jpeg_of(51, 1, 300, grey=True))], 50, 1, ties)
        run_jpeg_cases(api, [("rgb_2x3", jpeg_of(52, 2, 3, ss=0))], 97, 61, ties)           # every output from at most 3 taps
        run_jpeg_cases(api, [("grey_16000x2", jpeg_of(53, 16000, 2, grey=True))], 15999, 1, ties)
    report(ties)


def test_jpeg_batch_of_one_wide_and_small_pictures(api):
    """the fused / two-pass choice is made per batch from its widest row: one RGB row past CAP_L sends the small pictures through the
    two-pass kernels as well, and a row past CAP_S takes every picture to the large fused kernel"""
    ties = {}
    small = [("small_rgb_97", jpeg_of(60, 97, 23, 0)), ("small_grey_31", jpeg_of(61, 31, 40, grey=True)), ("small_rgb_5", jpeg_of(62, 5, 7, 1))]
    run_jpeg_cases(api, [("wide_rgb_5377", jpeg_of(63, 5377, 4))] + small, 64, 0, ties)
    run_jpeg_cases(api, small[:1] + [("wide_rgb_2049", jpeg_of(64, 2049, 4))] + small[1:], 64, 0, ties)
    report(ties)


# ---------------------------------------------------------------- PNG sources
def png_source(seed, w, h, kind):
    """(PNG file, the samples image-rs resamples, M).  kind: L / LA / RGB / RGBA at 8 or 16 bits (L16 ...), L16_trns / RGB16_trns
    (the colour key becomes a 0 / 65535 alpha), P / P_trns (palette looked up), L1 / L2 / L4 (sub-byte grey scaled to 0..255)"""
    from test_png_webp_emul import make_png
    rng = np.random.default_rng(seed)
    base, _, tail = kind.partition("_")
    if base.startswith("P"):
        pal = rng.integers(0, 256, (37, 3)).astype(np.uint8)
        pal[0], pal[1] = 0, 255
        idx = pattern(seed, h, w, 1, 36)[:, :, 0].astype(np.uint8)
        extra = [(b"PLTE", pal.tobytes())]
        pix = pal[idx].astype(np.int64)
        if tail == "trns":
            al = rng.integers(0, 256, 37).astype(np.uint8)
            extra.append((b"tRNS", al.tobytes()))
            pix = np.concatenate([pix, al[idx][:, :, None].astype(np.int64)], axis=2)
        return make_png(w, h, 8, 3, idx.tobytes(), extra), pix, 255
    if base in ("L1", "L2", "L4"):
        d = int(base[1])
        v = pattern(seed, h, w, 1, (1 << d) - 1)[:, :, 0]
        bits = np.unpackbits(v.astype(np.uint8)[:, :, None], axis=2)[:, :, 8 - d:].reshape(h, w * d)
        rows = np.packbits(bits, axis=1)
        return make_png(w, h, d, 0, rows.tobytes()), v[:, :, None] * (255 // ((1 << d) - 1)), 255
    depth = 16 if base.endswith("16") else 8
    mode = base[:-2] if depth == 16 else base
    nc, ctype = {"L": (1, 0), "LA": (2, 4), "RGB": (3, 2), "RGBA": (4, 6)}[mode]
    maxval = (1 << depth) - 1
    pix = pattern(seed, h, w, nc, maxval)
    extra = []
    if tail == "trns":
        key = pix[h // 2, w // 2].copy()
        pix[::2, ::5] = key   # the key hits a fifth of the pixels in every other row
        extra.append((b"tRNS", b"".join(int(k).to_bytes(2, "big") for k in key)))
        alpha = np.where((pix == key).all(axis=2), 0, maxval)
        src_pix = np.concatenate([pix, alpha[:, :, None]], axis=2)
    else:
        src_pix = pix
    raw = pix.astype(">u2" if depth == 16 else np.uint8).tobytes()
    return make_png(w, h, depth, ctype, raw, extra), src_pix, maxval


def run_png_cases(api, cases, width, height, ties, parity=True):
    """cases: [(name, (png, samples, M))] in one lossless PNG batch"""
    outs = api.cs_batch_compress([c[1][0] for c in cases], package().default_parameters(png_optimize=True, png_optimization_level=1, width=width, height=height))
    for (name, (src, pix, maxval)), out in zip(cases, outs):
        assert not isinstance(out, Exception), (name, out)
        if parity:
            assert out == oracle_png_resized(src, True, 1, width, height), name
        nw, nh = M.compute_dimensions(pix.shape[1], pix.shape[0], width, height)
        got, depth = decode_png(out)
        check_resized(name, got, depth, pix, nw, nh, maxval, ties)


PNG_KINDS = ["L", "LA", "RGB", "RGBA", "L16", "LA16", "RGB16", "RGBA16", "L16_trns", "RGB16_trns", "P", "P_trns", "L1", "L2", "L4"]


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
@pytest.mark.parametrize("kind", PNG_KINDS)
def test_png_every_kind_of_sample(api, kind, forced):
    """grey / GA / RGB / RGBA at 8 and 16 bits, 16-bit grey and RGB with a colour key, palette with and without tRNS, 1/2/4-bit grey"""
    cases = [(f"{kind}_{w}x{h}", png_source(70 + w, w, h, kind)) for (w, h) in [(97, 61), (41, 17), (6, 9)]]
    ties = {}
    with two_pass(forced):
        for (w, h) in [(31, 0), (0, 80), (133, 7)]:
            run_png_cases(api, cases, w, h, ties)
        run_png_cases(api, cases[:1], 97, 30, ties)   # width unchanged
    report(ties)


PNG_CAP_CASES = [("RGBA_4032", 4032, "RGBA"), ("RGBA_4033", 4033, "RGBA"), ("L_16128", 16128, "L"), ("L_16129", 16129, "L"),
                 ("RGB16_5376", 5376, "RGB16"), ("RGB16_5377", 5377, "RGB16"), ("LA16_8064", 8064, "LA16"), ("LA16_8065", 8065, "LA16")]


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
@pytest.mark.parametrize("case", PNG_CAP_CASES, ids=[c[0] for c in PNG_CAP_CASES])
def test_png_rows_at_the_lds_cap(api, case, forced):
    name, w, kind = case
    nc = {"RGBA": 4, "L": 1, "RGB16": 3, "LA16": 2}[kind]
    assert w * nc in (CAP_PNG, CAP_PNG + 1, CAP_PNG + 2, CAP_PNG + 3, CAP_PNG + 4)
    ties = {}
    with two_pass(forced):
        run_png_cases(api, [(name, png_source(w, w, 5, kind))], w * 3 // 4 + 1, 0, ties)
    report(ties)


def test_png_extreme_ratios_and_a_mixed_batch(api):
    ties = {}
    run_png_cases(api, [("RGB_3000x2", png_source(80, 3000, 2, "RGB"))], 1, 1, ties)
    run_png_cases(api, [("L16_1x300", png_source(81, 1, 300, "L16"))], 50, 1, ties)
    run_png_cases(api, [("RGBA16_2x3", png_source(82, 2, 3, "RGBA16"))], 97, 61, ties)
    run_png_cases(api, [("L16_16000x2", png_source(83, 16000, 2, "L16"))], 15999, 1, ties)   # f32 positions matter here
    run_png_cases(api, [("RGBA_identity", png_source(84, 40, 30, "RGBA"))], 40, 30, ties)
    # one row past the cap sends the whole batch through the two-pass kernels
    run_png_cases(api, [("small_LA", png_source(85, 33, 21, "LA")), ("wide_RGBA_4033", png_source(86, 4033, 3, "RGBA")),
                        ("small_RGB16", png_source(87, 29, 19, "RGB16")), ("small_P", png_source(88, 17, 40, "P"))], 60, 0, ties)
    report(ties)


# ---------------------------------------------------------------- PNG sources to lossless WebP: the pixel-source JPEG batch (in_kind -1)
def test_png_to_lossless_webp(api):
    """opaque 8-bit PNG sources to lossless WebP go through the JPEG row's resize from pixels (and a transparent one's alpha through it as
    a grey picture); libwebp decodes the result"""
    ties = {}
    cases = [("RGB_97x61", png_source(90, 97, 61, "RGB")), ("L_41x17", png_source(91, 41, 17, "L")), ("RGBA_37x23", png_source(92, 37, 23, "RGBA")),
             ("RGB_2049x40", png_source(93, 2049, 40, "RGB"))]
    for (width, height) in [(50, 0), (0, 90)]:
        outs = api.batch_convert([c[1][0] for c in cases], package().default_parameters(webp_lossless=True, width=width, height=height), FMT_WEBP)
        for (name, (src, pix, maxval)), out in zip(cases, outs):
            assert not isinstance(out, Exception), (name, out)
            nw, nh = M.compute_dimensions(pix.shape[1], pix.shape[0], width, height)
            got = np.asarray(PIL.open(io.BytesIO(out)).convert("RGBA")).astype(np.int64)
            check_resized(f"{name}_{width}x{height}", got, 8, pix, nw, nh, maxval, ties)
    report(ties)
