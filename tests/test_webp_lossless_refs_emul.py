"""Lossless WebP OUTPUT with backward references and a colour cache (CSH_VP8L=refs, k_vp8l_refs.hip).  Like the plain coder its bytes are this
project's own; what is pinned is the format's invariant, judged by libwebp (through Pillow): the file decodes to EXACTLY the pixels that went in -- and this
repo's decoder and the independent reader tests/_vp8l_parse.py agree.  On top of that: the stream really uses the tools, it is never larger than the plain
coder's, and the default (CSH_VP8L unset or "plain") stays the oracle's bytes.  The functions take the library as an argument: tests/
test_zzz_webp_lossless_refs_gpu.py runs them on the MI355X."""
import contextlib
import functools
import io
import json
import os
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageDraw

import _vp8l_parse as V
import test_webp_decode_emul as D
import test_webp_lossless_emul as E
from _util import ROOT, emul_api, png_cases
from gen_synth import synth_jpeg, synth_rgb

WINDOW = (1 << 20) - 120
MAX_LEN = 4096
CHUNK = 4096   # positions per wave in the parse (webp_kernels.h VP8L_CHUNK)
EMUL_CLI = os.path.join(ROOT, "tests", "emul", "caesiumclt_emul")


@pytest.fixture(scope="module")
def api():
    return emul_api()


@contextlib.contextmanager
def vp8l_mode(mode):
    """CSH_VP8L for the calls inside (None: unset); csl_encode_pixels reads it on every call"""
    old = os.environ.get("CSH_VP8L")
    if mode is None:
        os.environ.pop("CSH_VP8L", None)
    else:
        os.environ["CSH_VP8L"] = mode
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("CSH_VP8L", None)
        else:
            os.environ["CSH_VP8L"] = old


# ---------------------------------------------------------------------------------------------------- the pictures
def alpha_plane(w=320, h=240):
    a = np.full((h, w), 255, np.uint8)
    a[40:120, 30:150] = 0
    a[100:200, 180:300] = 128
    return a


def table_pictures():
    """the nine pictures of the size table; 320 x 240 except where the name says otherwise"""
    x, y = np.arange(320)[None, :], np.arange(240)[:, None]
    rects = Image.new("RGB", (320, 240), (250, 250, 250))
    d, rng = ImageDraw.Draw(rects), np.random.default_rng(16)
    colours = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(15)]   # and the background: 16
    for k in range(40):
        x0, y0 = int(rng.integers(0, 300)), int(rng.integers(0, 220))
        d.rectangle([x0, y0, x0 + int(rng.integers(5, 90)), y0 + int(rng.integers(5, 70))], fill=colours[k % 15])
    tile = np.random.default_rng(1).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    a = alpha_plane()
    return [("texture20", synth_rgb(31, 320, 240, texture=20.0)), ("texture5", synth_rgb(31, 320, 240, texture=5.0)), ("texture0", synth_rgb(31, 320, 240, texture=0.0)),
            ("texture0_640x480", synth_rgb(7, 640, 480, texture=0.0)),
            ("gradient", np.dstack([(x * 255 // 319) + 0 * y, (y * 255 // 239) + 0 * x, (x + y) * 255 // 558]).astype(np.uint8)),
            ("rectangles16", np.asarray(rects)), ("tiled16x16", np.tile(tile, (15, 20, 1))), ("flat", np.full((240, 320, 3), 77, np.uint8)),
            ("alpha_plane_as_grey", np.dstack([a, a, a]))]


GRAPHIC = ["gradient", "rectangles16", "tiled16x16", "flat", "alpha_plane_as_grey"]   # backward references must show here
TENFOLD = ["flat", "tiled16x16", "alpha_plane_as_grey"]                              # refs <= plain / 10: see test_emul_refs_sizes


@functools.lru_cache(maxsize=None)
def battery():
    """(name, lossless WebP source) -- the pixels that go into the coder are what libwebp reads from the source"""
    out = [("source%d" % i, s) for i, s in enumerate(E.sources())]
    out.append(("w0.webp", open(os.path.join(ROOT, "tests", "golden", "reference_samples", "w0.webp"), "rb").read()))
    out += [(n, D.lossless_of(a)) for n, a in table_pictures()]
    rgb = synth_rgb(3, 120, 90, texture=4.0)
    a = alpha_plane(120, 90)
    out.append(("rgba", D.lossless_of(np.dstack([rgb, a]), "RGBA", exact=True)))
    out.append(("grey_alpha", D.lossless_of(np.dstack([rgb[:, :, :1]] * 3 + [a]), "RGBA", exact=True)))
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 256, (3, 13000, 3), dtype=np.uint8)
    wide[1] = (9, 200, 31)                                  # a flat row of 13000 pixels holds whole chunks of the parse: their copies are at the length cap
    out.append(("wide_flat_row", D.lossless_of(wide)))
    far = rng.integers(0, 256, (1040, 1024, 3), dtype=np.uint8)
    far[-8:] = far[:8]                                      # the only repetition lies 1032 rows = 1 056 768 pixels back: beyond the window
    out.append(("far_repeat", D.lossless_of(far)))
    t = rng.integers(0, 256, (7, 12, 3), dtype=np.uint8)    # a 12 x 7 tile at width 300: its copies (distance 12, then 2100) run across every multiple of CHUNK
    out.append(("straddle", D.lossless_of(np.tile(t, (20, 25, 1)))))
    return tuple(out)


def want_pixels(src):
    im = Image.open(io.BytesIO(src))
    return np.asarray(im.convert("RGBA" if im.mode == "RGBA" else "RGB"))


@functools.lru_cache(maxsize=None)
def coded(api_key, mode):
    api = _APIS[api_key]
    with vp8l_mode(mode):
        outs = api.cs_batch_compress([s for _, s in battery()], E.params(webp_lossless=True))
    for (name, _), o in zip(battery(), outs):
        assert isinstance(o, bytes), (name, o)
    return tuple(outs)


_APIS = {}


def outputs(api, mode):
    _APIS[id(api)] = api
    return coded(id(api), mode)


@functools.lru_cache(maxsize=None)
def parsed(blob):
    return V.parse(blob)


def check_file(blob, want, name=""):
    """RIFF framing as E.check_vp8l checks it, and libwebp's reading of the file"""
    assert blob[:4] == b"RIFF" and blob[8:16] == b"WEBPVP8L" and int.from_bytes(blob[4:8], "little") == len(blob) - 8 and len(blob) % 2 == 0, name
    im = Image.open(io.BytesIO(blob))
    got = np.asarray(im.convert("RGBA" if want.shape[2] == 4 else "RGB"))
    assert got.shape == want.shape and np.array_equal(got, want), name


def check_tools(blob, want, name=""):
    st = parsed(blob)
    for length, dist, pos in st.refs:
        assert 1 <= dist <= pos and dist <= WINDOW and 1 <= length <= MAX_LEN, (name, length, dist, pos)
    rgba = V.rgba_of(st.argb)
    assert np.array_equal(rgba if want.shape[2] == 4 else rgba[:, :, :3], want), name
    return st


# ---------------------------------------------------------------------------------------------------- the checks
def test_the_reader_reads_libwebps_own_files():
    """tests/_vp8l_parse.py against libwebp's coder, which uses every tool of the format: the reader is independent of this repository's code"""
    for name, arr in table_pictures()[2:6]:
        st = V.parse(D.lossless_of(arr))
        assert np.array_equal(V.rgba_of(st.argb)[:, :, :3], arr), name
    st = V.parse(D.lossless_of(table_pictures()[5][1]))
    assert st.refs and all(d <= p for _, d, p in st.refs)


def run_round_trip(api):
    outs = outputs(api, "refs")
    for (name, src), out in zip(battery(), outs):
        check_file(out, want_pixels(src), name)
    for (name, src), got in zip(battery(), api.webp_decode(list(outs))):   # and this repo's own decoder
        want = want_pixels(src)
        assert not isinstance(got, Exception), (name, got)
        assert np.array_equal(got if got.shape[2] == want.shape[2] else got[:, :, :3], want if got.shape[2] == want.shape[2] else want[:, :, :3]), name


def test_emul_refs_round_trips_through_libwebp(api):
    run_round_trip(api)


def run_tools(api):
    outs = dict(zip([n for n, _ in battery()], outputs(api, "refs")))
    srcs = dict(battery())
    stats = {name: check_tools(outs[name], want_pixels(srcs[name]), name) for name in outs}
    for name in GRAPHIC:
        assert stats[name].refs, name
    st = stats["rectangles16"]
    assert st.cache_bits > 0 and st.cache_hits > 0
    assert max(l for l, _, _ in stats["wide_flat_row"].refs) == MAX_LEN            # the flat row reaches the cap
    assert all(d <= WINDOW for _, d, _ in stats["far_repeat"].refs)
    reach = {(p + l - 1) // CHUNK for l, d, p in stats["straddle"].refs if p - d < (p // CHUNK) * CHUNK}   # copies whose source starts in front of their chunk
    assert reach >= set(range(1, (300 * 140 - 1) // CHUNK + 1)), sorted(reach)
    # without the feature (the variable ignored) none of this holds
    plain = parsed(outputs(api, None)[[n for n, _ in battery()].index("flat")])
    assert not plain.refs and plain.cache_bits == 0


def test_emul_refs_stream_uses_the_tools(api):
    run_tools(api)


def libwebp_size(src):
    b = io.BytesIO()
    Image.open(io.BytesIO(src)).save(b, "WEBP", lossless=True, quality=75, method=4)   # what crate webp 0.3.1 asks of libwebp
    return len(b.getvalue())


def size_table(api):
    rows = []
    for (name, src), r, p in zip(battery(), outputs(api, "refs"), outputs(api, None)):
        lw = libwebp_size(src)
        rows.append((name, len(p), len(r), lw, len(p) / lw, len(r) / lw))
    return rows


def run_sizes(api):
    rows = size_table(api)
    for name, p, r, lw, pl, rl in rows:
        print("%-22s plain %8d  refs %8d  libwebp %8d  plain/libwebp %7.2f  refs/libwebp %7.2f" % (name, p, r, lw, pl, rl))
    for name, p, r, lw, pl, rl in rows:
        assert r <= p, name                                  # the fallback rule
    # the flat and alpha pictures need 76 800 / 4096 = 19 copies plus headers against 9.6 KB, the tiled one its first tile row's literals, a few dozen copies
    # and the code descriptions against 207 KB
    for name, p, r, lw, pl, rl in rows:
        if name in TENFOLD:
            assert r * 10 <= p, (name, p, r)


def test_emul_refs_sizes(api, capsys):
    with capsys.disabled():
        run_sizes(api)


def run_default_untouched(api):
    unset, plain = outputs(api, None), outputs(api, "plain")
    assert unset == plain
    for (name, src), out in list(zip(battery(), unset))[:20]:
        assert out == E.oracle_vp8l(out), name
    with vp8l_mode(""):
        assert api.compress_in_memory(battery()[0][1], E.params(webp_lossless=True)) == unset[0]
    with vp8l_mode("lz77"):
        outs = api.cs_batch_compress([battery()[0][1], battery()[1][1]], E.params(webp_lossless=True))
    for o in outs:
        assert isinstance(o, Exception) and o.code == 10201 and "CSH_VP8L" in str(o), o   # CS_ERR_UNSUPPORTED, per file
    assert outputs(api, "refs")[:3] != unset[:3]


def test_emul_default_is_untouched_and_unknown_values_fail(api):
    run_default_untouched(api)


def run_conversions(api):
    cases = dict(png_cases())
    names = ["RGB_97x61", "L_97x61", "P_97x61", "RGB_flat_64x48", "RGB_200x150_3chunks", "RGBA_97x61", "LA_97x61", "RGBA_300x2"]
    p = E.params(webp_lossless=True)
    with vp8l_mode("refs"):
        refs = api.batch_convert([cases[n] for n in names], p, 3)
        j = synth_jpeg(4, 120, 88, texture=30)
        jr = [api.convert_in_memory(j, p, 3), api.convert_in_memory(j, E.params(webp_lossless=True, width=60), 3)]
    with vp8l_mode(None):
        plain = api.batch_convert([cases[n] for n in names], p, 3)
        jp = [api.convert_in_memory(j, p, 3), api.convert_in_memory(j, E.params(webp_lossless=True, width=60), 3)]
    for name, r, pl in zip(names, refs, plain):
        assert isinstance(r, bytes) and isinstance(pl, bytes), (name, r, pl)
        im = Image.open(io.BytesIO(cases[name]))
        alpha = im.mode in ("RGBA", "LA")
        want = np.asarray(im.convert("RGBA" if alpha else "RGB"))
        check_file(r, want, name)
        check_tools(r, want, name)
        assert len(r) <= len(pl), name
    for r, pl in zip(jr, jp):
        want = np.asarray(Image.open(io.BytesIO(pl)).convert("RGB"))   # the plain file's pixels are the oracle's (tests/test_webp_lossless_emul.py)
        check_file(r, want)
        assert len(r) <= len(pl)
    assert Image.open(io.BytesIO(jr[1])).size[0] == 60


def test_emul_refs_conversions_from_png_and_jpeg(api):
    run_conversions(api)


def chunks_of(blob):
    assert blob[:4] == b"RIFF" and blob[8:12] == b"WEBP"
    out, pos = [], 12
    while pos + 8 <= len(blob):
        n = int.from_bytes(blob[pos + 4:pos + 8], "little")
        out.append((blob[pos:pos + 4], blob[pos + 8:pos + 8 + n]))
        pos += 8 + n + (n & 1)
    return out


def run_alph(api):
    def png_of(arr):
        b = io.BytesIO()
        Image.fromarray(arr, "RGBA").save(b, "PNG")
        return b.getvalue()
    big = np.dstack([synth_rgb(12, 320, 240, texture=6.0), alpha_plane()])
    srcs = [dict(png_cases())["RGBA_97x61"], png_of(big)]
    p = E.params(webp_quality=70)
    with vp8l_mode("refs"):
        refs = api.batch_convert(srcs, p, 3)
    with vp8l_mode(None):
        plain = api.batch_convert(srcs, p, 3)
    for k, (src, r, pl) in enumerate(zip(srcs, refs, plain)):
        assert isinstance(r, bytes) and isinstance(pl, bytes), (r, pl)
        cr, cp = chunks_of(r), chunks_of(pl)
        assert [c[0] for c in cr] == [b"VP8X", b"ALPH", b"VP8 "] == [c[0] for c in cp]
        assert cr[2][1] == cp[2][1]                                   # the colour frame does not know about the switch
        assert len(cr[1][1]) <= len(cp[1][1])
        alpha = np.asarray(Image.open(io.BytesIO(src)).convert("RGBA"))[:, :, 3]
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(r)).convert("RGBA"))[:, :, 3], alpha)
        st = V.parse(cr[1][1][1:], headerless=(alpha.shape[1], alpha.shape[0]))   # behind the chunk's header byte: a VP8L stream without its five header bytes
        assert np.array_equal((st.argb >> 8) & 255, alpha)
        if k == 1:
            assert st.refs and len(cr[1][1]) * 10 <= len(cp[1][1]), (len(cr[1][1]), len(cp[1][1]))


def test_emul_refs_alph_chunk(api):
    run_alph(api)


def run_cli(binary, tmp_path):
    """caesiumclt --lossless over WebP files and --format webp --lossless over PNG files, CSH_VP8L=refs in the environment"""
    wd, pd = tmp_path / "webps", tmp_path / "pngs"
    wd.mkdir(); pd.mkdir()
    pics = dict(table_pictures())
    for name in ("texture5", "rectangles16", "flat"):
        (wd / (name + ".webp")).write_bytes(D.lossless_of(pics[name]))
        Image.fromarray(pics[name]).save(pd / (name + ".png"))
    Image.fromarray(np.dstack([pics["gradient"], alpha_plane()]), "RGBA").save(pd / "rgba.png")
    got = {}
    for mode in ("refs", "plain"):
        env = dict(os.environ, CSH_VP8L=mode)
        for tag, args in (("w", ["--lossless", wd]), ("p", ["--lossless", "--format", "webp", pd])):
            r = subprocess.run([binary, *map(str, args), "-o", str(tmp_path / (tag + mode)), "--json"], capture_output=True, text=True, env=env)
            j = json.loads(r.stdout)
            assert [f["status"] for f in j["files"]] == ["success"] * len(j["files"]) and j["files"], r.stdout
            for f in j["files"]:
                got[(mode, tag, os.path.basename(f["original_path"]))] = open(f["output_path"], "rb").read()
    n = 0
    for (mode, tag, name), blob in got.items():
        if mode != "refs":
            continue
        src = Image.open((wd if tag == "w" else pd) / name)
        want = np.asarray(src.convert("RGBA" if src.mode == "RGBA" else "RGB"))
        check_file(blob, want, name)
        assert len(blob) <= len(got[("plain", tag, name)]), name
        n += 1
    assert n == 7
    assert got[("refs", "w", "flat.webp")] != got[("plain", "w", "flat.webp")]


def test_emul_refs_through_the_cli(api, tmp_path):
    run_cli(EMUL_CLI, tmp_path)


def test_emul_refs_do_not_depend_on_the_order_of_execution(api):
    """the hashed candidate and the cache's contents are defined by position (atomicMax of positions): the emulation run backwards writes the same bytes"""
    import ctypes
    srcs = [s for n, s in battery() if n in ("texture0", "rectangles16", "tiled16x16", "straddle", "rgba")]
    with vp8l_mode("refs"):
        fwd = api.cs_batch_compress(srcs, E.params(webp_lossless=True))
        api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
        api.L.csh_emul_set_reverse(1)
        try:
            rev = api.cs_batch_compress(srcs, E.params(webp_lossless=True))
        finally:
            api.L.csh_emul_set_reverse(0)
    assert fwd == rev
