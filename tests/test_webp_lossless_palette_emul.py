"""Lossless WebP OUTPUT with the colour-indexing transform (CSH_VP8L=palette, k_vp8l_palette.hip): everything CSH_VP8L=refs does, and for a picture
of at most 256 distinct ARGB values one more candidate stream -- the palette, the bundled indices coded by the refs stages -- of which the smallest is written.
Pinned, as for the refs coder: libwebp (Pillow), this repo's decoder and tests/_vp8l_parse.py read exactly the source's pixels; the stream has the transform
where it must and not where it cannot; it is never larger than the refs file and is the refs file where no palette exists; it meets a bound computed from the
source's pixels alone; and unset / plain / refs write the bytes they wrote before (tests/golden/vp8l_refs_digests.json).  The functions take the library:
tests/test_zzz_webp_lossless_palette_gpu.py runs them on the MI355X."""
import functools
import hashlib
import io
import json
import math
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import _vp8l_parse as V
import test_webp_decode_emul as D
import test_webp_lossless_emul as E
import test_webp_lossless_refs_emul as R
from _util import ROOT, emul_api, png_cases
from gen_synth import synth_rgb
from test_webp_lossless_refs_emul import battery as refs_battery, check_file, check_tools, vp8l_mode

CHUNK = R.CHUNK
DIGESTS = os.path.join(ROOT, "tests", "golden", "vp8l_refs_digests.json")


@pytest.fixture(scope="module")
def api():
    return emul_api()


# ---------------------------------------------------------------------------------------------------- the pictures
def dithered(rgb, colours):
    return np.asarray(Image.fromarray(rgb).quantize(colours, dither=Image.Dither.FLOYDSTEINBERG).convert("RGB"))


def distinct_colours(k):
    """k different RGB values, none a neighbour of another in every channel"""
    i = np.arange(k)
    return np.stack([(i * 37) & 255, (i >> 8) * 90 + ((i * 11) & 63), (i * 101 + 7) & 255], axis=1).astype(np.uint8)


def exactly(k, w, h, rng):
    """w x h pixels over exactly k colours, every one of them present"""
    idx = np.concatenate([np.arange(k), rng.integers(0, k, w * h - k)])
    return distinct_colours(k)[rng.permutation(idx).reshape(h, w)]


TWO = np.array([[200, 30, 90], [20, 180, 250]], np.uint8)   # two colours apart in every channel
# The 1 x 1 picture is RGBA, nearly transparent: an OPAQUE 1 x 1 picture can never take the palette.  Its palette stream is at least 109 bits (40 of signature and
# sizes, 11 + 1 + 4 x 4 + 4 + 1 of the transform and its one entry with every channel <= 1, 29 of the index stream, 18 more for alpha 255 as an 8-bit symbol in both)
# and its plain stream at most 107 for such a colour, 130 against 114 for a colour of TWO; the smallest stream is written.  With alpha 1 the plain stream's alpha
# residual is an 8-bit symbol (114 bits) and the palette entry's is not (102): the candidate's writer runs at packed width 1, which is what the case is for.
TWO_1X1 = np.array([[0, 1, 0, 1], [1, 0, 1, 1]], np.uint8)
FEW = ["dithered16", "dithered256", "noise2", "noise16", "dithered16_97x61"]
THRESHOLDS = [1, 2, 3, 4, 5, 16, 17, 256, 257]
EDGES = [("two_1x1", 2, 1, 1), ("two_7x1", 2, 7, 1), ("two_8x3", 2, 8, 3), ("two_9x3", 2, 9, 3), ("two_1x40", 2, 1, 40), ("two_67x9", 2, 67, 9), ("two_13000x3", 2, 13000, 3),
         ("four_3x5", 4, 3, 5), ("four_4x5", 4, 4, 5), ("four_5x5", 4, 5, 5), ("sixteen_1x20", 16, 1, 20), ("sixteen_2x20", 16, 2, 20), ("sixteen_3x20", 16, 3, 20)]
REFS_ROWS = ["rectangles16", "tiled16x16", "alpha_plane_as_grey", "flat", "texture20", "texture5"]


@functools.lru_cache(maxsize=None)
def pictures():
    """(name, (h, w, 3) RGB or (h, w, 4) RGBA pixels, palette): palette True = the stream must have the colour-indexing transform, False = it cannot (more than 256 colours),
    None = a picture of the refs battery that has a palette whose stream only has to be no larger"""
    rng = np.random.default_rng(3)
    def noise(k):
        colours = rng.integers(0, 256, (k, 3), dtype=np.uint8)
        return colours[rng.integers(0, k, (240, 320))]
    base = synth_rgb(31, 320, 240, texture=5.0)
    out = [("dithered16", dithered(base, 16), True), ("dithered256", dithered(base, 256), True), ("noise2", noise(2), True), ("noise16", noise(16), True),
           ("dithered16_97x61", dithered(synth_rgb(5, 97, 61, texture=5.0), 16), True)]
    out += [("exactly%d" % k, exactly(k, 40, 30, rng), k <= 256) for k in THRESHOLDS]
    for name, k, w, h in EDGES:
        if k == 2:
            out.append((name, (TWO_1X1 if w * h == 1 else TWO)[rng.integers(0, 2, (h, w))], True))
        else:
            out.append((name, exactly(k, w, h, rng), True))
    out.append(("two_rows_alike", np.tile(TWO[rng.integers(0, 2, (1, 320))], (240, 1, 1)), True))   # packed width 40, 9600 packed positions = 3 chunks
    table = dict(R.table_pictures())
    out += [(n, table[n], False if n.startswith("texture") else None) for n in REFS_ROWS]
    return tuple(out)


def colours_of(rgb):
    return len(np.unique(rgb.reshape(-1, rgb.shape[2]), axis=0))


def source_of(a):
    return D.lossless_of(np.ascontiguousarray(a), "RGBA", exact=True) if a.shape[2] == 4 else D.lossless_of(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def sources():
    return tuple(source_of(a) for _, a, _ in pictures())


_APIS = {}


@functools.lru_cache(maxsize=None)
def _coded(api_key, mode):
    with vp8l_mode(mode):
        outs = _APIS[api_key].cs_batch_compress(list(sources()), E.params(webp_lossless=True))
    for (name, _, _), o in zip(pictures(), outs):
        assert isinstance(o, bytes), (name, o)
    return tuple(outs)


def outputs(api, mode):
    _APIS[id(api)] = api
    return _coded(id(api), mode)


def packed_indices(argb):
    """(h, w) ARGB words -> (colours, the bundled indices as the format packs them: the palette ascending, 8 / 4 / 2 / 1 indices per packed pixel, lowest position
    in the lowest bits, a row's last packed pixel filled with zero bits)"""
    pal, idx = np.unique(argb, return_inverse=True)
    idx = idx.reshape(argb.shape).astype(np.uint32)
    n = len(pal)
    bits = 3 if n <= 2 else 2 if n <= 4 else 1 if n <= 16 else 0
    per, each = 1 << bits, 8 >> bits
    h, w = argb.shape
    pw = -(-w // per)
    padded = np.zeros((h, pw * per), np.uint32)
    padded[:, :w] = idx
    packed = (padded.reshape(h, pw, per) << (np.arange(per, dtype=np.uint32) * each)).sum(axis=2)
    return n, packed


def bound_bytes(argb, colours=None):
    """the literals-only cost of the palette stream: the order-0 entropy of the bundled indices, the prefix code's worst bit per symbol, the palette entries at
    <= 9 bits a channel, an allowance of 1024 bytes for six code descriptions and the framing"""
    n, packed = packed_indices(argb)
    count = np.bincount(packed.reshape(-1).astype(np.int64)).astype(np.float64)
    p = count[count > 0] / packed.size
    h0 = float(-(p * np.log2(p)).sum())
    return math.ceil(h0 * packed.size / 8) + packed.size / 8 + 5 * (colours if colours is not None else n) + 1024


def argb_of(rgb):
    a = rgb.astype(np.uint32)
    return np.uint32(0xFF000000) | (a[:, :, 0] << 16) | (a[:, :, 1] << 8) | a[:, :, 2]


# ---------------------------------------------------------------------------------------------------- the checks
def test_the_battery_is_what_its_names_say():
    for name, a, pal in pictures():
        if name.startswith("exactly"):
            assert colours_of(a) == int(name[7:]), name
        if pal is not None:
            assert (colours_of(a) <= 256) == pal, name
    got = {n: a.shape[:2][::-1] for n, a, _ in pictures()}
    assert all(got[n] == (w, h) for n, _, w, h in EDGES)
    assert colours_of(dict((n, a) for n, a, _ in pictures())["dithered16"]) == 16
    assert TOOL_CASES == [n for n, _, pal in pictures() if pal is not None]


def run_round_trip(api):
    """Pillow, this repo's decoder and the independent reader all read exactly the source's pixels"""
    outs = outputs(api, "palette")
    for (name, a, _), out in zip(pictures(), outs):
        check_file(out, a, name)
        check_tools(out, a, name)
    for (name, a, _), got in zip(pictures(), api.webp_decode(list(outs))):
        assert not isinstance(got, Exception), (name, got)
        assert np.array_equal(got[:, :, :a.shape[2]], a), name


def test_emul_palette_round_trips(api):
    run_round_trip(api)


TOOL_CASES = FEW + ["exactly%d" % k for k in THRESHOLDS] + [e[0] for e in EDGES] + ["two_rows_alike", "texture20", "texture5"]   # every picture that is not None


def run_tool_use(api, name):
    """the colour-indexing transform, alone, where a palette exists; never where there are more than 256 colours; every copy inside the window and the length cap
    (two_1x1: see TWO_1X1)"""
    names = [n for n, _, _ in pictures()]
    k = names.index(name)
    _, a, pal = pictures()[k]
    st = check_tools(outputs(api, "palette")[k], a, name)
    if pal:
        assert st.transforms == [3], (name, st.transforms)
    else:
        assert 3 not in st.transforms, (name, st.transforms)


@pytest.mark.parametrize("name", TOOL_CASES)
def test_emul_palette_tool_use(api, name):
    run_tool_use(api, name)


def run_packed_distances(api):
    """the refs stages see the PACKED width: rows alike are copies at distance 40, not 320, and the copies reach back past their chunk's start"""
    k = [n for n, _, _ in pictures()].index("two_rows_alike")
    st = R.parsed(outputs(api, "palette")[k])
    assert st.transforms == [3]
    assert any(d == 40 for _, d, _ in st.refs), st.refs[:8]
    assert any(p - d < (p // CHUNK) * CHUNK for _, d, p in st.refs if p >= CHUNK), st.refs


def test_emul_palette_copies_use_the_packed_width(api):
    run_packed_distances(api)


def run_never_larger(api):
    pal, refs = outputs(api, "palette"), outputs(api, "refs")
    for (name, a, _), p, r in zip(pictures(), pal, refs):
        print("%-22s colours %6d  refs %8d  palette %8d  libwebp %8d" % (name, colours_of(a), len(r), len(p), R.libwebp_size(source_of(a))))
    for (name, a, _), p, r in zip(pictures(), pal, refs):
        assert len(p) <= len(r), (name, len(p), len(r))
        if colours_of(a) > 256:
            assert p == r, name


def test_emul_palette_is_never_larger_and_is_refs_without_a_palette(api, capsys):
    with capsys.disabled():
        run_never_larger(api)


def run_bound(api):
    pal, refs = outputs(api, "palette"), outputs(api, "refs")
    rows = []
    for (name, a, _), p, r in zip(pictures(), pal, refs):
        if name in FEW:
            rows.append((name, len(p), bound_bytes(argb_of(a)), len(r)))
            print("%-22s palette %8d  bound %10.1f  refs %8d  palette/refs %.3f" % (rows[-1] + (len(p) / len(r),)))
    assert len(rows) == 5
    for name, p, bound, r in rows:
        assert p <= bound, (name, p, bound)
        assert p <= 0.75 * r, (name, p, r)


def test_emul_palette_meets_the_literals_only_bound(api, capsys):
    with capsys.disabled():
        run_bound(api)


def run_default_untouched(api):
    """unset, plain and refs write what they wrote before the palette existed: the digests were recorded on the emulation build of the commit before it"""
    want = json.load(open(DIGESTS))
    names = [n for n, _ in refs_battery()]
    for mode, key in ((None, "plain"), ("plain", "plain"), ("refs", "refs")):
        outs = R.outputs(api, mode)
        assert sorted(want[key]) == sorted(names)
        assert [n for n, o in zip(names, outs) if hashlib.sha256(o).hexdigest() != want[key][n]] == [], mode
    with vp8l_mode("palettes"):
        o = api.cs_batch_compress([refs_battery()[0][1]], E.params(webp_lossless=True))[0]
    assert isinstance(o, Exception) and o.code == 10201 and "CSH_VP8L" in str(o) and "palette" in str(o), o


def test_emul_default_plain_and_refs_do_not_move(api):
    run_default_untouched(api)


def png_of(arr, mode):
    b = io.BytesIO()
    Image.fromarray(arr, mode).save(b, "PNG")
    return b.getvalue()


def run_alpha_forms(api):
    """colours that differ only in alpha, and grey + alpha, from PNG sources through batch_convert"""
    rng = np.random.default_rng(8)
    levels = np.array([0, 60, 128, 200, 255], np.uint8)
    a = levels[rng.integers(0, 5, (45, 70))]
    rgba = np.dstack([np.full((45, 70, 3), (10, 200, 90), np.uint8), a])
    g = (np.array([30, 140, 250], np.uint8))[rng.integers(0, 3, (45, 70))]
    la = np.dstack([g, np.where(a > 100, 255, 0).astype(np.uint8)])
    srcs = [png_of(rgba, "RGBA"), png_of(la, "LA"), dict(png_cases())["RGBA_97x61"]]
    wants = [rgba, np.dstack([g, g, g, la[:, :, 1]]), np.asarray(Image.open(io.BytesIO(srcs[2])).convert("RGBA"))]
    p = E.params(webp_lossless=True)
    with vp8l_mode("palette"):
        pal = api.batch_convert(srcs, p, 3)
    with vp8l_mode("refs"):
        refs = api.batch_convert(srcs, p, 3)
    for k, (want, o, r) in enumerate(zip(wants, pal, refs)):
        assert isinstance(o, bytes) and isinstance(r, bytes), (o, r)
        check_file(o, want, str(k))
        st = check_tools(o, want, str(k))
        assert len(o) <= len(r), k
        if k < 2:
            assert st.transforms == [3] and len(o) < len(r), (k, st.transforms, len(o), len(r))
        else:
            assert colours_of(want) > 256 and o == r   # a photograph with transparency


def test_emul_palette_alpha_forms_from_png(api):
    run_alpha_forms(api)


def run_alph(api):
    """the ALPH chunk of a lossy conversion: R.run_alph with palette, and an alpha plane of iid noise over 4 levels against check 4's bound"""
    rng = np.random.default_rng(9)
    noisy = (np.array([0, 85, 170, 255], np.uint8))[rng.integers(0, 4, (90, 120))]
    big = np.dstack([synth_rgb(12, 320, 240, texture=6.0), R.alpha_plane()])
    srcs = [dict(png_cases())["RGBA_97x61"], png_of(big, "RGBA"), png_of(np.dstack([synth_rgb(13, 120, 90, texture=6.0), noisy]), "RGBA")]
    p = E.params(webp_quality=70)
    got = {}
    for mode in ("palette", "refs", None):
        with vp8l_mode(mode):
            got[mode] = api.batch_convert(srcs, p, 3)
    for k, (src, o, r, pl) in enumerate(zip(srcs, got["palette"], got["refs"], got[None])):
        assert isinstance(o, bytes) and isinstance(r, bytes) and isinstance(pl, bytes), (o, r, pl)
        co, cr, cp = R.chunks_of(o), R.chunks_of(r), R.chunks_of(pl)
        assert [c[0] for c in co] == [b"VP8X", b"ALPH", b"VP8 "]
        assert co[2][1] == cp[2][1]
        assert len(co[1][1]) <= len(cr[1][1]), (k, len(co[1][1]), len(cr[1][1]))
        alpha = np.asarray(Image.open(io.BytesIO(src)).convert("RGBA"))[:, :, 3]
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(o)).convert("RGBA"))[:, :, 3], alpha)
        st = V.parse(co[1][1][1:], headerless=(alpha.shape[1], alpha.shape[0]))
        assert np.array_equal((st.argb >> 8) & 255, alpha)
        if k == 2:
            a = alpha.astype(np.uint32)
            bound = bound_bytes(np.uint32(0xFF000000) | (a << 16) | (a << 8) | a, colours=4)
            print("ALPH of 4-level noise 120 x 90: palette %d  bound %.1f  refs %d" % (len(co[1][1]), bound, len(cr[1][1])))
            assert st.transforms == [3] and len(co[1][1]) <= bound, (len(co[1][1]), bound)


def test_emul_palette_alph_chunk(api, capsys):
    with capsys.disabled():
        run_alph(api)


def run_cli(binary, tmp_path):
    """caesiumclt --lossless over a dithered 16-colour WebP and --format webp --lossless over a P-mode PNG, CSH_VP8L=palette in the environment"""
    wd, pd = tmp_path / "webps", tmp_path / "pngs"
    wd.mkdir(); pd.mkdir()
    pics = dict((n, a) for n, a, _ in pictures())
    (wd / "dithered16.webp").write_bytes(D.lossless_of(pics["dithered16"]))
    Image.fromarray(pics["dithered16_97x61"]).quantize(16, dither=Image.Dither.NONE).save(pd / "p_mode.png")
    assert Image.open(pd / "p_mode.png").mode == "P"
    got = {}
    for mode in ("palette", "refs"):
        env = dict(os.environ, CSH_VP8L=mode)
        for tag, args in (("w", ["--lossless", wd]), ("p", ["--lossless", "--format", "webp", pd])):
            r = subprocess.run([binary, *map(str, args), "-o", str(tmp_path / (tag + mode)), "--json"], capture_output=True, text=True, env=env)
            j = json.loads(r.stdout)
            assert [f["status"] for f in j["files"]] == ["success"] and j["files"], r.stdout
            got[(mode, tag)] = open(j["files"][0]["output_path"], "rb").read()
    check_file(got[("palette", "w")], pics["dithered16"], "dithered16.webp")
    check_file(got[("palette", "p")], np.asarray(Image.open(pd / "p_mode.png").convert("RGB")), "p_mode.png")
    assert V.parse(got[("palette", "w")]).transforms == [3] and V.parse(got[("palette", "p")]).transforms == [3]
    assert len(got[("palette", "w")]) < len(got[("refs", "w")]) and len(got[("palette", "p")]) <= len(got[("refs", "p")])


def test_emul_palette_through_the_cli(api, tmp_path):
    run_cli(R.EMUL_CLI, tmp_path)


def run_batch_shape(api):
    """pictures with and without a palette in alternation, none with, all with: the order holds and every file is the one the picture gets alone"""
    src = dict(zip([n for n, _, _ in pictures()], sources()))
    photos = [D.lossless_of(synth_rgb(200 + i, w, h, texture=20.0)) for i, (w, h) in enumerate([(64, 48), (101, 67)])] + [src["exactly257"]]
    few = [src["dithered16_97x61"], src["exactly4"], src["two_67x9"]]
    p = E.params(webp_lossless=True)
    with vp8l_mode("palette"):
        alone = {s: api.compress_in_memory(s, p) for s in photos + few}
        for batch in ([few[0], photos[0], few[1], photos[1], few[2], photos[2]], photos, few, [photos[0], few[0], few[1], photos[1]]):
            outs = api.cs_batch_compress(batch, p)
            assert [o == alone[s] for s, o in zip(batch, outs)] == [True] * len(batch)
    for s in few:
        assert V.parse(alone[s]).transforms == [3]
    for s in photos:
        assert 3 not in V.parse(alone[s]).transforms


def test_emul_palette_batches_of_every_shape(api):
    run_batch_shape(api)


def test_emul_palette_does_not_depend_on_the_order_of_execution(api):
    """the palette is sorted by value and the count is a set's size: the emulation run backwards writes the same bytes"""
    import ctypes
    fwd = outputs(api, "palette")
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    with vp8l_mode("palette"):
        api.L.csh_emul_set_reverse(1)
        try:
            rev = api.cs_batch_compress(list(sources()), E.params(webp_lossless=True))
        finally:
            api.L.csh_emul_set_reverse(0)
    assert [n for (n, _, _), f, r in zip(pictures(), fwd, rev) if f != r] == []
