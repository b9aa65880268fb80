"""Lossless WebP OUTPUT with the meta prefix (entropy) image (CSH_VP8L=groups, k_vp8l_groups.hip): everything CSH_VP8L=palette does, and for every
picture of more than one tile one more candidate stream -- the refs stream's tokens coded with up to eight groups of five prefix codes, a group per tile -- of
which the smallest is written.  Pinned, as for the other coders: libwebp (Pillow), this repo's decoder and tests/_vp8l_parse.py read exactly the source's pixels;
the stream has an entropy image where regions differ and none where there is one tile; it is never larger than the palette mode's file and is that file where it
has no entropy image; on a picture of two unlike halves it is at most 0.94 of it; and unset / plain / refs / palette write the bytes they wrote before
(tests/golden/vp8l_refs_digests.json, tests/golden/vp8l_palette_digests.json).  The functions take the library: tests/test_zzz_webp_lossless_groups_gpu.py runs
them on the MI355X."""
import ctypes
import functools
import hashlib
import io
import json
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import _vp8l_parse as V
import test_webp_decode_emul as D
import test_webp_lossless_emul as E
import test_webp_lossless_palette_emul as P
import test_webp_lossless_refs_emul as R
from _util import ROOT, emul_api
from gen_synth import synth_rgb
from test_webp_lossless_palette_emul import source_of
from test_webp_lossless_refs_emul import check_file, check_tools, vp8l_mode

REFS_DIGESTS = os.path.join(ROOT, "tests", "golden", "vp8l_refs_digests.json")
PALETTE_DIGESTS = os.path.join(ROOT, "tests", "golden", "vp8l_palette_digests.json")
PAYS = 0.94   # halves_128x256: groups <= PAYS x palette (the model below gives the symbols 0.883 and the second set of descriptions and the entropy image 0.013)


@pytest.fixture(scope="module")
def api():
    return emul_api()


# ---------------------------------------------------------------------------------------------------- the pictures
def smooth(h, w, rng, y0=0):
    """(40 + x/2 + y/4, 200 - x/3, 90 + y) plus iid 0..7 per channel; y counts from row y0 of the whole picture"""
    x, y = np.arange(w)[None, :], np.arange(y0, y0 + h)[:, None]
    g = np.dstack([40 + x // 2 + y // 4, 200 - x // 3 + 0 * y, 90 + y + 0 * x])
    return ((g + rng.integers(0, 8, (h, w, 3))) & 255).astype(np.uint8)


def noise(h, w, rng):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def halves(h, w, rng=None):
    """the upper half iid uniform bytes, the lower half smooth"""
    rng = rng or np.random.default_rng(3)
    return np.vstack([noise(h // 2, w, rng), smooth(h - h // 2, w, rng, h // 2)])


def columns(h, w, rng):
    """the left half noise, the right half smooth"""
    return np.hstack([noise(h, w // 2, rng), smooth(h, w - w // 2, rng)])


MUST = ["halves_128x256", "halves_64x96", "bands_96x96", "halves_rgba_64x64"]   # an entropy image must show
CANNOT = ["one_tile_32x32", "1x1", "flat"]                                        # and cannot (one tile; nothing to gain)


@functools.lru_cache(maxsize=None)
def pictures():
    rng = np.random.default_rng(11)
    table, pal = dict(R.table_pictures()), dict((n, a) for n, a, _ in P.pictures())
    rgba = np.dstack([smooth(64, 64, rng), np.concatenate([np.full((32, 64), 255, np.uint8), rng.integers(0, 256, (32, 64), dtype=np.uint8)])])
    return (("halves_128x256", halves(128, 256)), ("halves_64x96", halves(64, 96)),
            ("bands_96x96", np.vstack([noise(32, 96, rng), smooth(32, 96, rng, 32), np.full((32, 96, 3), (9, 200, 31), np.uint8)])),
            ("halves_rgba_64x64", rgba), ("one_tile_32x32", noise(32, 32, rng)),
            ("33x33", halves(33, 33, rng)), ("31x65", halves(65, 31, rng)), ("1x1", noise(1, 1, rng)), ("4100x2", columns(2, 4100, rng)),
            ("tiled16x16", table["tiled16x16"]), ("rectangles16", table["rectangles16"]), ("flat", table["flat"]),
            ("texture5", synth_rgb(31, 320, 240, texture=5.0)), ("texture20", synth_rgb(31, 320, 240, texture=20.0)), ("dithered16", pal["dithered16"]))


@functools.lru_cache(maxsize=None)
def sources():
    return tuple(source_of(a) for _, a in pictures())


_APIS = {}


@functools.lru_cache(maxsize=None)
def _coded(api_key, mode):
    with vp8l_mode(mode):
        outs = _APIS[api_key].cs_batch_compress(list(sources()), E.params(webp_lossless=True))
    for (name, _), o in zip(pictures(), outs):
        assert isinstance(o, bytes), (name, o)
    return tuple(outs)


def outputs(api, mode):
    _APIS[id(api)] = api
    return _coded(id(api), mode)


def test_the_battery_is_what_its_names_say():
    got = {n: a.shape for n, a in pictures()}
    assert got["halves_128x256"] == (128, 256, 3) and got["halves_64x96"] == (64, 96, 3) and got["halves_rgba_64x64"] == (64, 64, 4)
    assert got["33x33"] == (33, 33, 3) and got["31x65"] == (65, 31, 3) and got["4100x2"] == (2, 4100, 3) and got["1x1"] == (1, 1, 3)
    assert set(MUST + CANNOT) <= set(got)


# ---------------------------------------------------------------------------------------------------- the checks
def run_round_trip(api):
    """Pillow, this repo's decoder and the independent reader all read exactly the source's pixels"""
    outs = outputs(api, "groups")
    for (name, a), out in zip(pictures(), outs):
        check_file(out, a, name)
        check_tools(out, a, name)
    for (name, a), got in zip(pictures(), api.webp_decode(list(outs))):
        assert not isinstance(got, Exception), (name, got)
        assert np.array_equal(got[:, :, :a.shape[2]], a), name


def test_emul_groups_round_trip(api):
    run_round_trip(api)


def run_tool_use(api):
    """an entropy image where the picture's regions differ, none where it is one tile or flat; without one the file is the palette mode's"""
    grp, pal = outputs(api, "groups"), outputs(api, "palette")
    seen = {}
    for (name, a), g, p in zip(pictures(), grp, pal):
        st = R.parsed(g)
        seen[name] = st.meta_prefix
        if not st.meta_prefix:
            assert g == p, name
        assert not R.parsed(p).meta_prefix, name
    print("entropy image:", " ".join("%s=%d" % kv for kv in seen.items()))
    assert [n for n in MUST if not seen[n]] == [] and [n for n in CANNOT if seen[n]] == []


def test_emul_groups_tool_use(api, capsys):
    with capsys.disabled():
        run_tool_use(api)


def run_never_larger(api):
    rows = [(n, len(g), len(p)) for (n, _), g, p in zip(pictures(), outputs(api, "groups"), outputs(api, "palette"))]
    rows += [(n, len(g), len(p)) for (n, _, _), g, p in zip(P.pictures(), P.outputs(api, "groups"), P.outputs(api, "palette"))]
    rows += [(n, len(g), len(p)) for (n, _), g, p in zip(R.battery(), R.outputs(api, "groups"), R.outputs(api, "palette"))]
    for n, g, p in rows:
        print("%-22s palette %8d  groups %8d  groups/palette %.4f" % (n, p, g, g / p))
    assert [(n, g, p) for n, g, p in rows if g > p] == []


def test_emul_groups_are_never_larger(api, capsys):
    with capsys.disabled():
        run_never_larger(api)


def left_residual_bits(a, parts):
    """order-0 entropy, in bits, of the left-neighbour residuals of every channel, with one set of statistics per part (a list of row slices)"""
    res = (a.astype(np.int16) - np.concatenate([a[:, :1] * 0, a[:, :-1]], axis=1)) & 255
    bits = 0.0
    for rows in parts:
        for c in range(a.shape[2]):
            n = np.bincount(res[rows, :, c].reshape(-1), minlength=256).astype(np.float64)
            n = n[n > 0]
            bits -= float((n * np.log2(n / n.sum())).sum())
    return bits


def test_the_model_stays_under_the_cap():
    """where PAYS comes from: two sets of statistics against one on halves_128x256, plus 0.013 for the second set of descriptions and the entropy image"""
    a = dict(pictures())["halves_128x256"]
    one, two = left_residual_bits(a, [slice(0, 128)]), left_residual_bits(a, [slice(0, 64), slice(64, 128)])
    assert two / one + 0.013 <= PAYS, (two / one, one, two)


def run_pays(api):
    k = [n for n, _ in pictures()].index("halves_128x256")
    g, p = len(outputs(api, "groups")[k]), len(outputs(api, "palette")[k])
    print("halves_128x256: palette %d  groups %d  groups/palette %.4f (<= %.2f)" % (p, g, g / p, PAYS))
    assert g <= PAYS * p, (g, p)


def test_emul_groups_pay(api, capsys):
    with capsys.disabled():
        run_pays(api)


def run_other_modes_untouched(api):
    """unset, plain, refs and palette write the bytes recorded on the emulation build of the commit before the groups existed; a name that is none fails per item"""
    want = json.load(open(REFS_DIGESTS))
    names = [n for n, _ in R.battery()]
    for mode, key in ((None, "plain"), ("plain", "plain"), ("refs", "refs")):
        assert sorted(want[key]) == sorted(names)
        assert [n for n, o in zip(names, R.outputs(api, mode)) if hashlib.sha256(o).hexdigest() != want[key][n]] == [], mode
    want = json.load(open(PALETTE_DIGESTS))["palette"]
    names = [n for n, _, _ in P.pictures()]
    assert sorted(want) == sorted(names)
    assert [n for n, o in zip(names, P.outputs(api, "palette")) if hashlib.sha256(o).hexdigest() != want[n]] == []
    with vp8l_mode("group"):
        outs = api.cs_batch_compress(list(sources()[:3]), E.params(webp_lossless=True))
    for o in outs:
        assert isinstance(o, Exception) and o.code == 10201 and "CSH_VP8L" in str(o) and "groups" in str(o), o


def test_emul_the_other_modes_do_not_move(api):
    run_other_modes_untouched(api)


def test_emul_groups_do_not_depend_on_the_order_of_execution(api):
    """every count is a sum and every choice goes by value and index: the emulation run backwards gives the same labels, so the same bytes"""
    fwd = outputs(api, "groups")
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    with vp8l_mode("groups"):
        api.L.csh_emul_set_reverse(1)
        try:
            rev = api.cs_batch_compress(list(sources()), E.params(webp_lossless=True))
        finally:
            api.L.csh_emul_set_reverse(0)
    assert [n for (n, _), f, r in zip(pictures(), fwd, rev) if f != r] == []


def run_batch_shape(api):
    """a batch of one; pictures that take the groups, the palette, the refs stream and the plain stream mixed, in both orders: the order holds and every file is the
    one the picture gets alone"""
    src = dict(zip([n for n, _ in pictures()], sources()))
    psrc = dict(zip([n for n, _, _ in P.pictures()], P.sources()))
    twice = np.tile(np.random.default_rng(17).integers(0, 256, (16, 32, 3), dtype=np.uint8), (2, 1, 1))   # one tile, 512 colours, its lower half a copy of the upper
    mix = [("groups", src["halves_64x96"]), ("palette", psrc["dithered16_97x61"]), ("refs", source_of(twice)), ("plain", src["one_tile_32x32"]), ("groups", src["bands_96x96"]),
           ("palette", psrc["exactly4"])]
    p = E.params(webp_lossless=True)
    with vp8l_mode("groups"):
        alone = [api.compress_in_memory(s, p) for _, s in mix]
        assert api.cs_batch_compress([mix[0][1]], p) == [alone[0]]
        assert api.cs_batch_compress([s for _, s in mix], p) == alone
        assert api.cs_batch_compress([s for _, s in mix[::-1]], p) == alone[::-1]
    for (kind, _), out in zip(mix, alone):
        st = V.parse(out)
        assert st.meta_prefix == (kind == "groups") and (3 in st.transforms) == (kind == "palette"), (kind, st.meta_prefix, st.transforms)
        if kind == "refs":
            assert st.refs
        if kind == "plain":
            assert not st.refs and st.cache_bits == 0
    with vp8l_mode("entropy"):
        outs = api.cs_batch_compress([s for _, s in mix], p)
    assert all(isinstance(o, Exception) and o.code == 10201 for o in outs), outs


def test_emul_groups_batches(api):
    run_batch_shape(api)


def run_alph(api):
    """the ALPH chunk of a lossy conversion follows the variable: an alpha plane that is half noise and half flat"""
    rng = np.random.default_rng(13)
    alpha = np.concatenate([rng.integers(0, 256, (32, 96), dtype=np.uint8), np.full((32, 96), 200, np.uint8)])
    src = P.png_of(np.dstack([synth_rgb(14, 96, 64, texture=6.0), alpha]), "RGBA")
    p = E.params(webp_quality=70)
    got = {}
    for mode in ("groups", "palette"):
        with vp8l_mode(mode):
            got[mode] = api.batch_convert([src], p, 3)[0]
        assert isinstance(got[mode], bytes), got[mode]
    cg, cp = R.chunks_of(got["groups"]), R.chunks_of(got["palette"])
    assert [c[0] for c in cg] == [b"VP8X", b"ALPH", b"VP8 "]
    assert cg[2][1] == cp[2][1]
    assert len(cg[1][1]) <= len(cp[1][1])
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got["groups"])).convert("RGBA"))[:, :, 3], alpha)
    st = V.parse(cg[1][1][1:], headerless=(96, 64))
    assert np.array_equal((st.argb >> 8) & 255, alpha)
    print("ALPH of half noise, half flat 96 x 64: palette %d  groups %d  entropy image %d" % (len(cp[1][1]), len(cg[1][1]), st.meta_prefix))


def test_emul_groups_alph_chunk(api, capsys):
    with capsys.disabled():
        run_alph(api)


def run_cli(binary, api, tmp_path):
    """caesiumclt --lossless over WebP files with CSH_VP8L=groups in the environment writes what the C ABI writes"""
    wd = tmp_path / "webps"
    wd.mkdir()
    src = dict(zip([n for n, _ in pictures()], sources()))
    for name in ("halves_64x96", "one_tile_32x32"):
        (wd / (name + ".webp")).write_bytes(src[name])
    r = subprocess.run([binary, "--lossless", str(wd), "-o", str(tmp_path / "out"), "--json"], capture_output=True, text=True, env=dict(os.environ, CSH_VP8L="groups"))
    j = json.loads(r.stdout)
    assert [f["status"] for f in j["files"]] == ["success"] * 2, r.stdout
    with vp8l_mode("groups"):
        for f in j["files"]:
            name = os.path.basename(f["original_path"])[:-5]
            assert open(f["output_path"], "rb").read() == api.compress_in_memory(src[name], E.params(webp_lossless=True)), name
    assert V.parse(open([f for f in j["files"] if "halves" in f["original_path"]][0]["output_path"], "rb").read()).meta_prefix


def test_emul_groups_through_the_cli(api, tmp_path):
    run_cli(R.EMUL_CLI, api, tmp_path)
