"""Lossless WebP OUTPUT with a match finder over the format's whole window (CSH_VP8L=far, k_vp8l_far.hip): everything CSH_VP8L=groups does, and
for every record a second token set from a hash chain over the whole record, of which the smaller in exact bits is kept.  Pinned: libwebp (Pillow), this repo's
decoder and tests/_vp8l_parse.py read exactly the source's pixels; a band repeated 128 rows lower (and one repeated 1 048 320 positions lower, the window's edge)
is coded as copies of the first and costs what the picture without the second band costs; a band 1 048 512 positions lower is outside the window and is not;
no file is larger than the groups mode's; unset / plain / refs / palette / groups write the bytes they wrote before (tests/golden/vp8l_*_digests.json).  The
functions take the library: tests/test_zzz_webp_lossless_far_gpu.py runs them on the MI355X."""
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
import test_webp_lossless_emul as E
import test_webp_lossless_groups_emul as G
import test_webp_lossless_palette_emul as P
import test_webp_lossless_refs_emul as R
from _util import ROOT, emul_api
from gen_synth import synth_rgb
from test_webp_lossless_palette_emul import source_of
from test_webp_lossless_refs_emul import check_file, check_tools, vp8l_mode

REFS_DIGESTS = os.path.join(ROOT, "tests", "golden", "vp8l_refs_digests.json")
PALETTE_DIGESTS = os.path.join(ROOT, "tests", "golden", "vp8l_palette_digests.json")
GROUPS_DIGESTS = os.path.join(ROOT, "tests", "golden", "vp8l_groups_digests.json")
WINDOW = R.WINDOW


@pytest.fixture(scope="module")
def api():
    return emul_api()


# ---------------------------------------------------------------------------------------------------- the pictures
def flat(h, w): return np.full((h, w, 3), (9, 200, 31), np.uint8)
def build(w, gap_rows, second=True, band=48, seed=5):      # flat 16 rows | A | noise gap | flat 16 rows | A or flat
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 256, (band, w, 3), dtype=np.uint8)
    N = rng.integers(0, 256, (gap_rows, w, 3), dtype=np.uint8)
    return np.vstack([flat(16, w), A, N, flat(16, w), A if second else flat(band, w)])
def edge(w, second=True):                                   # flat 16 | A (16 rows) | flat 48 | A or flat
    rng = np.random.default_rng(9)
    A = rng.integers(0, 256, (16, w, 3), dtype=np.uint8)
    return np.vstack([flat(16, w), A, flat(48, w), A if second else flat(16, w)])
# two = build(256, 64); one = build(256, 64, False); near_two = build(256, 0, band=16); near_one = build(256, 0, False, band=16)
# edge_in = edge(16380); edge_out = edge(16383); edge_one = edge(16383, False)


def rgba_repeat():
    """build()'s layout with an alpha sample: flat 16 | A (48 rows) | noise 32 | flat 16 | A, 256 wide: the second A lies 96 x 256 = 24 576 positions behind the first"""
    rng = np.random.default_rng(21)
    f = np.full((16, 256, 4), (9, 200, 31, 140), np.uint8)
    A, N = rng.integers(0, 256, (48, 256, 4), dtype=np.uint8), rng.integers(0, 256, (32, 256, 4), dtype=np.uint8)
    return np.vstack([f, A, N, f, A])


def alpha_repeat():
    """an alpha plane in build()'s layout, 256 x 192: its band comes back 128 x 256 = 32 768 positions lower"""
    rng = np.random.default_rng(22)
    A, N = rng.integers(0, 256, (48, 256), dtype=np.uint8), rng.integers(0, 256, (64, 256), dtype=np.uint8)
    f = np.full((16, 256), 200, np.uint8)
    return np.vstack([f, A, N, f, A])


SLOW_READ = ["edge_one"]   # the pure-Python reader takes about 3 s on a file of 1.5 M pixels: it reads edge_in and edge_out


@functools.lru_cache(maxsize=None)
def pictures():
    table, pal, grp = dict(R.table_pictures()), dict((n, a) for n, a, _ in P.pictures()), dict(G.pictures())
    return (("two", build(256, 64)), ("one", build(256, 64, False)), ("near_two", build(256, 0, band=16)), ("near_one", build(256, 0, False, band=16)),
            ("edge_in", edge(16380)), ("edge_out", edge(16383)), ("edge_one", edge(16383, False)),
            ("tiled16x16", table["tiled16x16"]), ("rectangles16", table["rectangles16"]), ("flat", table["flat"]), ("dithered16", pal["dithered16"]),
            ("texture5", synth_rgb(31, 320, 240, texture=5.0)), ("halves_128x256", grp["halves_128x256"]), ("33x33", grp["33x33"]), ("1x1", grp["1x1"]),
            ("4100x2", grp["4100x2"]), ("rgba_repeat", rgba_repeat()))


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


def named(api, mode):
    return dict(zip([n for n, _ in pictures()], outputs(api, mode)))


def test_the_battery_is_what_its_names_say():
    got = {n: a.shape for n, a in pictures()}
    assert got["two"] == got["one"] == (192, 256, 3) and got["near_two"] == got["near_one"] == (64, 256, 3)
    assert got["edge_in"] == (96, 16380, 3) and got["edge_out"] == got["edge_one"] == (96, 16383, 3) and got["rgba_repeat"] == (160, 256, 4)
    pics = dict(pictures())
    assert np.array_equal(pics["two"][16:64], pics["two"][144:192]) and np.array_equal(pics["edge_in"][16:32], pics["edge_in"][80:96])
    assert 64 * 16380 <= WINDOW < 64 * 16383 and 128 * 256 > 16384


# ---------------------------------------------------------------------------------------------------- the checks
def run_round_trip(api):
    """1: Pillow, this repo's decoder and the independent reader all read exactly the source's pixels; 4: every copy of every file stays inside the window and
    inside the picture (check_tools)"""
    outs = outputs(api, "far")
    for (name, a), out in zip(pictures(), outs):
        check_file(out, a, name)
        if name not in SLOW_READ:
            check_tools(out, a, name)
    for (name, a), got in zip(pictures(), api.webp_decode(list(outs))):
        assert not isinstance(got, Exception), (name, got)
        assert np.array_equal(got[:, :, :a.shape[2]], a), name


def test_emul_far_round_trip(api):
    run_round_trip(api)


def copied(blob, dist):
    """the pixels of the file's copies at exactly this distance"""
    return sum(l for l, d, _ in R.parsed(blob).refs if d == dist)


def run_far_copy_found(api):
    """2: the second band is coded as copies of the first.  On the code as it stood CSH_VP8L=groups wrote `two` without one such copy"""
    far = named(api, "far")
    got = copied(far["two"], 128 * 256), copied(far["edge_in"], 64 * 16380)
    print("copied at 128 x 256 in two: %d of %d; at 64 x 16380 in edge_in: %d of %d" % (got[0], 48 * 256, got[1], 16 * 16380))
    assert got[0] >= 48 * 256 - 64 and got[1] >= 16 * 16380 - 64, got


def test_emul_far_copy_is_found(api, capsys):
    with capsys.disabled():
        run_far_copy_found(api)


def run_far_copy_pays(api):
    """3: at most 58 bits per copy token: `two` needs 3 copies of 4096 pixels, at most 6 with the chunks' cuts, edge_in 64, at most 128: 44 and 928 bytes, and two
    slightly longer code descriptions"""
    far, grp = named(api, "far"), named(api, "groups")
    print("two: far %d  groups %d  groups(one) %d;  edge_in: far %d  groups %d  groups(edge_one) %d" %
          (len(far["two"]), len(grp["two"]), len(grp["one"]), len(far["edge_in"]), len(grp["edge_in"]), len(grp["edge_one"])))
    assert len(far["two"]) <= len(grp["one"]) + 256, (len(far["two"]), len(grp["one"]))
    assert len(far["edge_in"]) <= len(grp["edge_one"]) + 1024, (len(far["edge_in"]), len(grp["edge_one"]))


def test_emul_far_copy_pays(api, capsys):
    with capsys.disabled():
        run_far_copy_pays(api)


def run_window(api):
    """4: a band 1 048 512 positions lower is outside the window: no copy reaches it (every copy is held to the window and to its position), and the file pays for
    the band twice"""
    far = named(api, "far")
    for name in ("edge_out", "edge_in"):
        refs = R.parsed(far[name]).refs
        assert refs and all(1 <= d <= WINDOW and d <= p for _, d, p in refs), name
    assert copied(far["edge_out"], 64 * 16383) == 0
    print("edge_out: far %d = %.3f x edge_in's %d" % (len(far["edge_out"]), len(far["edge_out"]) / len(far["edge_in"]), len(far["edge_in"])))
    assert len(far["edge_out"]) >= 1.9 * len(far["edge_in"])


def test_emul_far_window_holds(api, capsys):
    with capsys.disabled():
        run_window(api)


def run_never_larger(api):
    """5: per picture the far file is never larger than the groups file"""
    rows = [(n, len(f), len(g)) for (n, _), f, g in zip(pictures(), outputs(api, "far"), outputs(api, "groups"))]
    rows += [(n, len(f), len(g)) for (n, _), f, g in zip(G.pictures(), G.outputs(api, "far"), G.outputs(api, "groups"))]
    rows += [(n, len(f), len(g)) for (n, _, _), f, g in zip(P.pictures(), P.outputs(api, "far"), P.outputs(api, "groups"))]
    rows += [(n, len(f), len(g)) for (n, _), f, g in zip(R.battery(), R.outputs(api, "far"), R.outputs(api, "groups"))]
    for n, f, g in rows:
        print("%-22s groups %8d  far %8d  far/groups %.4f" % (n, g, f, f / g))
    assert [(n, f, g) for n, f, g in rows if f > g] == []


def test_emul_far_is_never_larger(api, capsys):
    with capsys.disabled():
        run_never_larger(api)


def run_other_modes_untouched(api):
    """6: unset, plain, refs, palette and groups write the bytes recorded on the emulation build of the commit before this mode existed; a name that is none fails
    per item and the message names far"""
    sha = lambda o: hashlib.sha256(o).hexdigest()
    want = json.load(open(REFS_DIGESTS))
    names = [n for n, _ in R.battery()]
    for mode, key in ((None, "plain"), ("plain", "plain"), ("refs", "refs")):
        assert sorted(want[key]) == sorted(names)
        assert [n for n, o in zip(names, R.outputs(api, mode)) if sha(o) != want[key][n]] == [], mode
    want = json.load(open(PALETTE_DIGESTS))["palette"]
    pnames = [n for n, _, _ in P.pictures()]
    assert sorted(want) == sorted(pnames)
    assert [n for n, o in zip(pnames, P.outputs(api, "palette")) if sha(o) != want[n]] == []
    want = json.load(open(GROUPS_DIGESTS))
    for key, nm, outs in (("refs", names, R.outputs(api, "groups")), ("palette", pnames, P.outputs(api, "groups")), ("groups", [n for n, _ in G.pictures()], G.outputs(api, "groups"))):
        assert sorted(want[key]) == sorted(nm)
        assert [n for n, o in zip(nm, outs) if sha(o) != want[key][n]] == [], key
    with vp8l_mode("fars"):
        outs = api.cs_batch_compress(list(sources()[:4]), E.params(webp_lossless=True))
    for o in outs:
        assert isinstance(o, Exception) and o.code == 10201 and "CSH_VP8L" in str(o) and "far" in str(o).split("(")[-1].replace(")", "").split(", "), o


def test_emul_the_other_modes_do_not_move(api):
    run_other_modes_untouched(api)


def test_emul_far_does_not_depend_on_the_order_of_execution(api):
    """7: the chain is a stable sort by value and every choice goes by value: the emulation run backwards writes the same bytes"""
    fwd = outputs(api, "far")
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    with vp8l_mode("far"):
        api.L.csh_emul_set_reverse(1)
        try:
            rev = api.cs_batch_compress(list(sources()), E.params(webp_lossless=True))
        finally:
            api.L.csh_emul_set_reverse(0)
    assert [n for (n, _), f, r in zip(pictures(), fwd, rev) if f != r] == []


def run_batch_shape(api):
    """8: a photograph, a palette picture and a picture with a far repeat in one batch, in both orders: every file is the one the picture gets alone"""
    src = dict(zip([n for n, _ in pictures()], sources()))
    psrc = dict(zip([n for n, _, _ in P.pictures()], P.sources()))
    mix = [("photo", src["texture5"]), ("palette", psrc["dithered16_97x61"]), ("far", src["two"]), ("far", src["rgba_repeat"])]
    p = E.params(webp_lossless=True)
    with vp8l_mode("far"):
        alone = [api.compress_in_memory(s, p) for _, s in mix]
        assert api.cs_batch_compress([s for _, s in mix], p) == alone
        assert api.cs_batch_compress([s for _, s in mix[::-1]], p) == alone[::-1]
    assert 3 in V.parse(alone[1]).transforms
    assert copied(alone[2], 128 * 256) >= 48 * 256 - 64 and copied(alone[3], 96 * 256) >= 48 * 256 - 64


def test_emul_far_batches(api):
    run_batch_shape(api)


def run_cli(binary, api, tmp_path):
    """8: caesiumclt --lossless over a WebP file with CSH_VP8L=far in the environment writes what the C ABI writes"""
    wd = tmp_path / "webps"
    wd.mkdir()
    src = dict(zip([n for n, _ in pictures()], sources()))["two"]
    (wd / "two.webp").write_bytes(src)
    r = subprocess.run([binary, "--lossless", str(wd), "-o", str(tmp_path / "out"), "--json"], capture_output=True, text=True, env=dict(os.environ, CSH_VP8L="far"))
    j = json.loads(r.stdout)
    assert [f["status"] for f in j["files"]] == ["success"], r.stdout
    blob = open(j["files"][0]["output_path"], "rb").read()
    with vp8l_mode("far"):
        assert blob == api.compress_in_memory(src, E.params(webp_lossless=True))
    assert copied(blob, 128 * 256) >= 48 * 256 - 64


def test_emul_far_through_the_cli(api, tmp_path):
    run_cli(R.EMUL_CLI, api, tmp_path)


def run_alph(api):
    """1, 8: the ALPH chunk of a lossy conversion follows the variable: an alpha plane whose band comes back 32 768 positions lower is coded as copies of it"""
    alpha = alpha_repeat()
    src = P.png_of(np.dstack([synth_rgb(14, 256, 192, texture=6.0), alpha]), "RGBA")
    p = E.params(webp_quality=70)
    got = {}
    for mode in ("far", "groups"):
        with vp8l_mode(mode):
            got[mode] = api.batch_convert([src], p, 3)[0]
        assert isinstance(got[mode], bytes), got[mode]
    cf, cg = R.chunks_of(got["far"]), R.chunks_of(got["groups"])
    assert [c[0] for c in cf] == [b"VP8X", b"ALPH", b"VP8 "]
    assert cf[2][1] == cg[2][1]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got["far"])).convert("RGBA"))[:, :, 3], alpha)
    st = V.parse(cf[1][1][1:], headerless=(256, 192))
    assert np.array_equal((st.argb >> 8) & 255, alpha)
    assert all(1 <= d <= WINDOW and d <= pos for _, d, pos in st.refs)
    far_px = sum(l for l, d, _ in st.refs if d == 128 * 256)
    print("ALPH with a band 32 768 positions lower, 256 x 192: groups %d  far %d  copied at that distance %d of %d" % (len(cg[1][1]), len(cf[1][1]), far_px, 48 * 256))
    assert far_px >= 48 * 256 - 64 and len(cf[1][1]) < len(cg[1][1])


def test_emul_far_alph_chunk(api, capsys):
    with capsys.disabled():
        run_alph(api)
