"""CMYK, YCCK and RGB-colourspace JPEG inputs (tests/_jpeg_spaces.py) through the emulation build, on every route: the coefficient transcode
against Pillow's decode and the oracle's coefficients; lossy under CSH_PROFILE=plain against Pillow / libjpeg-turbo's own re-save of the same
file from SOF on; under the default and the scalar profile every component against what the oracle makes of a grey (or YCbCr) file holding the same
coefficients; conversions to PNG, WebP and a resized JPEG against Pillow's convert("RGB") of the source; --max-size against libcaesium's walk; and a
batch that mixes these files with ordinary ones.  test_zzz_jpeg_spaces_gpu.py runs these bodies on the device."""
import contextlib
import io
import os

import numpy as np
import pytest

import _jpeg_spaces as S
from _jpeg_markers import listed, same_coefficients, seg, walk
from _util import device_quantiser, device_scan_script, emul_api, oracle_lossless, oracle_lossy, package
from gen_synth import synth_jpeg
from oracle import oracle as O

PNG, WEBP = 1, 3
_cache = {}


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


@contextlib.contextmanager
def profile(name):
    """CSH_PROFILE for the library (read when a batch is made) and for the oracle helpers of _util alike; None: unset (the default profile)"""
    old = os.environ.pop("CSH_PROFILE", None)
    if name:
        os.environ["CSH_PROFILE"] = name
    try:
        yield
    finally:
        os.environ.pop("CSH_PROFILE", None)
        if old is not None:
            os.environ["CSH_PROFILE"] = old


def one(api, key, call):
    """a call's result, once per library and key; a refusal as ("refused", code)"""
    k = (id(api),) + key
    if k not in _cache:
        try:
            _cache[k] = call()
        except package().CaesiumError as e:
            _cache[k] = ("refused", e.code)
    return _cache[k]


def lossless(api, name, data):
    return one(api, ("lossless", name), lambda: api.compress_in_memory(data, params(jpeg_optimize=True)))


def lossy(api, name, data, prof, **kw):
    def call():
        with profile(prof):
            return api.compress_in_memory(data, params(**kw))
    return one(api, ("lossy", name, prof, tuple(sorted(kw.items()))), call)


def to_png(api, name, data, width):
    return one(api, ("png", name, width), lambda: api.convert_in_memory(data, params(png_optimize=True, width=width), PNG))


def pil(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def pil_rgb(data):
    return np.asarray(pil(data).convert("RGB"))


def sof_on(data):
    return data[S.frame(data)["sof"]:]


def ncomp(kind):
    return 3 if kind == S.RGB else 4


# ---------------------------------------------------------------- 1. the coefficient transcode
def check_lossless(api):
    bad = []
    for name, data, kind in S.sources():
        out = lossless(api, name, data)
        if isinstance(out, tuple):
            bad.append((name, out))
            continue
        src, dst = pil(data), pil(out)
        if src.mode != dst.mode or not np.array_equal(np.asarray(src), np.asarray(dst)):
            bad.append((name, "Pillow decodes other samples"))
        a, b = O.decode(data), O.decode(out)
        if not same_coefficients(a, b):
            bad.append((name, "coefficients"))
        fa, fb = S.frame(data), S.frame(out)
        if fa["comps"] != fb["comps"] or fa["adobe"] != fb["adobe"] or fb["jfif"] or fb["marker"] != 0xC2:
            bad.append((name, "frame", fa, fb))
        if any(not np.array_equal(a.qtable(t), b.qtable(t)) for t in {c[3] for c in fa["comps"]}):
            bad.append((name, "quantisation tables"))
        if b.scans() != S.general_script(ncomp(kind)):
            bad.append((name, "scans", b.scans()))
        if "prog" in name and sof_on(out) != sof_on(data):   # Pillow's progressive, optimised file IS libjpeg's all-purpose script with optimal tables
            bad.append((name, "differs from the source behind SOF2"))
    assert not bad, listed(bad)


# ---------------------------------------------------------------- 2. CSH_PROFILE=plain against libjpeg-turbo
def pillow_resave(data, kind, table, progressive):
    b = io.BytesIO()
    pil(data).save(b, "JPEG", qtables=[[int(v) for v in table]], progressive=progressive, optimize=True, **({"keep_rgb": True} if kind == S.RGB else {}))
    return b.getvalue()


def merged_dht(data):
    """the file with every run of consecutive DHT segments written as ONE segment holding their tables in order -- mozjpeg's marker style (emit_multi_dht),
    which the library writes as the reference's engine does; libjpeg-turbo writes a segment per table"""
    out, last, run = bytearray(), 0, []
    segs = walk(data)
    for k, (m, a, b) in enumerate(segs):
        if m == 0xC4:
            run.append((a, b))
            if segs[k + 1][0] != 0xC4:
                body = b"".join(data[x + 4:y] for x, y in run)
                out += data[last:run[0][0]] + seg(0xC4, body)
                last, run = b, []
    return bytes(out + data[last:])


def check_plain_equals_libjpeg(api):
    """no colour conversion lies on either side: Pillow hands libjpeg-turbo the samples it decoded, in the file's own space.  Progressive files are compared
    as they are.  A baseline file of Pillow's differs from the library's in one thing, traced to the marker style and not to what is coded: libjpeg-turbo
    writes its two optimal tables as two DHT segments (28 + 46 bytes in the 17 x 9 RGB case), the library as one (70 bytes: the same tables in the same
    order, one segment header less) -- so the reference is Pillow's file with that run of segments merged, and everything else still has to be equal byte for byte"""
    bad = []
    for name, data, kind in S.sources():
        if kind not in (S.CMYK, S.RGB):
            continue
        for progressive in (True, False):
            out = lossy(api, name, data, "plain", jpeg_progressive=progressive)
            if isinstance(out, tuple):
                bad.append((name, progressive, out))
                continue
            table = O.decode(out).qtable(0)
            ref = pillow_resave(data, kind, table, progressive)
            assert np.array_equal(O.decode(ref).qtable(0), table), "Pillow did not take the table"
            f = S.frame(out)
            want_ids = b"RGB" if kind == S.RGB else b"CMYK"
            if bytes(c[0] for c in f["comps"]) != want_ids or any(c[1:] != (1, 1, 0) for c in f["comps"]) or f["jfif"] or f["adobe"] != S.frame(data)["adobe"]:
                bad.append((name, progressive, "frame", f))
            if sof_on(out) != sof_on(ref if progressive else merged_dht(ref)):
                bad.append((name, progressive, "differs from Pillow's re-save", len(out), len(ref)))
    assert not bad, listed(bad)


# ---------------------------------------------------------------- 3. the default and the scalar profile against the oracle, per component
def check_profile_equals_oracle(api, prof):
    bad = []
    for name, data, kind in S.sources():
        out = lossy(api, name, data, prof)
        if isinstance(out, tuple):
            bad.append((name, out))
            continue
        got, f = O.decode(out), S.frame(out)
        if got.scans() != S.general_script(ncomp(kind)):
            bad.append((name, "scans", got.scans()))
        with profile(prof):
            if kind == S.YCCK:
                # Y and K at the luma factors of 4:2:0 (Auto), Cb and Cr 1x1; tables 0 1 1 0
                if [c[1:] for c in f["comps"]] != [(2, 2, 0), (1, 1, 1), (1, 1, 1), (2, 2, 0)] or f["adobe"] != 2 or f["jfif"]:
                    bad.append((name, "frame", f))
                ref = O.decode(oracle_lossy(S.ycc_of(data)))
                for c in range(3):
                    if not np.array_equal(S.real_blocks(got, c), S.real_blocks(ref, c)):
                        bad.append((name, "component", c))
                singles = [3]
            else:
                singles = range(ncomp(kind))
            for c in singles:
                ref = O.decode(oracle_lossy(S.grey_of(data, c)))
                if not np.array_equal(S.real_blocks(got, c), S.real_blocks(ref, 0)):
                    bad.append((name, "component", c, "differs from the oracle's grey file"))
        again = lossless(api, name + "/" + str(prof), out)
        if isinstance(again, tuple) or sof_on(again) != sof_on(out):
            bad.append((name, "its own output does not transcode to itself"))
    assert not bad, listed(bad)


# ---------------------------------------------------------------- 4. to PNG
def check_png(api):
    from PIL import Image
    bad = []
    for name, data, kind in S.sources():
        rgb = pil_rgb(data)
        h, w = rgb.shape[:2]
        for width in (0, max(3, (w * 5) // 8)):
            out = to_png(api, name, data, width)
            if isinstance(out, tuple):
                bad.append((name, width, out))
                continue
            got = np.asarray(Image.open(io.BytesIO(out)).convert("RGB"))
            want = rgb if not width else O.lanczos3_resize(rgb, *O.compute_dimensions(w, h, width, 0))
            if got.shape != want.shape or not np.array_equal(got, want):
                bad.append((name, width, int(np.abs(got.astype(int) - want.astype(int)).max()) if got.shape == want.shape else ("shape", got.shape, want.shape)))
    assert not bad, listed(bad)


# ---------------------------------------------------------------- 5. to lossy WebP, and resized toward JPEG
def check_webp_and_resized_jpeg(api):
    bad = []
    for name, data, kind in S.sources():
        rgb = pil_rgb(data)
        h, w = rgb.shape[:2]
        out = one(api, ("webp", name), lambda: api.convert_in_memory(data, params(webp_quality=85), WEBP))
        if out != O.webp_encode_rgb(rgb, 85):
            bad.append((name, "webp", out if isinstance(out, tuple) else "other bytes"))
        width = max(9, (w * 3) // 4)
        out = one(api, ("resized", name), lambda: api.compress_in_memory(data, params(width=width)))
        want = O.pixels_to_jpeg(rgb, O.params(quality=80, progressive=1, subsampling=420, qtable_profile=3, marker_style=1, scan_script=device_scan_script(), **device_quantiser()), width, 0)
        if out != want:   # an ordinary YCbCr JPEG of the resized RGB
            bad.append((name, "resized jpeg", out if isinstance(out, tuple) else "other bytes"))
    assert not bad, listed(bad)


# ---------------------------------------------------------------- 6. --max-size
def libcaesium_walk(encode, max_size):
    """libcaesium's bisection (quality 80, bounds 1 / 101, 2 % tolerance, 10 tries) over encode(q) -> (quality it ends at, bytes)"""
    tol = max_size * 2 // 100
    q, less, high, out = 80, 1, 101, None
    for _ in range(10):
        out = encode(q)
        if len(out) <= max_size and max_size - len(out) < tol:
            return q, out
        if len(out) <= max_size:
            less = q
        else:
            high = q
        nq = min(max((high + less) // 2, 1), 100)
        if nq == q:
            return q, out
        q = nq
    return q, out


def check_max_size(api):
    bad = []
    for name, data, kind in S.sources():
        if name not in ("cmyk_base_97x61", "rgb_prog_97x61", "ycck_2112_200x150", "cmyk_plain_17x9"):
            continue
        at80 = lossy(api, name, data, None)
        for target in (len(lossy(api, name, data, None, jpeg_quality=40)) + 1, len(at80) * 3):   # one the walk has to come down for, one the first try meets
            p = params()
            try:
                out = api.compress_to_size_in_memory(data, p, target)
            except package().CaesiumError as e:
                bad.append((name, target, e.code))
                continue
            q = int(p.jpeg_quality)
            if len(out) > target:
                bad.append((name, target, "does not fit", len(out)))
            if out != lossy(api, name, data, None, jpeg_quality=q):
                bad.append((name, target, "differs from a plain run at the reported quality", q))
            wq, wout = libcaesium_walk(lambda qq: lossy(api, name, data, None, jpeg_quality=qq), target)
            if (wq, wout) != (q, out):
                bad.append((name, target, "walk ends at", wq, "call reports", q))
    assert not bad, listed(bad)


# ---------------------------------------------------------------- 7. a mixed batch
def ordinary():
    from PIL import Image
    g = io.BytesIO()
    Image.fromarray(np.asarray(pil(synth_jpeg(53, 90, 50, texture=9)).convert("L"))).save(g, "JPEG", quality=85)
    return [("ordinary_420_80x56", synth_jpeg(51, 80, 56, texture=10)), ("ordinary_prog_444_57x35", synth_jpeg(52, 57, 35, subsampling=0, progressive=True, texture=5)),
            ("ordinary_grey_90x50", g.getvalue())]


def check_mixed_batch(api):
    mixed = []
    for k, (name, data, _) in enumerate(S.sources()):
        mixed += [ordinary()[k % 3], (name, data)]
    blobs = [m[1] for m in mixed]
    for kind, p, ref in (("lossy", params(), oracle_lossy), ("lossless", params(jpeg_optimize=True), oracle_lossless)):
        outs = api.batch_compress(blobs, p)
        assert len(outs) == len(blobs)
        bad = []
        for k, ((name, data), out) in enumerate(zip(mixed, outs)):
            if isinstance(out, Exception):
                bad.append((k, name, out.code))
            elif name.startswith("ordinary"):
                if out != ref(data):
                    bad.append((k, name, "differs from the oracle"))
            elif out != (lossy(api, name, data, None) if kind == "lossy" else lossless(api, name, data)):
                bad.append((k, name, "differs from the file alone"))
        assert not bad, kind + ": " + listed(bad)
    outs = api.batch_convert(blobs, params(png_optimize=True), PNG)
    bad = [(k, m[0]) for k, (m, out) in enumerate(zip(mixed, outs)) if isinstance(out, Exception) or (not m[0].startswith("ordinary") and out != to_png(api, m[0], m[1], 0))]
    assert not bad, "png: " + listed(bad)


def test_lossless_transcode(api):
    check_lossless(api)


def test_plain_profile_equals_libjpeg_turbo(api):
    check_plain_equals_libjpeg(api)


@pytest.mark.parametrize("prof", [None, "scalar"], ids=["default", "scalar"])
def test_profile_equals_oracle_per_component(api, prof):
    check_profile_equals_oracle(api, prof)


def test_to_png_equals_pillow_rgb(api):
    check_png(api)


def test_to_webp_and_resized_jpeg(api):
    check_webp_and_resized_jpeg(api)


def test_max_size(api):
    check_max_size(api)


def test_mixed_batch_equals_file_by_file(api):
    check_mixed_batch(api)
