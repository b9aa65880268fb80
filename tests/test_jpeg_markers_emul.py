"""Files whose DRI, DQT or DHT change between two scans (tests/_jpeg_markers.py) through the emulation build: every case converted to PNG
against Pillow's own decode of the file, compressed against oracle_lossy, transcoded against oracle_lossless -- all exact -- and the whole
battery as one batch between ordinary files against the same files one by one.  test_zzz_jpeg_markers_gpu.py runs these bodies on the device."""
import io

import numpy as np
import pytest

from _jpeg_markers import MISMATCHED, battery, listed, ordinary, references, same_coefficients
from _util import emul_api, package
from oracle import oracle as O

PNG = 1
UNSUPPORTED_JPEG_FEATURE = 20101
KINDS = {"png": (lambda: params(png_optimize=True)), "lossy": (lambda: params()), "lossless": (lambda: params(jpeg_optimize=True))}
_singles = {}


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


def norm(out):
    return ("refused", out.code) if isinstance(out, Exception) else out


def singles(api, kind):
    """every file of the battery and the ordinary ones through the single-file entry points, once per library: name -> bytes or ("refused", code)"""
    key = (id(api), kind)
    if key not in _singles:
        res = {}
        for name, data, _ in battery() + ordinary():
            try:
                res[name] = api.convert_in_memory(data, KINDS[kind](), PNG) if kind == "png" else api.compress_in_memory(data, KINDS[kind]())
            except package().CaesiumError as e:
                res[name] = norm(e)
        _singles[key] = res
    return _singles[key]


def png_rgb(out):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(out)).convert("RGB"))


def check_png_equals_pillow(api):
    got, ref, bad = singles(api, "png"), references(), []
    for name, _, _ in battery():
        out = got[name]
        if isinstance(out, tuple):
            bad.append((name, out))
            continue
        rgb = png_rgb(out)
        if rgb.shape != ref[name]["rgb"].shape or not np.array_equal(rgb, ref[name]["rgb"]):
            bad.append((name, int(np.abs(rgb.astype(int) - ref[name]["rgb"].astype(int)).max()) if rgb.shape == ref[name]["rgb"].shape else "shape"))
    assert not bad, listed(bad)


def check_lossy_equals_oracle(api):
    got, ref = singles(api, "lossy"), references()
    bad = [name for name, _, _ in battery() if got[name] != ref[name]["lossy"]]
    assert not bad, listed(bad)


def check_lossless_equals_oracle(api):
    got, ref, bad = singles(api, "lossless"), references(), []
    for name, data, expect in battery():
        if expect == MISMATCHED:   # refused by the oracle and the library alike, and only here: the two checks above hold for this file too
            if not isinstance(ref[name]["lossless"], O.OracleError) or got[name] != ("refused", UNSUPPORTED_JPEG_FEATURE):
                bad.append((name, got[name] if isinstance(got[name], tuple) else "transcoded", ref[name]["lossless"] if isinstance(ref[name]["lossless"], Exception) else "oracle transcoded"))
            continue
        if isinstance(ref[name]["lossless"], Exception) or got[name] != ref[name]["lossless"]:
            bad.append((name, got[name] if isinstance(got[name], tuple) else "other bytes"))
            continue
        if not same_coefficients(O.decode(data), O.decode(got[name])):
            bad.append((name, "coefficients"))
    assert not bad, listed(bad)


def check_batch_equals_file_by_file(api):
    """the battery as one batch, an ordinary file in front of each case: the same results in the same order as file by file (nothing the
    planner keeps for one item reaches the next)"""
    mixed = []
    for k, case in enumerate(battery()):
        mixed += [ordinary()[k % len(ordinary())], case]
    blobs = [c[1] for c in mixed]
    for kind in KINDS:
        outs = api.batch_convert(blobs, KINDS[kind](), PNG) if kind == "png" else api.batch_compress(blobs, KINDS[kind]())
        assert len(outs) == len(mixed)
        one = singles(api, kind)
        bad = [(k, c[0]) for k, (c, out) in enumerate(zip(mixed, outs)) if norm(out) != one[c[0]]]
        assert not bad, kind + ": " + listed(bad)
        refused = [c[0] for c, out in zip(mixed, outs) if isinstance(out, Exception)]
        assert refused == ([c[0] for c in battery() if c[2] == MISMATCHED] if kind == "lossless" else []), (kind, refused)


def test_png_equals_pillow(api):
    check_png_equals_pillow(api)


def test_lossy_equals_oracle(api):
    check_lossy_equals_oracle(api)


def test_lossless_equals_oracle(api):
    check_lossless_equals_oracle(api)


def test_batch_equals_file_by_file(api):
    check_batch_equals_file_by_file(api)
