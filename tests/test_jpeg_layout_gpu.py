"""Every integral sampling layout and 4:1:1 output on the MI355X, through the C ABI and the caesiumclt binary, against the oracle byte for byte
(the emulation build runs the full matrix: test_jpeg_layout_emul.py).  Every GPU step runs under a time limit of its own: a C call that does
not return in time ends the process (faulthandler), the CLI runs under subprocess's timeout."""
import contextlib
import faulthandler
import os
import subprocess

import pytest

from _jpeg_layout import LAYOUTS, layout_jpeg
from _util import ROOT, oracle_jpeg_to_png, oracle_lossy, oracle_resized, package, product_api
from gen_synth import synth_jpeg

pytestmark = pytest.mark.gpu
PNG = 1


@contextlib.contextmanager
def time_limit(seconds):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def api():
    a = product_api()
    if a.device_count() < 1:
        pytest.fail("no HIP device visible")
    return a


def params(**kw):
    return package().default_parameters(**kw)


@pytest.mark.parametrize("ss", [0, 444, 411])
def test_layouts_equal_oracle(api, ss):
    srcs = [layout_jpeg(k, w, h, n) for k, n in enumerate(sorted(LAYOUTS)) for (w, h) in ((3, 5), (33, 17), (101, 67))]
    with time_limit(120):
        outs = api.batch_compress(srcs, params(jpeg_chroma_subsampling=ss))
    assert outs == [oracle_lossy(s, subsampling=ss or 420) for s in srcs]


def test_resize_and_png_equal_oracle(api):
    srcs = [layout_jpeg(10 + k, 101, 67, n) for k, n in enumerate(sorted(LAYOUTS))]
    with time_limit(120):
        sized = api.batch_compress(srcs, params(width=60, jpeg_chroma_subsampling=411))
        pngs = api.batch_convert(srcs, params(png_optimize=True), PNG)
    assert sized == [oracle_resized(s, 60, 0, subsampling=411) for s in srcs]
    assert pngs == [oracle_jpeg_to_png(s, True) for s in srcs]


def test_large_batches(api):
    """64 files a batch: a 1920 x 1080 4:2:0 camera picture to 4:1:1 (the vector path), a 1080 x 1920 4:4:0 one to auto, small files of
    every layout around them"""
    small = [layout_jpeg(20 + k, 40 + 3 * k, 24 + k, sorted(LAYOUTS)[k % len(LAYOUTS)]) for k in range(63)]
    cam = synth_jpeg(5, 1920, 1080, fast=True)
    a = small[:31] + [cam] + small[31:]
    with time_limit(180):
        outs = api.batch_compress(a, params(jpeg_chroma_subsampling=411))
    assert len(outs) == 64 and outs[31] == oracle_lossy(cam, subsampling=411)
    assert outs == [oracle_lossy(s, subsampling=411) for s in a]
    tall = layout_jpeg(6, 1080, 1920, "440")
    b = [tall] + small
    with time_limit(180):
        outs = api.batch_compress(b, params())
    assert outs[0] == oracle_lossy(tall)
    assert outs == [oracle_lossy(s) for s in b]


def test_cli_tree_at_411(tmp_path):
    cli = os.path.join(ROOT, "caesium-clt_amd", "bin", "caesiumclt")
    src_root = tmp_path / "in"
    files = {}
    for k, n in enumerate(sorted(LAYOUTS)):
        rel = os.path.join(f"d{k % 3}", f"{n}.jpg")
        files[rel] = layout_jpeg(150 + k, 90 + 7 * k, 50 + 3 * k, n)
    files["cam.jpg"] = synth_jpeg(7, 320, 240, texture=10)
    for rel, data in files.items():
        p = src_root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(data)
    out = tmp_path / "out"
    r = subprocess.run([cli, "-q", "80", "--jpeg-chroma-subsampling", "4:1:1", "-R", "-S", "-o", str(out), str(src_root)],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    for rel, data in files.items():
        assert (out / rel).read_bytes() == oracle_lossy(data, quality=80, subsampling=411), rel
