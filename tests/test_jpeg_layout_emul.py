"""Every integral sampling layout on the JPEG pixel path, and 4:1:1 output: the emulation build against the oracle, byte for byte.

Inputs are tests/_jpeg_layout.py files (4:4:0, 4:1:1, 4:1:0, luma 3x1 / 1x4, Cb and Cr sampled differently, 4:2:0 as a control) at sizes
around the 32-pixel 4:1:1 MCU; outputs are every --jpeg-chroma-subsampling value, and the resize, size-targeting, JPEG -> PNG / WebP and
PNG -> JPEG paths.  Layouts libjpeg refuses (more than 10 blocks per MCU, ratios that are not whole numbers) still answer 20101.
The MI355X runs a reduced matrix in test_jpeg_layout_gpu.py."""
import pytest

from _jpeg_layout import LAYOUTS, REFUSED, layout_jpeg
from _util import (emul_api, oracle_jpeg_to_png, oracle_jpeg_to_webp, oracle_lossless, oracle_lossy, oracle_png_to_jpeg, oracle_resized,
                   package)
from gen_synth import synth_jpeg, synth_png

SIZES = [(1, 1), (3, 5), (17, 9), (31, 8), (33, 17), (101, 67), (250, 130)]
JPEG, PNG, WEBP = 0, 1, 3


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


@pytest.fixture(scope="module")
def matrix():
    """every layout at every size; a progressive transcode and a restart-interval file of each layout at one size"""
    cases = [(f"{n}_{w}x{h}", layout_jpeg(k, w, h, n)) for k, n in enumerate(sorted(LAYOUTS)) for (w, h) in SIZES]
    for k, n in enumerate(sorted(LAYOUTS)):
        cases.append((f"{n}_prog", oracle_lossless(layout_jpeg(50 + k, 45, 29, n), progressive=1)))
        cases.append((f"{n}_rst", layout_jpeg(60 + k, 70, 41, n, restart_interval=3)))
    return cases


@pytest.mark.parametrize("ss", [0, 444, 422, 420, 411])
def test_every_layout_to_every_subsampling(api, matrix, ss):
    outs = api.batch_compress([c[1] for c in matrix], params(jpeg_chroma_subsampling=ss))
    for (name, src), out in zip(matrix, outs):
        assert not isinstance(out, Exception), (name, out)
        assert out == oracle_lossy(src, subsampling=ss or 420), (name, ss)


def test_411_output_from_ordinary_inputs(api):
    """the hot case (a 4:2:0 camera file to 4:1:1) and 4:4:4 / 4:2:2 inputs; widths on every side of the vector path's edges"""
    srcs = [synth_jpeg(3 + i, w, h, subsampling=ss, texture=20) for i, (w, h, ss) in
            enumerate([(320, 240, 2), (333, 101, 2), (64, 64, 2), (47, 33, 2), (8, 8, 2), (130, 77, 0), (161, 97, 1)])]
    outs = api.batch_compress(srcs, params(jpeg_chroma_subsampling=411))
    assert outs == [oracle_lossy(s, subsampling=411) for s in srcs]
    # the sequential (baseline) output script too
    from oracle import oracle as O
    from _util import device_quantiser, device_scan_script
    out = api.compress_in_memory(srcs[0], params(jpeg_chroma_subsampling=411, jpeg_progressive=False))
    assert out == O.jpeg_compress(srcs[0], O.params(quality=80, progressive=0, subsampling=411, qtable_profile=3, marker_style=1,
                                                    scan_script=device_scan_script(), **device_quantiser()))


@pytest.mark.parametrize("ss", [0, 411, 444])
def test_resize(api, ss):
    for k, n in enumerate(sorted(LAYOUTS)):
        src = layout_jpeg(70 + k, 101, 67, n)
        for w, h in ((60, 0), (0, 90)):
            assert api.compress_in_memory(src, params(width=w, height=h, jpeg_chroma_subsampling=ss)) == oracle_resized(src, w, h, subsampling=ss or 420), (n, w, h)


def test_max_size(api):
    from test_pipeline_emul import reference_size_walk
    srcs = [layout_jpeg(80 + k, 120, 90, n) for k, n in enumerate(sorted(LAYOUTS))]
    for ss in (0, 411):
        target = 3000
        outs = api.batch_compress_to_size(srcs, params(jpeg_chroma_subsampling=ss), target)
        for n, src, out in zip(sorted(LAYOUTS), srcs, outs):
            want = reference_size_walk(src, target, encode=lambda s, q: oracle_lossy(s, q, subsampling=ss or 420))[1]
            assert out == want, (n, ss)


def test_jpeg_to_png_and_webp(api):
    cases = [layout_jpeg(90 + k, w, h, n) for k, n in enumerate(sorted(LAYOUTS)) for (w, h) in ((33, 17), (101, 67))]
    assert api.batch_convert(cases, params(png_optimize=True), PNG) == [oracle_jpeg_to_png(s, True) for s in cases]
    assert api.batch_convert(cases, params(png_optimize=False), PNG) == [oracle_jpeg_to_png(s, False) for s in cases]
    assert api.batch_convert(cases, params(webp_quality=80), WEBP) == [oracle_jpeg_to_webp(s, 80) for s in cases]
    assert api.batch_convert(cases[:4], params(webp_quality=75, width=40), WEBP) == [oracle_jpeg_to_webp(s, 75, 40) for s in cases[:4]]


def test_png_to_jpeg_411(api):
    pngs = [synth_png(100 + k, w, h, mode) for k, (w, h, mode) in enumerate([(97, 61, "RGB"), (33, 17, "RGBA"), (3, 5, "RGB"), (64, 48, "L")])]
    assert api.batch_convert(pngs, params(jpeg_chroma_subsampling=411), JPEG) == [oracle_png_to_jpeg(s, subsampling=411) for s in pngs]
    assert api.batch_convert(pngs[:2], params(jpeg_chroma_subsampling=411, width=50), JPEG) == [oracle_png_to_jpeg(s, width=50, subsampling=411) for s in pngs[:2]]


def test_mixed_batch_keeps_order_and_results(api):
    """one cs_batch_compress call: every layout between ordinary 4:2:0 files, a refused layout and a file that is no image"""
    blobs, want = [], []
    for k, n in enumerate(sorted(LAYOUTS)):
        a = synth_jpeg(110 + k, 64 + 8 * k, 48, texture=10)
        s = layout_jpeg(120 + k, 57 + 4 * k, 35, n)
        blobs += [a, s]
    blobs.insert(5, layout_jpeg(130, 40, 24, "11_blocks"))
    blobs.append(b"not an image")
    for ss in (0, 411):
        outs = api.cs_batch_compress(blobs, params(jpeg_chroma_subsampling=ss))
        assert len(outs) == len(blobs)
        for i, (src, out) in enumerate(zip(blobs, outs)):
            if i == 5:
                assert isinstance(out, Exception) and out.code == 20101
            elif i == len(blobs) - 1:
                assert isinstance(out, Exception)
            else:
                assert out == oracle_lossy(src, subsampling=ss or 420), (i, ss)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_layouts_answer_20101(api, name):
    src = layout_jpeg(140, 40, 24, name)
    for ss in (0, 411):
        with pytest.raises(package().CaesiumError) as e:
            api.compress_in_memory(src, params(jpeg_chroma_subsampling=ss))
        assert e.value.code == 20101
    with pytest.raises(package().CaesiumError) as e:
        api.convert_in_memory(src, params(), PNG)
    assert e.value.code == 20101
