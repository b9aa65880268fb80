"""The oracle's statement of the JPEG path for sampling layouts beyond 4:4:4 / 4:2:2 / 4:2:0 (CPU only; passes without the device library).

Decoder side, live-pinned: files of tests/_jpeg_layout.py's writer (4:4:0, 4:1:1, 4:1:0, luma 3x1 and 1x4, Cb and Cr sampled differently),
baseline, with restart markers and as progressive transcodes, decode to the same YCbCr samples in the oracle and in libjpeg-turbo (Pillow,
draft("YCbCr"): libjpeg-turbo's own upsampling, no colour conversion).

Encoder side, model-checked: Pillow cannot write 4:1:1 (JpegImagePlugin maps "4:1:1" to 4:2:0), so the oracle's 4:1:1 chroma samples are
checked against a numpy statement of jcsample.c's int_downsample (right-edge expansion, then (sum of 4 + 2) >> 2), not against a live
libjpeg."""
import io

import numpy as np
import pytest

from _jpeg_layout import LAYOUTS, layout_jpeg
from _util import oracle_lossless

PIL = pytest.importorskip("PIL.Image")
SIZES = [(101, 67), (17, 9), (3, 5)]


def libjpeg_ycc(src):
    im = PIL.open(io.BytesIO(src))
    im.draft("YCbCr", im.size)
    return np.asarray(im)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_writer_files_decode_alike_in_oracle_and_libjpeg(name):
    from oracle import oracle as O
    for k, (w, h) in enumerate(SIZES):
        for ri in (0, 2):
            src = layout_jpeg(30 + k, w, h, name, restart_interval=ri)
            sof = src.index(b"\xff\xc0")
            assert src[sof + 11] >> 4 == LAYOUTS[name][0][0] and src[sof + 11] & 15 == LAYOUTS[name][0][1]
            for f in (src, oracle_lossless(src, progressive=1)):
                want = libjpeg_ycc(f)
                assert want.shape == (h, w, 3)
                assert np.array_equal(O.decode(f).pixels(), want), (name, w, h, ri, f is src)


def int_downsample_411(full):
    """jcsample.c for a 4x1 component: columns padded to the block width by repeating the last one, (sum of 4 + 2) >> 2"""
    h, w = full.shape
    pw = -(-(-(-w // 4)) // 8) * 8
    cols = np.minimum(np.arange(4 * pw), w - 1)
    return (full[:, cols].reshape(h, pw, 4).astype(np.int64).sum(axis=2) + 2) >> 2


@pytest.mark.parametrize("name", ["420", "440", "411", "y14", "y21_cb12_cr11"])
def test_oracle_411_chroma_is_int_downsample(name):
    from oracle import oracle as O
    for k, (w, h) in enumerate(SIZES + [(33, 17), (250, 130)]):
        src = layout_jpeg(40 + k, w, h, name)
        full = O.decode(src).pixels()
        comps = O.trellis_inputs(src, O.params(quality=80, progressive=1, subsampling=411, qtable_profile=3, marker_style=1, scan_script=2))
        assert [(c["h"], c["v"]) for c in comps] == [(4, 1), (1, 1), (1, 1)]
        for c in (1, 2):
            t = comps[c]
            model = int_downsample_411(full[:, :, c])
            rb, cb = t["real_bh"], t["real_bw"]
            got = t["samples"][:rb, :cb].reshape(rb, cb, 8, 8).transpose(0, 2, 1, 3).reshape(rb * 8, cb * 8)
            rows = np.minimum(np.arange(rb * 8), h - 1)   # rows below the last replicate it
            assert np.array_equal(got, model[rows][:, :cb * 8]), (name, w, h, c)
        luma = comps[0]
        got = luma["samples"][:luma["real_bh"], :luma["real_bw"]].reshape(luma["real_bh"], luma["real_bw"], 8, 8).transpose(0, 2, 1, 3)
        got = got.reshape(luma["real_bh"] * 8, luma["real_bw"] * 8)
        assert np.array_equal(got[:h, :w], full[:, :, 0])
