"""The oracle's decode of files whose DRI, DQT or DHT change between scans (tests/_jpeg_markers.py) against libjpeg-turbo through Pillow,
exactly -- before the library is compared with the oracle on the same files (test_jpeg_markers_emul.py, test_zzz_jpeg_markers_gpu.py).
Pillow is imported plainly: this judge has no skip path."""
import numpy as np
import pytest
from PIL import Image  # noqa: F401 - the judge; a missing Pillow is an error here, not a skip

from _jpeg_markers import MISMATCHED, battery, listed, oracle_rgb, pillow_rgb, same_coefficients
from _util import oracle_lossless, oracle_lossy
from oracle import oracle as O


def test_decode_pixels_equal_libjpeg_turbo_on_every_case():
    bad = []
    for name, data, _ in battery():
        got, want = oracle_rgb(data), pillow_rgb(data)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append((name, int(np.abs(got.astype(int) - want.astype(int)).max()) if got.shape == want.shape else "shape"))
    assert not bad, listed(bad)


def test_lossless_keeps_the_coefficients_or_refuses_mismatched_tables():
    bad = []
    for name, data, expect in battery():
        if expect == MISMATCHED:
            with pytest.raises(O.OracleError, match="unsupported"):
                oracle_lossless(data)
            assert oracle_lossy(data)   # only the coefficient transcode is refused
            continue
        a, b = O.decode(data), O.decode(oracle_lossless(data))
        if not same_coefficients(a, b) or not np.array_equal(a.pixels(), b.pixels()):
            bad.append(name)
    assert not bad, listed(bad)
