"""The inflate catalogue (tests/_inflate_cases.py) on the MI355X: the checks of test_inflate_emul.py with four waves a workgroup, their
barriers and hand-overs, which the emulation build does not play."""
import zlib

import numpy as np
import pytest

import _deflate as D
import _inflate_cases as IC
from _util import package, product_api
from oracle import oracle as O
from test_inflate_emul import check_catalogue

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_inflate_catalogue(api):
    check_catalogue(api, IC.cached_valid(), IC.cached_invalid())


def test_worst_convergence_alone(api):
    """the worst-case convergence stream alone in a batch, after a zlib stream of a picture of the same size; prints the inflate's time
    (k_png_huff + k_png_lz77, device events) for each"""
    worst = next(c for c in IC.cached_valid() if c.name == "worst_convergence")
    row = np.random.default_rng(3).integers(0, 256, (1, worst.width), dtype=np.uint8)
    plain = D.png_file(zlib.compress(D.filter_rows(row, 1, [0]), 6), worst.width, 1, 0, 8)
    params = package().default_parameters(png_optimize=True, png_optimization_level=2)
    names = api.png_kernel_names()
    for name, png in (("zlib_row", plain), ("worst_convergence", worst.png)):
        b = api.png_batch([png], params)
        try:
            t = b.run()
            out = b.fetch()[0]
        finally:
            b.close()
        assert out == O.png_optimize(png, 2)[0], name
        print("%s: %s %.3f ms" % (name, names[0], t.kernel_ms[0]))
