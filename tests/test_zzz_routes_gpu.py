"""The routes behind the C entry points on the MI355X: the mixed compress and convert batches of tests/test_routes_emul.py (one file per kind, no picture larger
than 64 x 48) through the product library -- the hipcc build of capi.cpp and route_*.cpp must route as the emulation build does."""
import pytest

import test_routes_emul as E
from _util import product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


@pytest.mark.parametrize("kw", E.COMPRESS_CALLS, ids=["lossy", "optimize", "webp_lossless"])
def test_mixed_compress_batch(api, kw):
    E.test_emul_mixed_compress_batch(api, kw)


@pytest.mark.parametrize("fmt,kw", E.CONVERT_CALLS, ids=["webp", "webp_lossless", "png_optimize", "png_lossy", "jpeg"])
def test_mixed_convert_batch_takes_every_route(api, fmt, kw):
    E.test_emul_mixed_convert_batch_takes_every_route(api, fmt, kw)


def test_every_batch_entry_point_without_a_results_array(api):
    E.test_emul_every_batch_entry_point_without_a_results_array(api)
