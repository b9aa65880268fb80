"""Files whose DRI, DQT or DHT change between two scans on the MI355X, through the C ABI: the bodies of test_jpeg_markers_emul.py.  Every body
runs under a time limit of its own: a C call that does not return in time ends the process (faulthandler)."""
import contextlib
import faulthandler

import pytest

import test_jpeg_markers_emul as bodies
from _util import product_api

pytestmark = pytest.mark.gpu


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
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_png_equals_pillow(api):
    with time_limit(120):
        bodies.check_png_equals_pillow(api)


def test_lossy_equals_oracle(api):
    with time_limit(120):
        bodies.check_lossy_equals_oracle(api)


def test_lossless_equals_oracle(api):
    with time_limit(120):
        bodies.check_lossless_equals_oracle(api)


def test_batch_equals_file_by_file(api):
    with time_limit(120):
        bodies.check_batch_equals_file_by_file(api)
