"""CMYK, YCCK and RGB-colourspace JPEG inputs on the MI355X, through the C ABI: the bodies of test_jpeg_spaces_emul.py.  Every body runs under a
time limit of its own: a C call that does not return in time ends the process (faulthandler)."""
import contextlib
import faulthandler

import pytest

import test_jpeg_spaces_emul as bodies
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


def test_lossless_transcode(api):
    with time_limit(120):
        bodies.check_lossless(api)


def test_plain_profile_equals_libjpeg_turbo(api):
    with time_limit(120):
        bodies.check_plain_equals_libjpeg(api)


@pytest.mark.parametrize("prof", [None, "scalar"], ids=["default", "scalar"])
def test_profile_equals_oracle_per_component(api, prof):
    with time_limit(120):
        bodies.check_profile_equals_oracle(api, prof)


def test_to_png_equals_pillow_rgb(api):
    with time_limit(120):
        bodies.check_png(api)


def test_to_webp_and_resized_jpeg(api):
    with time_limit(120):
        bodies.check_webp_and_resized_jpeg(api)


def test_max_size(api):
    with time_limit(120):
        bodies.check_max_size(api)


def test_mixed_batch_equals_file_by_file(api):
    with time_limit(120):
        bodies.check_mixed_batch(api)
