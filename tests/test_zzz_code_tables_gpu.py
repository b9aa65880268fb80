"""The prefix codes in the files the product library writes on the MI355X follow from the symbols those files code: the checks of
tests/test_code_tables_emul.py (every DEFLATE block, every lossless WebP code, every table of a baseline JPEG against tests/_prefix_model.py) through
libcaesium_hip.so.  No device FAILS: nothing here skips."""
import pytest

import test_code_tables_emul as T
from _util import product_api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_deflate_tables(api, capsys):
    with capsys.disabled():
        T.run_deflate(api)


def test_vp8l_tables(api, capsys):
    with capsys.disabled():
        T.run_vp8l(api)


def test_jpeg_tables(api, capsys):
    with capsys.disabled():
        T.run_jpeg(api)
