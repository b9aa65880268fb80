"""The Lanczos3 resize on the MI355X against the float64 model of image-rs (tests/_lanczos_model.py): the cases of
test_resize_model_emul.py through the product library -- every LDS cap side, forced and natural two-pass for JPEG and PNG sources,
16-bit multi-channel PNGs, extreme ratios, a batch of one wide picture and small ones, and lossless WebP from PNG sources.  Each output
sample passes the acceptance rule and each file equals the oracle's.  After the other device tests (the file name sorts last)."""
import pytest

import test_resize_model_emul as T
from _util import product_api

# a wedged kernel must end the run, not hold the box
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900, method="thread")]


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
@pytest.mark.parametrize("case", T.JPEG_CAP_CASES, ids=[c[0] for c in T.JPEG_CAP_CASES])
def test_jpeg_rows_at_the_lds_caps(api, case, forced):
    T.test_jpeg_rows_at_the_lds_caps(api, case, forced)


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
def test_jpeg_shapes_and_ratios(api, forced):
    T.test_jpeg_shapes_and_ratios(api, forced)


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
def test_jpeg_extreme_ratios(api, forced):
    T.test_jpeg_extreme_ratios(api, forced)


def test_jpeg_batch_of_one_wide_and_small_pictures(api):
    T.test_jpeg_batch_of_one_wide_and_small_pictures(api)


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
@pytest.mark.parametrize("kind", T.PNG_KINDS)
def test_png_every_kind_of_sample(api, kind, forced):
    T.test_png_every_kind_of_sample(api, kind, forced)


@pytest.mark.parametrize("forced", [False, True], ids=["natural", "two_pass"])
@pytest.mark.parametrize("case", T.PNG_CAP_CASES, ids=[c[0] for c in T.PNG_CAP_CASES])
def test_png_rows_at_the_lds_cap(api, case, forced):
    T.test_png_rows_at_the_lds_cap(api, case, forced)


def test_png_extreme_ratios_and_a_mixed_batch(api):
    T.test_png_extreme_ratios_and_a_mixed_batch(api)


def test_png_to_lossless_webp(api):
    T.test_png_to_lossless_webp(api)
