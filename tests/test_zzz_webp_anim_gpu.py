"""Animated WebP inputs on the MI355X: the cases of tests/test_webp_anim_emul.py through the product library (canvases pinned to libwebp's AnimDecoder via
Pillow, the output to the fixed rule and to the still path's bytes)."""
import os

import pytest

import test_webp_anim_emul as E
from _util import ROOT, product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900, method="thread")]
PRODUCT_CLI = os.path.join(ROOT, "caesium-clt_amd", "bin", "caesiumclt")


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_canvases_equal_libwebp(api):
    E.test_emul_canvases_equal_libwebp(api)


def test_lossless_run_keeps_canvases_and_follows_the_rule(api):
    E.test_emul_lossless_run_keeps_canvases_and_follows_the_rule(api)


@pytest.mark.parametrize("quality", [35, 85])
def test_lossy_run_follows_the_rule_and_codes_like_the_still_path(api, quality):
    E.test_emul_lossy_run_follows_the_rule_and_codes_like_the_still_path(api, quality)


def test_damaged_animations_fail_alone(api):
    E.test_emul_damaged_animations_fail_alone(api)


def test_metadata_is_carried_under_keep_metadata(api):
    E.test_emul_metadata_is_carried_under_keep_metadata(api)


def test_compress_to_size_on_an_animation(api):
    E.test_emul_compress_to_size_on_an_animation(api)


def test_lossless_run_with_the_far_coder(api, monkeypatch):
    E.test_emul_lossless_run_with_the_far_coder(api, monkeypatch)


def test_cli_takes_a_tree_with_an_animation(api, tmp_path):
    assert os.path.exists(PRODUCT_CLI), "caesium-clt_amd/bin/caesiumclt is not built (python -c 'import __graft_entry__ as g; g.build()')"
    E.run_cli_over_a_tree(PRODUCT_CLI, tmp_path)
