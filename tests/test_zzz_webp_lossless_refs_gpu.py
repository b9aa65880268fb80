"""Lossless WebP with backward references and a colour cache (CSH_VP8L=refs) on the MI355X: the cases of tests/test_webp_lossless_refs_emul.py through the
product library, and the comparison that counts for kernels whose source the two builds share -- the device's bytes against the emulation build's."""
import os

import pytest

import test_webp_lossless_refs_emul as R
from _util import ROOT, emul_api, product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800, method="thread")]
PRODUCT_CLI = os.path.join(ROOT, "caesium-clt_amd", "bin", "caesiumclt")


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_refs_round_trip_through_libwebp(api):
    R.run_round_trip(api)


def test_refs_stream_uses_the_tools(api):
    R.run_tools(api)


def test_refs_sizes(api, capsys):
    with capsys.disabled():
        R.run_sizes(api)


def test_default_is_untouched_and_unknown_values_fail(api):
    R.run_default_untouched(api)


def test_refs_conversions_from_png_and_jpeg(api):
    R.run_conversions(api)


def test_refs_alph_chunk(api):
    R.run_alph(api)


def test_refs_through_the_cli(api, tmp_path):
    assert os.path.exists(PRODUCT_CLI), "caesium-clt_amd/bin/caesiumclt is not built (python -c 'import __graft_entry__ as g; g.build()')"
    R.run_cli(PRODUCT_CLI, tmp_path)


def test_device_writes_the_emulations_bytes_twice(api):
    """every battery picture: the device's refs file equals the emulation build's byte for byte, and a second run on the device gives the same bytes (the
    hashed candidate and the cache are defined by position, never by which lane's store landed last)"""
    names = [n for n, _ in R.battery()]
    dev = R.outputs(api, "refs")
    emu = R.outputs(emul_api(), "refs")
    assert [n for n, d, e in zip(names, dev, emu) if d != e] == []
    with R.vp8l_mode("refs"):
        again = api.cs_batch_compress([s for _, s in R.battery()], R.E.params(webp_lossless=True))
    assert [n for n, d, a in zip(names, dev, again) if d != a] == []
