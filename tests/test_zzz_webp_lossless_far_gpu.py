"""Lossless WebP with the match finder over the whole window (CSH_VP8L=far) on the MI355X: the cases of tests/test_webp_lossless_far_emul.py through the product
library, and the device's bytes against the emulation build's (the two builds share the kernels' source)."""
import os

import pytest

import test_webp_lossless_far_emul as F
from _util import ROOT, emul_api, product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800, method="thread")]
PRODUCT_CLI = os.path.join(ROOT, "caesium-clt_amd", "bin", "caesiumclt")


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_far_round_trip(api):
    F.run_round_trip(api)


def test_far_copy_is_found(api, capsys):
    with capsys.disabled():
        F.run_far_copy_found(api)


def test_far_copy_pays(api, capsys):
    with capsys.disabled():
        F.run_far_copy_pays(api)


def test_far_window_holds(api, capsys):
    with capsys.disabled():
        F.run_window(api)


def test_far_is_never_larger(api, capsys):
    with capsys.disabled():
        F.run_never_larger(api)


def test_the_other_modes_do_not_move(api):
    F.run_other_modes_untouched(api)


def test_far_batches(api):
    F.run_batch_shape(api)


def test_far_alph_chunk(api, capsys):
    with capsys.disabled():
        F.run_alph(api)


def test_far_through_the_cli(api, tmp_path):
    assert os.path.exists(PRODUCT_CLI), "caesium-clt_amd/bin/caesiumclt is not built (python -c 'import __graft_entry__ as g; g.build()')"
    F.run_cli(PRODUCT_CLI, api, tmp_path)


def test_device_writes_the_emulations_bytes_twice(api):
    """every picture of the far battery: the device's file equals the emulation build's byte for byte -- the chain is the same, whichever lane, wave or block came
    first -- and a second run on the device gives the same bytes"""
    names = [n for n, _ in F.pictures()]
    dev = F.outputs(api, "far")
    emu = F.outputs(emul_api(), "far")
    assert [n for n, d, e in zip(names, dev, emu) if d != e] == []
    with F.vp8l_mode("far"):
        again = api.cs_batch_compress(list(F.sources()), F.E.params(webp_lossless=True))
    assert [n for n, d, a in zip(names, dev, again) if d != a] == []
