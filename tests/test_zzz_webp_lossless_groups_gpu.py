"""Lossless WebP with the meta prefix (entropy) image (CSH_VP8L=groups) on the MI355X: the cases of tests/test_webp_lossless_groups_emul.py through the product
library, and the device's bytes against the emulation build's (the two builds share the kernels' source)."""
import os

import pytest

import test_webp_lossless_groups_emul as G
from _util import ROOT, emul_api, product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800, method="thread")]
PRODUCT_CLI = os.path.join(ROOT, "caesium-clt_amd", "bin", "caesiumclt")


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_groups_round_trip(api):
    G.run_round_trip(api)


def test_groups_tool_use(api, capsys):
    with capsys.disabled():
        G.run_tool_use(api)


def test_groups_are_never_larger(api, capsys):
    with capsys.disabled():
        G.run_never_larger(api)


def test_groups_pay(api, capsys):
    with capsys.disabled():
        G.run_pays(api)


def test_the_other_modes_do_not_move(api):
    G.run_other_modes_untouched(api)


def test_groups_batches(api):
    G.run_batch_shape(api)


def test_groups_alph_chunk(api, capsys):
    with capsys.disabled():
        G.run_alph(api)


def test_groups_through_the_cli(api, tmp_path):
    assert os.path.exists(PRODUCT_CLI), "caesium-clt_amd/bin/caesiumclt is not built (python -c 'import __graft_entry__ as g; g.build()')"
    G.run_cli(PRODUCT_CLI, api, tmp_path)


def test_device_writes_the_emulations_bytes_twice(api):
    """every picture of the groups battery: the device's file equals the emulation build's byte for byte -- the labels are the same, whichever lane or wave came
    first -- and a second run on the device gives the same bytes"""
    names = [n for n, _ in G.pictures()]
    dev = G.outputs(api, "groups")
    emu = G.outputs(emul_api(), "groups")
    assert [n for n, d, e in zip(names, dev, emu) if d != e] == []
    with G.vp8l_mode("groups"):
        again = api.cs_batch_compress(list(G.sources()), G.E.params(webp_lossless=True))
    assert [n for n, d, a in zip(names, dev, again) if d != a] == []
