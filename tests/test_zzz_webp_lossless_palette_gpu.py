"""Lossless WebP with the colour-indexing transform (CSH_VP8L=palette) on the MI355X: the cases of tests/test_webp_lossless_palette_emul.py through the product
library, and the device's bytes against the emulation build's (the two builds share the kernels' source)."""
import os

import pytest

import test_webp_lossless_palette_emul as P
from _util import ROOT, emul_api, product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800, method="thread")]
PRODUCT_CLI = os.path.join(ROOT, "caesium-clt_amd", "bin", "caesiumclt")


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_palette_round_trips(api):
    P.run_round_trip(api)


@pytest.mark.parametrize("name", P.TOOL_CASES)
def test_palette_tool_use(api, name):
    P.run_tool_use(api, name)


def test_palette_copies_use_the_packed_width(api):
    P.run_packed_distances(api)


def test_palette_is_never_larger_and_is_refs_without_a_palette(api, capsys):
    with capsys.disabled():
        P.run_never_larger(api)


def test_palette_meets_the_literals_only_bound(api, capsys):
    with capsys.disabled():
        P.run_bound(api)


def test_default_plain_and_refs_do_not_move(api):
    P.run_default_untouched(api)


def test_palette_alpha_forms_from_png(api):
    P.run_alpha_forms(api)


def test_palette_alph_chunk(api, capsys):
    with capsys.disabled():
        P.run_alph(api)


def test_palette_through_the_cli(api, tmp_path):
    assert os.path.exists(PRODUCT_CLI), "caesium-clt_amd/bin/caesiumclt is not built (python -c 'import __graft_entry__ as g; g.build()')"
    P.run_cli(PRODUCT_CLI, tmp_path)


def test_palette_batches_of_every_shape(api):
    P.run_batch_shape(api)


def test_device_writes_the_emulations_bytes_twice(api):
    """every picture of the palette battery: the device's file equals the emulation build's byte for byte, and a second run on the device gives the same bytes
    (the count is a set's size and the palette is sorted by value, so no lane's or wave's order shows)"""
    names = [n for n, _, _ in P.pictures()]
    dev = P.outputs(api, "palette")
    emu = P.outputs(emul_api(), "palette")
    assert [n for n, d, e in zip(names, dev, emu) if d != e] == []
    with P.vp8l_mode("palette"):
        again = api.cs_batch_compress(list(P.sources()), P.E.params(webp_lossless=True))
    assert [n for n, d, a in zip(names, dev, again) if d != a] == []
