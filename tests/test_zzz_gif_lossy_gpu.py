"""GIF inputs under CSH_GIF=lossy on the MI355X: the checks of tests/test_gif_lossy_emul.py through the product library (the candidate rows against the model's
lists, the route's bytes against the model's, the rendering bound, sizes, routing, the CLI)."""
import os

import pytest

import test_gif_lossy_emul as L
from _util import ROOT, product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600, method="thread")]
PRODUCT_CLI = os.path.join(ROOT, "caesium-clt_amd", "bin", "caesiumclt")


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_near_tap_equals_the_model(api):
    L.check_near_taps(api)


def test_ramp_outputs_equal_the_model_within_the_bound(api):
    L.check_ramp(api)


def test_cube_outputs_under_the_cut_and_a_full_table(api):
    L.check_cube(api)


def test_chunk_seams(api, monkeypatch):
    L.check_seams(api, monkeypatch)


def test_disposal_cases(api):
    L.check_disposals(api)


def test_routing_under_lossy(api, monkeypatch):
    L.check_routing(api, monkeypatch)


def test_cli_under_lossy(api, tmp_path):
    assert os.path.exists(PRODUCT_CLI), "caesium-clt_amd/bin/caesiumclt is not built (python -c 'import __graft_entry__ as g; g.build()')"
    L.run_cli_over_a_gif(PRODUCT_CLI, tmp_path)
