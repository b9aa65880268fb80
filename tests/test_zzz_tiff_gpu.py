"""TIFF inputs with CSH_TIFF set on the MI355X: the cases of tests/test_tiff_emul.py through the product library (the decoders' tap against the model, the output's
bytes against the Python statement of its rule, libtiff as a witness, metadata, fallbacks, errors, routing, the CLI)."""
import os

import pytest

import test_tiff_emul as E
from _util import ROOT, product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600, method="thread")]
PRODUCT_CLI = os.path.join(ROOT, "caesium-clt_amd", "bin", "caesiumclt")


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_decoder_tap_equals_the_model(api):
    E.check_decoder(api)


def test_outputs_equal_the_model_and_decode_to_the_input(api, monkeypatch):
    E.check_outputs(api, monkeypatch)


def test_decoder_reads_what_libtiff_writes(api):
    E.check_pillow_files(api)


def test_metadata_is_kept_under_keep_metadata_only(api):
    E.check_metadata(api)


def test_fallbacks_return_the_input(api):
    E.check_fallbacks(api)


def test_malformed_files_fail_alone(api):
    E.check_malformed(api)


def test_routing_under_each_setting(api, monkeypatch):
    E.check_routing(api, monkeypatch)


def test_cli_compresses_tiff_files_under_the_variable_only(api, tmp_path):
    assert os.path.exists(PRODUCT_CLI), "caesium-clt_amd/bin/caesiumclt is not built (python -c 'import __graft_entry__ as g; g.build()')"
    E.run_cli_over_tiffs(PRODUCT_CLI, tmp_path)
