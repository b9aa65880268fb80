"""Grouped speculation of the parallel JPEG decoder (k_decode_par.hip k_dec_spec_group, CSH_DEC_GROUP) on the MI355X, through the C ABI: every file equals
the oracle's and equals the same call under CSH_DEC_GROUP=1, csh_timing.n_dec_group is what was asked for and n_dec_seeds the sum of
ceil(live sub-sequences / G) over the parallel-decoded scans and restart segments.  Bodies shared with tests/test_dec_group_emul.py."""
import pytest

import test_dec_group_emul as E
from _util import product_api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


@pytest.mark.parametrize("G", E.GROUPS)
def test_group_edges(api, monkeypatch, G):
    E.check_group_edges(api, monkeypatch, G)


@pytest.mark.parametrize("G", E.GROUPS)
def test_restart_intervals(api, monkeypatch, G):
    E.check_restart_intervals(api, monkeypatch, G)


@pytest.mark.parametrize("G", E.GROUPS)
def test_streams_cut_short(api, monkeypatch, G):
    E.check_streams_cut_short(api, monkeypatch, G)


@pytest.mark.parametrize("G", E.GROUPS)
def test_progressive_first_scans(api, monkeypatch, G):
    E.check_progressive_first_scans(api, monkeypatch, G)


@pytest.mark.parametrize("G", E.GROUPS)
def test_label_creep(api, monkeypatch, G):
    E.check_label_creep(api, monkeypatch, G)


@pytest.mark.parametrize("G", E.GROUPS)
def test_slow_synchronisation(api, monkeypatch, G):
    E.check_slow_synchronisation(api, monkeypatch, G)


@pytest.mark.parametrize("G", E.GROUPS)
def test_reruns(api, monkeypatch, G):
    E.check_reruns(api, monkeypatch, G)
