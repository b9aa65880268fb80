"""EOB runs resolved per 64-block word (k_entropy.hip k_ac_runs_words) on the MI355X, through the C ABI: every file of every case equals the oracle's and
equals the same batch under CSH_AC_RUNS=slot, in the default, scalar and plain profiles.  Cases and bodies shared with tests/test_ac_runs_emul.py, which
also shows (on the emulation build's path counters) that each case takes the path it is named for."""
import pytest

import test_ac_runs_emul as E
from _util import product_api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


@pytest.mark.parametrize("name,prof", E.CASE_PROFILES)
def test_case(api, monkeypatch, name, prof):
    E.check_case(api, monkeypatch, name, prof)
