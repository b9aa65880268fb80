"""The rescue paths of the parallel JPEG decoder (k_dec_mark_pending, k_dec_dense<3>, k_dec_chain, the hand-over to the sequential kernel) on the MI355X,
through the C ABI, reached with the list rounds capped by CSH_TEST_DEC_ROUNDS: every file equals the oracle's and the same call without the cap, the
counters of csh_timing agree with each other, and with no round at all the label chain has run for every input.  Which scans the chain settles depends on
the order the lanes ran in and is not asserted.  Bodies shared with tests/test_dec_rescue_emul.py."""
import pytest

import test_dec_rescue_emul as R
from _util import product_api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


@pytest.mark.parametrize("G", R.GROUPS)
@pytest.mark.parametrize("cap", R.CAPS)
@pytest.mark.parametrize("name", R.NAMES)
def test_rescue(api, monkeypatch, name, cap, G):
    R.check_rescue(api, monkeypatch, name, cap, G)


@pytest.mark.parametrize("G", R.GROUPS)
def test_labels_creep_and_lanes_walk(api, monkeypatch, G):
    R.check_creep(api, monkeypatch, G)
