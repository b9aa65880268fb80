"""The refinement kernels at the edges of what their LDS holds (k_aclist.hip k_list_refine and k_list_refine_pack: the round of 256 tokens, the 32-code table,
the 17-word histogram) on the MI355X, through the C ABI: every file equals the oracle's and equals the same call under CSH_REF_PACK=0.  Bodies shared with
tests/test_ref_lds_emul.py."""
import pytest

import test_ref_lds_emul as E
from _util import product_api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


@pytest.mark.parametrize("prof", E.PROFILES)
def test_most_tokens(api, monkeypatch, prof):
    E.check_most_tokens(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_most_bits(api, monkeypatch, prof):
    E.check_most_bits(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_mixed(api, monkeypatch, prof):
    E.check_mixed(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_alphabet(api, monkeypatch, prof):
    E.check_alphabet(api, monkeypatch, prof)
