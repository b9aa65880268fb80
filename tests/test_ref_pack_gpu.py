"""The AC refinement scans packed from the compacted coefficient lists, without tokens (k_aclist.hip k_list_refine<false> + k_list_refine_pack) on the MI355X,
through the C ABI: every file equals the oracle's and equals the same call under CSH_REF_PACK=0, and csh_timing.n_ref_packed says which path ran.  Bodies
shared with tests/test_ref_pack_emul.py."""
import pytest

import test_ref_pack_emul as E
from _util import product_api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


@pytest.mark.parametrize("prof", E.PROFILES)
def test_chunk_edges(api, monkeypatch, prof):
    E.check_chunk_edges(api, monkeypatch, prof)


@pytest.mark.parametrize("R", (1, 3, 8))
@pytest.mark.parametrize("prof", E.PROFILES)
def test_run_edges(api, monkeypatch, prof, R):
    E.check_run_edges(api, monkeypatch, prof, R)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_unaligned(api, monkeypatch, prof):
    E.check_unaligned(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_dense_blocks(api, monkeypatch, prof):
    E.check_dense_blocks(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_crafted(api, monkeypatch, prof):
    E.check_crafted(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_pending_bits(api, monkeypatch, prof):
    E.check_pending_bits(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_flat(api, monkeypatch, prof):
    E.check_flat(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_gated_stage(api, monkeypatch, prof):
    E.check_gated_stage(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_pools_that_overflow(api, monkeypatch, prof):
    E.check_pools_that_overflow(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_run_twice_and_rerun(api, monkeypatch, prof):
    E.check_run_twice_and_rerun(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_max_size(api, monkeypatch, prof):
    E.check_max_size(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_sequential(api, monkeypatch, prof):
    E.check_sequential(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", (None, "plain"))
def test_ref_list_off(api, monkeypatch, prof):
    E.check_ref_list_off(api, monkeypatch, prof)
