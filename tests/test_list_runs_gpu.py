"""List runs (k_aclist.hip: one wave of k_list_stats, k_list_pack and k_list_refine per run of up to CSH_LIST_RUN chunks) on the MI355X, through the C ABI:
every file equals the oracle's and equals the same call under CSH_LIST_RUN=1, and csh_timing.n_list_runs is the sum of ceil(chunks / R) over the work items
coded from the lists.  Bodies shared with tests/test_list_runs_emul.py."""
import pytest

import test_list_runs_emul as E
from _util import product_api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


@pytest.mark.parametrize("R", (2, 3))
@pytest.mark.parametrize("prof", E.PROFILES)
def test_boundaries(api, monkeypatch, prof, R):
    E.check_boundaries(api, monkeypatch, prof, R)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_default_run(api, monkeypatch, prof):
    E.check_default_run(api, monkeypatch, prof)


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", E.PROFILES)
def test_layouts(api, monkeypatch, prof, R):
    E.check_layouts(api, monkeypatch, prof, R)


@pytest.mark.parametrize("R", (3, None))
@pytest.mark.parametrize("prof", E.PROFILES)
def test_dense_window(api, monkeypatch, prof, R):
    E.check_dense_window(api, monkeypatch, prof, R)


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", E.PROFILES)
def test_flat(api, monkeypatch, prof, R):
    E.check_flat(api, monkeypatch, prof, R)


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", (None, "scalar"))
def test_gated_stage(api, monkeypatch, prof, R):
    E.check_gated_stage(api, monkeypatch, prof, R)


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", E.PROFILES)
def test_pools_that_overflow(api, monkeypatch, prof, R):
    E.check_pools_that_overflow(api, monkeypatch, prof, R)


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", E.PROFILES)
def test_reruns(api, monkeypatch, prof, R):
    E.check_reruns(api, monkeypatch, prof, R)


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", E.PROFILES)
def test_sequential(api, monkeypatch, prof, R):
    E.check_sequential(api, monkeypatch, prof, R)
