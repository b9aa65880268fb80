"""The quantised AC levels that live in the coefficient lists alone (PlaneWork::ac_lists) on the MI355X, through the C ABI: every file equals
the oracle's and equals the same call under CSH_AC_TILES=1, over poisoned tiles too, csh_timing.n_ac_in_lists says which path ran, and the
debug tap returns the final coefficients.  Bodies shared with tests/test_ac_tiles_emul.py."""
import pytest

import test_ac_tiles_emul as E
import test_fused_lists_emul as F
from _util import product_api
from gen_synth import synth_jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


@pytest.mark.parametrize("prof", E.PROFILES)
def test_bytes(api, monkeypatch, prof):
    E.check_bytes(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_bytes_over_poisoned_tiles(api, monkeypatch, prof):
    E.check_bytes(api, monkeypatch, prof, poison=True)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_fallback_switches(api, monkeypatch, prof):
    E.check_fallback_switches(api, monkeypatch, prof)


def test_tap(api, monkeypatch):
    E.check_tap(api, monkeypatch)


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_reruns(api, monkeypatch, prof):
    E.check_reruns(api, monkeypatch, prof)


def test_to_size(api, monkeypatch):
    E.check_to_size(api, monkeypatch)


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_dense_and_overflowing(api, monkeypatch, prof):
    E.check_dense_and_overflowing(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_1080p_and_a_wide_batch(api, monkeypatch, prof):
    """the bench's size (every component flagged: 32 400 luma blocks, 127 chunks, the last one partial) next to files whose luma keeps its tile"""
    F.set_profile(monkeypatch, prof)
    cases = [(1920, 1080, 0), (1920, 1080, 0)] + [(640 + 8 * (i % 3), 480, 3 * i) for i in range(10)]
    srcs = [synth_jpeg(30 + i, w, h, texture=tex) for i, (w, h, tex) in enumerate(cases)]
    E.check_group(api, monkeypatch, srcs, [c[0] for c in cases], 420)
