"""The level-0 coefficient lists built inside the forward-DCT kernels (k_pixel.hip nzf_*) on the MI355X, through the C ABI: every file
equals the oracle's and equals the same call under CSH_NZ_FUSED=0, and csh_timing.n_fused_lists says which path ran.  Bodies shared
with tests/test_fused_lists_emul.py."""
import pytest

import test_fused_lists_emul as E
from _util import product_api
from gen_synth import synth_jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


@pytest.mark.parametrize("prof", E.PROFILES)
def test_layouts(api, monkeypatch, prof):
    E.check_layouts(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_dense_blocks(api, monkeypatch, prof):
    E.check_dense_blocks(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_clipped_highlights(api, monkeypatch, prof):
    E.check_clipped_highlights(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_baseline_needs_no_list(api, monkeypatch, prof):
    E.check_baseline_needs_no_list(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_run_twice_and_rerun(api, monkeypatch, prof):
    E.check_run_twice_and_rerun(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_max_size(api, monkeypatch, prof):
    E.check_max_size(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_pools_that_overflow(api, monkeypatch, prof):
    E.check_pools_that_overflow(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", E.PROFILES)
def test_1080p_and_a_wide_batch(api, monkeypatch, prof):
    """the bench's size (every component aligned: 32 400 luma blocks, 127 chunks, the last one partial) next to files whose luma falls back"""
    E.set_profile(monkeypatch, prof)
    cases = [(1920, 1080, 0), (1920, 1080, 0)] + [(640 + 8 * (i % 3), 480, 3 * i) for i in range(10)]
    srcs = [synth_jpeg(30 + i, w, h, texture=tex) for i, (w, h, tex) in enumerate(cases)]
    E.check_group(api, monkeypatch, srcs, [c[0] for c in cases], 420)
