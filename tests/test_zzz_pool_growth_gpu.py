"""Output pools that overflow and grow, on the device: the bodies of test_pool_growth_emul.py through the product library, and one case only the device makes
meaningful -- waves of k_bool_code in which pieces that run out of room sit beside pieces that do not (the emulation runs lanes one at a time)."""
import pytest

import test_pool_growth_emul as T
from _util import oracle_jpeg_to_webp, product_api

# a wedged kernel must end the run, not hold the box (these files are last, so ending the process loses nothing after them)
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900, method="thread")]


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_webp_routes_grow_once_and_twice(api, monkeypatch):
    assert T.check_jpeg_to_webp_grows(api, monkeypatch) == [1, 2]
    assert T.check_jpeg_to_webp_grows(api, monkeypatch, width=260, nmb=T.macroblocks(260, 195)) == [1, 2]
    assert T.check_png_to_webp_grows(api, monkeypatch) == [1, 2, 2]
    assert T.check_png_with_alpha_grows(api, monkeypatch) == [1, 2]
    assert T.check_webp_to_webp_grows(api, monkeypatch) == [1, 2]


def test_mixed_batches_keep_files_and_failures(api, monkeypatch):
    assert T.check_mixed_jpeg_batch(api, monkeypatch) == 2
    assert T.check_mixed_png_batch(api, monkeypatch) == 2


def test_exhaustion_fails_the_large_file_alone(api, monkeypatch):
    T.check_exhaustion(api, monkeypatch)


def test_boolean_coder_in_pieces_under_overflow(api, monkeypatch):
    assert T.check_bool_pieces_under_overflow(api, monkeypatch) == [1, 2, 1, 2]


def test_jpeg_raw_pool_grows(api, monkeypatch):
    assert T.check_raw_pool(api, monkeypatch, None, 2400) >= 1
    assert T.check_raw_pool(api, monkeypatch, None, 2400, subsampling=0, beside=False) == 3
    assert T.check_raw_pool(api, monkeypatch, "plain", 650) >= 1
    assert T.check_raw_pool(api, monkeypatch, "plain", 2400, subsampling=0, beside=False) >= 1


def test_jpeg_pools_that_cannot_grow_enough_end_cleanly(api, monkeypatch):
    T.check_raw_and_token_pools_together(api, monkeypatch)
    T.check_jpeg_exhaustion_halves_the_group(api, monkeypatch)


def test_size_walk_over_a_growing_pool(api, monkeypatch):
    T.check_size_walk(api, monkeypatch)


@pytest.mark.parametrize("quality,expect", [(85, 1), (100, 2)])
def test_waves_mix_pieces_that_overflow_with_pieces_that_fit(api, monkeypatch, quality, expect):
    """64 copies of busy_200x150 interleaved one to one with 64 copies of flat_64x48, JPEG -> WebP under shift 4: a flat picture is one or two pieces of k_bool_code,
    a busy one several, so the waves hold lanes that give up (and keep walking their loops with the overflow flag set) beside lanes that write to the end.  Every
    file is the oracle's.  The batch repeats itself as often as its largest file asks: at quality 85 the busy picture (22 140 bytes, between the first two
    reservations of 10 596 and 29 316) needs one growth, at quality 100 (33 654 bytes) two -- both asserted from the oracle's file"""
    T.set_env(monkeypatch, CSH_TEST_POOL_SHIFT=4)
    busy, flat = T.busy_jpeg(), T.flat_jpeg()
    wb, wf = oracle_jpeg_to_webp(busy, quality), oracle_jpeg_to_webp(flat, quality)
    T.check_growths("busy", wb, 130, expect)
    assert T.growths(wf, 12) == 0
    b = api.webp_batch([busy, flat] * 64, T.params(webp_quality=quality))
    try:
        t = b.run()
        outs = b.fetch()
    finally:
        b.close()
    assert outs == [wb, wf] * 64
    assert t.n_pool_retries == expect, t.n_pool_retries
