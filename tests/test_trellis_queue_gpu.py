"""k_trellis_ac's run queue on the MI355X (a grid of what is resident at once, runs of chunks handed out densest first, the next chunk's
block fetched during the current one): byte for byte against the oracle whatever the batch's shape, and on every run of a batch object
(the queue is zeroed in front of every launch)."""
import pytest

import test_trellis_emul as E
from _util import oracle_lossy, product_api
from gen_synth import synth_jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


def oracle_all(srcs, qs):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(16) as ex:   # (the oracle releases the GIL)
        return list(ex.map(lambda a: oracle_lossy(a[0], a[1]), zip(srcs, qs)))


def test_mixed_batch_many_more_runs_than_workgroups(api, monkeypatch):
    """q 100 files (lists past the 16 entries that live in LDS: the spill slots), 1080p q 80 files and hundreds of tiny images in one batch:
    many more runs than resident workgroups, so that every workgroup takes runs from the queue again and again"""
    monkeypatch.setenv("CSH_PROFILE", "mozjpeg")
    srcs = [synth_jpeg(300 + i, 1920, 1080, texture=5 * i) for i in range(3)]
    srcs += [synth_jpeg(310 + i, 320 + 48 * i, 240, subsampling=i % 3, texture=40 + 10 * i) for i in range(6)]
    srcs += [synth_jpeg(400 + i, 8 + 7 * (i % 9), 8 + 5 * (i % 7), subsampling=i % 3, texture=i % 50) for i in range(600)]
    qs = [80] * 3 + [100] * 6 + [(100, 80, 30)[i % 3] for i in range(600)]
    b = api.batch(srcs, E.params())
    try:
        b.retain_dct()
        b.run()
        b.set_quality(qs)
        b.rerun_encode()
        outs = b.fetch()
    finally:
        b.close()
    for i, (o, w) in enumerate(zip(outs, oracle_all(srcs, qs))):
        assert o == w, (i, qs[i])


def test_fewer_runs_than_the_grid(api, monkeypatch):
    """one small file: a run or two per component, a grid of that many workgroups"""
    monkeypatch.setenv("CSH_PROFILE", "mozjpeg")
    for q in (80, 100):
        src = synth_jpeg(77, 96, 64, texture=30)
        assert api.compress_in_memory(src, E.params(jpeg_quality=q)) == oracle_lossy(src, q), q


def test_the_same_batch_run_again_and_size_targeting(api, monkeypatch):
    """a batch object run three times (the queue starts at its head every time) and a --max-size walk (one trellis pass per try)"""
    monkeypatch.setenv("CSH_PROFILE", "mozjpeg")
    srcs = [synth_jpeg(500 + i, 640 + 96 * i, 480, subsampling=(2, 0, 1)[i % 3], texture=10 + 15 * i) for i in range(5)]
    want = oracle_all(srcs, [80] * len(srcs))
    b = api.batch(srcs, E.params())
    try:
        for k in range(3):
            b.run()
            assert b.fetch() == want, k
    finally:
        b.close()
    E.check_size_targeting(api, monkeypatch)
