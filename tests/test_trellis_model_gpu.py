"""The trellis quantiser on the MI355X against its stated cost model (tests/_trellis_model.py, tests/test_trellis_model.py): files made by the
device through product_api() equal the oracle's byte for byte, and their levels are admissible and of minimum model cost in float64.  Only
here do k_trellis_ac's wave-wide loop bounds, ballots and LDS / HBM spill boundary run with 64 different blocks in a wave (the emulation
build runs each lane alone): the battery's noise and full-texture files put blocks of few and of many list entries side by side."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import test_trellis_model as T
from _util import oracle_lossy, product_api
from gen_synth import synth_jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: the product has no CPU path"
    return a


def _default_case(src, q):
    return T.Case("file", src, q, 420)


def _check_files(srcs, qs, outs, what):
    """byte parity with the oracle and the model check for every file of a batch, in the default profile"""
    def one(i):
        case = _default_case(srcs[i], qs[i])
        assert outs[i] == oracle_lossy(srcs[i], qs[i]), (what, i, qs[i])
        return T.verify(T.export(case, "default"), outs[i], (what, i, qs[i]))
    with ThreadPoolExecutor(16) as ex:   # (the oracle releases the GIL)
        return max(ex.map(one, range(len(srcs))))


def test_device_battery_optimal_admissible_and_the_oracles(api, monkeypatch):
    worst = 0.0
    for prof, (_, env, _) in T.PROFILES.items():
        monkeypatch.setenv("CSH_PROFILE", env)
        for case in T.cached_battery():
            out = api.compress_in_memory(case.src, T.device_params(case, prof))
            assert out == T.oracle_file(case, prof), (case.name, prof)
            worst = max(worst, T.verify(T.export(case, prof), out, (case.name, prof)))
    print(f"device battery: worst gap {worst:.3g} of the tolerance")


def test_device_mixed_batch_retained_and_requantised(api, monkeypatch):
    """three 1080p files at q 80 and the mixed batch of test_trellis_queue_gpu.py (600 tiny files at q 100, 80, 30: many more runs than
    resident workgroups), run at q 80, then re-quantised from the retained DCT at each file's own quality"""
    monkeypatch.setenv("CSH_PROFILE", "mozjpeg")
    srcs = [synth_jpeg(300 + i, 1920, 1080, texture=5 * i) for i in range(3)]
    srcs += [synth_jpeg(310 + i, 320 + 48 * i, 240, subsampling=i % 3, texture=40 + 10 * i) for i in range(6)]
    srcs += [synth_jpeg(400 + i, 8 + 7 * (i % 9), 8 + 5 * (i % 7), subsampling=i % 3, texture=i % 50) for i in range(600)]
    qs = [80] * 3 + [100] * 6 + [(100, 80, 30)[i % 3] for i in range(600)]
    b = api.batch(srcs, T.device_params(_default_case(srcs[0], 80), "default"))
    try:
        b.retain_dct()
        b.run()
        first = b.fetch()
        b.set_quality(qs)
        b.rerun_encode()
        outs = b.fetch()
    finally:
        b.close()
    w1 = _check_files(srcs[:3], [80] * 3, first[:3], "1080p q80")
    w2 = _check_files(srcs, qs, outs, "rerun")
    print(f"mixed batch: worst gap {max(w1, w2):.3g} of the tolerance")


def test_device_size_walk_and_sequential(api, monkeypatch):
    """a --max-size walk, checked at the quality where libcaesium's walk ends; and sequential output"""
    from test_pipeline_emul import reference_size_walk
    monkeypatch.setenv("CSH_PROFILE", "mozjpeg")
    srcs = [synth_jpeg(i, 160 + 16 * i, 120, subsampling=(0, 2, 1)[i % 3], texture=10 + 9 * i) for i in range(4)]
    for i, (src, out) in enumerate(zip(srcs, api.batch_compress_to_size(srcs, T.device_params(_default_case(srcs[0], 80), "default"), 4000))):
        seq, want = reference_size_walk(src, 4000)
        assert out == want, i
        T.verify(T.export(T.Case("walk", src, seq[-1], 420), "default"), out, ("walk", i, seq[-1]))
    for i, src in enumerate(srcs):
        case = T.Case("seq", src, 80, 420)
        out = api.compress_in_memory(src, T.device_params(case, "baseline"))
        assert out == T.oracle_file(case, "baseline"), i
        T.verify(T.export(case, "baseline"), out, ("seq", i))
