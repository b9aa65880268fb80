"""The level-0 coefficient lists built inside the forward-DCT kernels (k_pixel.hip nzf_*), on the CPU emulation build: every
file equals the oracle's and equals the same call under CSH_NZ_FUSED=0 (k_nzlist builds every list from the tiles, as before), and
csh_timing.n_fused_lists says which path ran -- a run that silently took the fallback everywhere fails here.  The same bodies run on the
MI355X in tests/test_fused_lists_gpu.py.

A component's list is built by the transform when its real block grid is as wide as its MCU-padded one (a workgroup's 256 blocks are then
a list chunk): every component with horizontal sampling factor 1 (chroma of 4:2:0 / 4:2:2, everything of 4:4:4, grey), and luma when
ceil(width / 8) is a multiple of its sampling factor -- a width that is a multiple of the MCU width in particular."""
import ctypes
import io

import numpy as np
import pytest

from _util import emul_api, oracle_lossy, package
from gen_synth import synth_jpeg, synth_rgb

PROFILES = (None, "scalar", "plain")
SS_IN = {444: 0, 422: 1, 420: 2}


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


def set_profile(monkeypatch, prof):
    if prof: monkeypatch.setenv("CSH_PROFILE", prof)
    else: monkeypatch.delenv("CSH_PROFILE", raising=False)


def fused_components(width, out_ss, ncomp=3):
    """how many components of a progressive lossy output the transform builds the list of: real_bw == bw per component"""
    if ncomp == 1:
        return 1
    h = {444: 1, 422: 2, 420: 2, 411: 4}[out_ss]   # luma's horizontal factor; chroma has 1 and is always as wide as its padded grid
    luma_real, luma_padded = -(-width // 8), -(-width // (8 * h)) * h
    return 2 + (1 if luma_real == luma_padded else 0)


def noise_jpeg(w, h, seed, subsampling):
    """white noise at q 100: every coefficient of every block is a list entry -- a wave's 64 blocks hold twice what its stretch of LDS does"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    b = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(b, format="JPEG", quality=100, subsampling=subsampling)
    return b.getvalue()


def grey_jpeg(w, h, seed, texture=20):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(synth_rgb(seed, w, h, texture)).convert("L").save(b, format="JPEG", quality=90)
    return b.getvalue()


def run_batch(api, srcs, p):
    b = api.batch(srcs, p)
    t = b.run()
    outs = b.fetch()
    b.close()
    return outs, t.n_fused_lists


def check_group(api, monkeypatch, srcs, widths, out_ss, ncomps=None, quality=80, progressive=True, expect=None):
    """one batch: the oracle's bytes, the bytes of the unfused path, and the path each took"""
    p = params(jpeg_quality=quality, jpeg_chroma_subsampling=out_ss, jpeg_progressive=progressive)
    ncomps = ncomps or [3] * len(srcs)
    if expect is None:
        expect = sum(fused_components(w, out_ss, nc) for w, nc in zip(widths, ncomps)) if progressive else 0
    monkeypatch.delenv("CSH_NZ_FUSED", raising=False)
    outs, n = run_batch(api, srcs, p)
    monkeypatch.setenv("CSH_NZ_FUSED", "0")
    ref, n0 = run_batch(api, srcs, p)
    monkeypatch.delenv("CSH_NZ_FUSED", raising=False)
    assert n0 == 0, "CSH_NZ_FUSED=0 must leave every list to k_nzlist"
    assert n == expect, (n, expect, widths, out_ss)
    for i, (src, o, r) in enumerate(zip(srcs, outs, ref)):
        assert isinstance(o, bytes), (i, o)
        assert o == r, ("fused != unfused", i, widths[i], out_ss)
        assert o == oracle_lossy(src, quality, progressive=1 if progressive else 0, subsampling=out_ss), ("!= oracle", i, widths[i], out_ss)
    return n


# (width, height, input subsampling, texture)
ALIGNED_420 = [(128, 96, 420, 45), (208, 136, 420, 20), (64, 48, 420, 30), (16, 16, 420, 10), (320, 240, 420, 60)]   # 442 luma blocks: a last partial chunk; 48 / 12 blocks; one chroma block; five luma chunks
UNALIGNED_420 = [(101, 67, 420, 0), (97, 61, 420, 80), (33, 31, 420, 60), (8, 8, 420, 20), (1, 1, 420, 0), (104, 72, 420, 30)]   # ceil(w / 8) odd: luma falls back, chroma does not


def synth_set(cases):
    return [synth_jpeg(7 + k, w, h, subsampling=SS_IN[ss], texture=tex) for k, (w, h, ss, tex) in enumerate(cases)], [c[0] for c in cases]


def check_layouts(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    # 4:2:0 kept: k_xform_direct (luma) and k_resample_fdct_420 (chroma); all three lists of every file come from the transform
    srcs, widths = synth_set(ALIGNED_420)
    assert check_group(api, monkeypatch, srcs, widths, 420) == 3 * len(srcs)
    # widths that are not a multiple of the MCU width: luma's list is k_nzlist's, the two chroma lists the transform's
    srcs, widths = synth_set(UNALIGNED_420)
    assert check_group(api, monkeypatch, srcs, widths, 420) == 2 * len(srcs)
    # both kinds in one batch
    srcs, widths = synth_set(ALIGNED_420[:2] + UNALIGNED_420[:3] + ALIGNED_420[2:4])
    assert check_group(api, monkeypatch, srcs, widths, 420) == 3 * 4 + 2 * 3
    # 4:2:0 -> 4:2:2 and -> 4:4:4: chroma through k_resample_plane + k_plane_fdct
    srcs, widths = synth_set([(160, 120, 420, 25), (97, 61, 420, 40), (48, 40, 420, 5)])
    assert check_group(api, monkeypatch, srcs, widths, 422) == 3 + 2 + 3
    assert check_group(api, monkeypatch, srcs, widths, 444) == 9
    # 4:4:4 input, kept (every component through k_xform_direct) and subsampled (chroma through k_plane_fdct)
    srcs, widths = synth_set([(104, 72, 444, 30), (64, 48, 444, 10), (17, 9, 444, 50), (8, 8, 444, 0)])
    assert check_group(api, monkeypatch, srcs, widths, 444) == 12
    assert check_group(api, monkeypatch, srcs, widths, 420) == 2 + 3 + 2 + 2
    # grey: one component, one block
    greys = [grey_jpeg(203, 155, 7), grey_jpeg(8, 8, 8), grey_jpeg(64, 64, 9)]
    assert check_group(api, monkeypatch, greys, [203, 8, 64], 420, ncomps=[1, 1, 1]) == 3


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_layouts(api, monkeypatch, prof):
    check_layouts(api, monkeypatch, prof)


def check_dense_blocks(api, monkeypatch, prof):
    """noise at q 98 .. 100: a wave's entries do not fit its stretch of LDS and go straight to memory; mixed with waves that fit"""
    set_profile(monkeypatch, prof)
    srcs = [noise_jpeg(128, 128, 1, 0), noise_jpeg(144, 80, 2, 0), synth_jpeg(3, 128, 96, subsampling=0, texture=30)]
    for q in (100, 98):
        assert check_group(api, monkeypatch, srcs, [128, 144, 128], 444, quality=q) == 9
    srcs = [noise_jpeg(160, 96, 4, 2), synth_jpeg(5, 97, 61, texture=70)]
    assert check_group(api, monkeypatch, srcs, [160, 97], 420, quality=99) == 5


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_dense_blocks(api, monkeypatch, prof):
    check_dense_blocks(api, monkeypatch, prof)


def check_clipped_highlights(api, monkeypatch, prof):
    """the picture the trellis tests use for deringing: the default profile's transform rewrites its blocks in LDS before the list's entries go there"""
    from test_trellis_emul import saturated_jpeg
    set_profile(monkeypatch, prof)
    for ss in (420, 444, 422):
        srcs = [saturated_jpeg(subsampling=SS_IN[ss]), saturated_jpeg(203, 155, seed=8, subsampling=SS_IN[ss])]
        check_group(api, monkeypatch, srcs, [160, 203], ss)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_clipped_highlights(api, monkeypatch, prof):
    check_clipped_highlights(api, monkeypatch, prof)


def check_baseline_needs_no_list(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    srcs, widths = synth_set(ALIGNED_420[:3] + UNALIGNED_420[:2])
    assert check_group(api, monkeypatch, srcs, widths, 420, progressive=False) == 0


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_baseline_needs_no_list(api, monkeypatch, prof):
    check_baseline_needs_no_list(api, monkeypatch, prof)


def check_run_twice_and_rerun(api, monkeypatch, prof):
    """one batch run twice: the cursors and counts the transform adds to are zeroed in front of it every time.  A re-run at other qualities goes through
    the transform again where the profile derings (fused) and re-quantises the retained DCT where it does not (k_nzlist)"""
    set_profile(monkeypatch, prof)
    monkeypatch.delenv("CSH_NZ_FUSED", raising=False)
    srcs, widths = synth_set(ALIGNED_420[:3] + UNALIGNED_420[:2])
    expect = sum(fused_components(w, 420) for w in widths)
    b = api.batch(srcs, params())
    b.retain_dct()
    t1 = b.run(); first = b.fetch()
    t2 = b.run(); second = b.fetch()
    assert t1.n_fused_lists == expect and t2.n_fused_lists == expect
    assert first == second
    for src, o in zip(srcs, first):
        assert o == oracle_lossy(src)
    quals = [33, 0, 97, 5, 60]
    b.set_quality(quals)
    t3 = b.rerun_encode()
    assert t3.n_fused_lists == (expect if prof is None else 0)
    for src, o, q in zip(srcs, b.fetch(), quals):
        assert o == oracle_lossy(src, q or 80), q
    b.close()


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_run_twice_and_rerun(api, monkeypatch, prof):
    check_run_twice_and_rerun(api, monkeypatch, prof)


def check_max_size(api, monkeypatch, prof):
    """--max-size: every try is a re-run; each file ends where libcaesium's walk over full runs ends, fused or not"""
    from test_pipeline_emul import reference_size_walk
    set_profile(monkeypatch, prof)
    srcs = [synth_jpeg(i, 160 + 16 * i, 120, subsampling=(0, 2, 1)[i % 3], texture=10 + 9 * i) for i in range(3)] + [synth_jpeg(9, 101, 67, texture=40)]
    monkeypatch.delenv("CSH_NZ_FUSED", raising=False)
    outs = api.batch_compress_to_size(srcs, params(), 4000)
    monkeypatch.setenv("CSH_NZ_FUSED", "0")
    ref = api.batch_compress_to_size(srcs, params(), 4000)
    monkeypatch.delenv("CSH_NZ_FUSED", raising=False)
    assert outs == ref
    for src, out in zip(srcs, outs):
        assert out == reference_size_walk(src, 4000)[1]


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_max_size(api, monkeypatch, prof):
    check_max_size(api, monkeypatch, prof)


def check_pools_that_overflow(api, monkeypatch, prof):
    """CSH_TEST_POOL_SHIFT: the lists' regions start a sixteenth of their estimate -- the transform's reservation fails, says so (overflow[1]) and the run is repeated"""
    set_profile(monkeypatch, prof)
    monkeypatch.setenv("CSH_TEST_POOL_SHIFT", "4")
    srcs = [synth_jpeg(41, 320, 240, texture=40), synth_jpeg(42, 200, 136, subsampling=0, texture=70), synth_jpeg(43, 97, 61, texture=10)]
    check_group(api, monkeypatch, srcs, [320, 200, 97], 420)


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_emul_pools_that_overflow(api, monkeypatch, prof):
    check_pools_that_overflow(api, monkeypatch, prof)


def test_emul_back_to_front(api, monkeypatch):
    """the emulation runs every launch's workgroups and lanes in reverse: where a chunk lands in its list's region changes, no file does"""
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    api.L.csh_emul_set_reverse(1)
    try:
        for prof in PROFILES:
            set_profile(monkeypatch, prof)
            srcs, widths = synth_set(ALIGNED_420[:4] + UNALIGNED_420[:2])
            check_group(api, monkeypatch, srcs, widths, 420)
            check_group(api, monkeypatch, [noise_jpeg(128, 128, 1, 0)], [128], 444, quality=100)
    finally:
        api.L.csh_emul_set_reverse(0)
