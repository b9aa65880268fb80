"""The quantised AC levels that live in the coefficient lists alone (PlaneWork::ac_lists), on the CPU emulation build.
Where the forward-DCT kernels build a component's level-0 list and every coding kernel takes its AC levels from the lists, the transform stores
octet 0 of a block only and k_trellis_ac stores nothing to the tile.  Every file equals the oracle's and equals the same call under
CSH_AC_TILES=1 (the tiles written whole, as before), csh_timing.n_ac_in_lists says which path ran, and under the poison bit of CSH_DEBUG (the
output tiles start the run as garbage) no file changes: a kernel that still read octets 1..7 of such a component would read the garbage.  The
same bodies run on the MI355X in tests/test_ac_tiles_gpu.py.

Which components: those whose list the transform builds (test_fused_lists_emul.fused_components), in progressive output, with none of the
fallback switches set."""
import numpy as np
import pytest

import test_fused_lists_emul as F
from _util import emul_api, oracle_lossy, package
from gen_synth import synth_jpeg

PROFILES = F.PROFILES
POISON = "32768"   # CSH_DEBUG: batch_run.cpp Run::pixels
FALLBACKS = ("CSH_NZ_FUSED", "CSH_NZ_ONCE", "CSH_TR_SORT", "CSH_REF_LIST")


@pytest.fixture(scope="module")
def api():
    return emul_api()


def run_batch(api, srcs, p):
    b = api.batch(srcs, p)
    t = b.run()
    outs = b.fetch()
    b.close()
    return outs, t.n_ac_in_lists


_oracle = {}


def oracle_cached(src, quality, progressive, out_ss):
    """the oracle's file, once per (source, profile, parameters): the byte cases and the poison cases ask for the same ones"""
    import os
    key = (src, os.environ.get("CSH_PROFILE"), quality, progressive, out_ss)
    if key not in _oracle:
        _oracle[key] = oracle_lossy(src, quality, progressive=1 if progressive else 0, subsampling=out_ss)
    return _oracle[key]


def check_group(api, monkeypatch, srcs, widths, out_ss, ncomps=None, quality=80, progressive=True, poison=False):
    """one batch: the oracle's bytes, the bytes with the tiles written whole, and the number of components each run kept out of the tiles"""
    p = F.params(jpeg_quality=quality, jpeg_chroma_subsampling=out_ss, jpeg_progressive=progressive)
    ncomps = ncomps or [3] * len(srcs)
    expect = sum(F.fused_components(w, out_ss, nc) for w, nc in zip(widths, ncomps)) if progressive else 0
    monkeypatch.delenv("CSH_AC_TILES", raising=False)
    if poison: monkeypatch.setenv("CSH_DEBUG", POISON)
    outs, n = run_batch(api, srcs, p)
    monkeypatch.delenv("CSH_DEBUG", raising=False)
    monkeypatch.setenv("CSH_AC_TILES", "1")
    ref, n1 = run_batch(api, srcs, p)
    monkeypatch.delenv("CSH_AC_TILES", raising=False)
    assert n1 == 0, "CSH_AC_TILES=1 must store every component's levels to its tiles"
    assert n == expect, (n, expect, widths, out_ss)
    for i, (src, o, r) in enumerate(zip(srcs, outs, ref)):
        assert isinstance(o, bytes), (i, o)
        assert o == r, ("lists only != tiles written", i, widths[i], out_ss)
        assert o == oracle_cached(src, quality, progressive, out_ss), ("!= oracle", i, widths[i], out_ss)
    return n


# (width, height, input subsampling, texture)
ALIGNED_420 = [(128, 96, 420, 45), (208, 136, 420, 20), (16, 16, 420, 10), (320, 240, 420, 60)]   # 442 luma blocks: a last partial chunk; one chroma block; five luma chunks
MIXED_420 = [(97, 61, 420, 80), (136, 96, 420, 30)]   # ceil(w / 8) odd: luma keeps its tile, the two chroma components do not


def check_bytes(api, monkeypatch, prof, poison=False):
    F.set_profile(monkeypatch, prof)
    srcs, widths = F.synth_set(ALIGNED_420)
    assert check_group(api, monkeypatch, srcs, widths, 420, poison=poison) == 3 * len(srcs)
    srcs, widths = F.synth_set(MIXED_420)
    assert check_group(api, monkeypatch, srcs, widths, 420, poison=poison) == 2 * len(srcs)
    srcs, widths = F.synth_set([(64, 48, 444, 30)])
    assert check_group(api, monkeypatch, srcs, widths, 444, poison=poison) == 3
    assert check_group(api, monkeypatch, [F.grey_jpeg(203, 155, 7)], [203], 420, ncomps=[1], poison=poison) == 1
    srcs, widths = F.synth_set([(160, 120, 420, 25), (97, 61, 420, 40)])   # 4:2:0 -> 4:2:2: chroma through k_resample_plane + k_plane_fdct
    assert check_group(api, monkeypatch, srcs, widths, 422, poison=poison) == 3 + 2
    srcs, widths = F.synth_set(ALIGNED_420[:1] + MIXED_420[:1])
    assert check_group(api, monkeypatch, srcs, widths, 420, progressive=False, poison=poison) == 0   # sequential output is coded from the tiles


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_bytes(api, monkeypatch, prof):
    check_bytes(api, monkeypatch, prof)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_bytes_over_poisoned_tiles(api, monkeypatch, prof):
    check_bytes(api, monkeypatch, prof, poison=True)


def check_fallback_switches(api, monkeypatch, prof):
    """each of the switches that brings a reader of the tiles back keeps the tiles whole by itself"""
    F.set_profile(monkeypatch, prof)
    srcs, widths = F.synth_set(ALIGNED_420[:1] + MIXED_420[:1])
    p = F.params()
    for name in FALLBACKS:
        monkeypatch.setenv(name, "0")
        outs, n = run_batch(api, srcs, p)
        monkeypatch.delenv(name, raising=False)
        assert n == 0, (name, n)
        for src, o in zip(srcs, outs):
            assert o == oracle_cached(src, 80, True, 420), name
    outs, n = run_batch(api, srcs, p)
    assert n == 3 + 2


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_fallback_switches(api, monkeypatch, prof):
    check_fallback_switches(api, monkeypatch, prof)


def tap_sources():
    """the three sources of test_pipeline_gpu.test_stage_taps_equal_oracle and one more aligned 4:2:0 file"""
    return [synth_jpeg(5, 128, 96, texture=45), synth_jpeg(6, 97, 61, texture=80), synth_jpeg(3, 64, 48, subsampling=0), synth_jpeg(11, 208, 136, texture=30)]


def check_tap(api, monkeypatch):
    """csh_batch_read_coefs(.., which = 1) writes the AC coefficients back from the lists: the final coefficients of every component, twice over, and the batch runs on as before"""
    from oracle import oracle as O
    F.set_profile(monkeypatch, None)
    for name in FALLBACKS + ("CSH_AC_TILES", "CSH_DEBUG"): monkeypatch.delenv(name, raising=False)
    blobs = tap_sources()
    refs = [oracle_lossy(src) for src in blobs]
    # the case can fail: in the aligned source the trellis changes some coefficient 1..7 -- octet 0, which the transform stores with the scalar levels --, so a
    # tap that left octet 0 as the run leaves it would return the scalar level there
    monkeypatch.setenv("CSH_PROFILE", "scalar")
    scalar = O.decode(oracle_lossy(blobs[0]))
    F.set_profile(monkeypatch, None)
    final = O.decode(refs[0])
    assert any(not np.array_equal(final.coefs_zigzag(c)[..., 1:8], scalar.coefs_zigzag(c)[..., 1:8]) for c in range(3))
    b = api.batch(blobs, F.params())
    t = b.run()
    assert t.n_ac_in_lists == 3 + 2 + 3 + 3
    outs = b.fetch()
    for again in range(2):
        for i, ref in enumerate(refs):
            oo = O.decode(ref)
            for c in range(3):
                assert np.array_equal(b.coefs(i, c, 1)[0], oo.coefs_zigzag(c)), ("requant", again, i, c)
    t2 = b.run()
    assert t2.n_ac_in_lists == t.n_ac_in_lists
    assert b.fetch() == outs and outs == refs
    b.close()
    # the `scalar` profile has no trellis and no in-place compaction of the level-0 list (k_nzfilter under CSH_NZ_COMPACT0): the tap rebuilds from the list as the
    # transform left it, chunk padding and all
    monkeypatch.setenv("CSH_PROFILE", "scalar")
    srefs = [oracle_lossy(src) for src in blobs]
    b = api.batch(blobs, F.params())
    assert b.run().n_ac_in_lists == t.n_ac_in_lists
    for again in range(2):
        for i, ref in enumerate(srefs):
            oo = O.decode(ref)
            for c in range(3):
                assert np.array_equal(b.coefs(i, c, 1)[0], oo.coefs_zigzag(c)), ("scalar", again, i, c)
    assert b.fetch() == srefs
    b.close()
    F.set_profile(monkeypatch, None)


def test_emul_tap(api, monkeypatch):
    check_tap(api, monkeypatch)


def check_reruns(api, monkeypatch, prof):
    """a re-run at other qualities: through the transform again in the default profile (flagged again), a re-quantisation of the retained DCT in `scalar` (whole tiles, k_nzlist)"""
    F.set_profile(monkeypatch, prof)
    srcs, widths = F.synth_set(ALIGNED_420[:2] + MIXED_420[:1])
    expect = sum(F.fused_components(w, 420) for w in widths)
    b = api.batch(srcs, F.params())
    b.retain_dct()
    t1 = b.run()
    assert t1.n_ac_in_lists == expect
    for src, o in zip(srcs, b.fetch()):
        assert o == oracle_cached(src, 80, True, 420)
    quals = [33, 0, 97]
    b.set_quality(quals)
    t2 = b.rerun_encode()
    assert t2.n_ac_in_lists == (expect if prof is None else 0)
    for src, o, q in zip(srcs, b.fetch(), quals):
        assert o == oracle_lossy(src, q or 80), q
    t3 = b.run()   # ... and a whole run behind the re-quantisation
    assert t3.n_ac_in_lists == expect
    for src, o, q in zip(srcs, b.fetch(), quals):
        assert o == oracle_lossy(src, q or 80), q
    b.close()


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_emul_reruns(api, monkeypatch, prof):
    check_reruns(api, monkeypatch, prof)


def check_to_size(api, monkeypatch):
    from test_pipeline_emul import reference_size_walk
    F.set_profile(monkeypatch, None)
    src = synth_jpeg(12, 160, 120, texture=30)
    assert api.compress_to_size_in_memory(src, F.params(), 3000) == reference_size_walk(src, 3000)[1]


def test_emul_to_size(api, monkeypatch):
    check_to_size(api, monkeypatch)


def check_dense_and_overflowing(api, monkeypatch, prof):
    """white noise at q 100: a wave's entries do not fit its stretch of LDS (the list builder's second walk) and a block's list does not fit the trellis's LDS (its spill);
    then lists whose regions are too small at first: the run is repeated"""
    F.set_profile(monkeypatch, prof)
    assert check_group(api, monkeypatch, [F.noise_jpeg(64, 64, 1, 0)], [64], 444, quality=100) == 3
    monkeypatch.setenv("CSH_TEST_POOL_SHIFT", "4")
    srcs = [synth_jpeg(41, 320, 240, texture=40), synth_jpeg(42, 200, 136, subsampling=0, texture=70), synth_jpeg(43, 97, 61, texture=10)]
    check_group(api, monkeypatch, srcs, [320, 200, 97], 420)
    monkeypatch.delenv("CSH_TEST_POOL_SHIFT", raising=False)


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_emul_dense_and_overflowing(api, monkeypatch, prof):
    check_dense_and_overflowing(api, monkeypatch, prof)
