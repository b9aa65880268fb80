"""The AC refinement scans PACKED from the compacted coefficient lists, without tokens (k_aclist.hip k_list_refine<false> + k_list_refine_pack),
on the CPU emulation build.  Every check runs three ways: the files equal the oracle's byte for byte, they equal the same call under CSH_REF_PACK=0 (pass 2 of
k_list_refine writes tokens, k_pack packs them, as before; CSH_REF_PACK=1 names the new path whatever the default is), and csh_timing.n_ref_packed says which
path ran -- a run that silently took the old path fails here.  The emulation build also stops when a chunk does not start where chunk_off says or a run does
not end where its sizes say.  The same bodies run on the MI355X in tests/test_ref_pack_gpu.py.

n_ref_packed counts the refinement work items a run packed from the lists: the script's refinement scans (tests/test_refine_lists_emul.py refine_scans), plus
luma's 3 -> 2 for every image that goes through the search's conditional stage ST_1B; 0 under CSH_REF_PACK=0, under CSH_REF_LIST=0 and for sequential output."""
import ctypes

import numpy as np
import pytest

import test_refine_lists_emul as E
from _util import emul_api, oracle_lossless, oracle_lossy
from gen_synth import synth_jpeg

PROFILES = E.PROFILES
params = E.params


@pytest.fixture(scope="module")
def api():
    return emul_api()


def expected_packed(ncomps, outs, prof, progressive=True):
    extra = E.st1b_images(outs) if (progressive and prof != "plain") else 0
    return E.refine_scans(ncomps, prof, progressive) + extra, extra


def check_group(api, monkeypatch, srcs, ncomps, prof, want, p=None, progressive=True):
    """one batch on both paths: the counter of each, the old path's bytes, the oracle's bytes (want(src) -> bytes).  Returns the new path's timing and how many
    images went through ST_1B"""
    p = p or params(jpeg_progressive=progressive)
    monkeypatch.setenv("CSH_REF_PACK", "1")
    outs, t = E.run_batch(api, srcs, p)
    monkeypatch.setenv("CSH_REF_PACK", "0")
    ref, t0 = E.run_batch(api, srcs, p)
    monkeypatch.delenv("CSH_REF_PACK", raising=False)
    assert t0.n_ref_packed == 0, "CSH_REF_PACK=0 must leave every refinement scan to the tokens and k_pack"
    assert t.n_search_extra == t0.n_search_extra and t.n_list_refine == t0.n_list_refine
    for i, (src, o, r) in enumerate(zip(srcs, outs, ref)):
        assert isinstance(o, bytes), (i, o)
        assert o == r, ("packed from lists != packed from tokens", i, prof)
        assert o == want(src), ("!= oracle", i, prof)
    n, extra = expected_packed(ncomps, outs, prof, progressive)
    assert t.n_ref_packed == n, (t.n_ref_packed, n, extra, prof)
    assert t.n_ref_packed == t.n_list_refine
    return t, extra


def set_run(monkeypatch, R):
    if R is None: monkeypatch.delenv("CSH_LIST_RUN", raising=False)
    else: monkeypatch.setenv("CSH_LIST_RUN", str(R))


# ---- 1. chunk edges: grey pictures of 1, 255, 256, 257 and 272 blocks; 4:2:0 pictures with one and with five luma chunks
def check_chunk_edges(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    srcs, ncomps = E.edge_set()
    check_group(api, monkeypatch, srcs, ncomps, prof, oracle_lossy)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_chunk_edges(api, monkeypatch, prof):
    check_chunk_edges(api, monkeypatch, prof)


# ---- 2. run edges: a grey component of exactly 8, of 9 and of 17 chunks (64 x 32, 72 x 32 and 136 x 32 blocks), one wave per 1, 3 and 8 chunks: a run that is
# the whole scan, a last run of one chunk, full runs with a remainder; position, window and carries cross the chunk edges inside a run
RUN_EDGE_SIZES = [(512, 256), (576, 256), (1088, 256)]
_run_edge_srcs = []


def run_edge_set():
    if not _run_edge_srcs:
        _run_edge_srcs.extend(E.grey_jpeg(w, h, 40 + i, texture=25 + 15 * i) for i, (w, h) in enumerate(RUN_EDGE_SIZES))
    return list(_run_edge_srcs), [1] * len(RUN_EDGE_SIZES)


def check_run_edges(api, monkeypatch, prof, R):
    E.set_profile(monkeypatch, prof)
    set_run(monkeypatch, R)
    srcs, ncomps = run_edge_set()
    t, _ = check_group(api, monkeypatch, srcs, ncomps, prof, oracle_lossy)
    assert t.n_list_runs > 0


@pytest.mark.parametrize("R", (1, 3, 8))
@pytest.mark.parametrize("prof", PROFILES)
def test_emul_run_edges(api, monkeypatch, prof, R):
    check_run_edges(api, monkeypatch, prof, R)


# ---- 3. real width != padded width
def check_unaligned(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    srcs, ncomps = E.unaligned_set()
    check_group(api, monkeypatch, srcs, ncomps, prof, oracle_lossy)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_unaligned(api, monkeypatch, prof):
    check_unaligned(api, monkeypatch, prof)


# ---- 4. dense blocks: white noise at q 100 and q 98, 4:4:4 and 4:2:0 -- 63 entries per block, 63-bit correction words, the most bits a step puts into the window
def check_dense_blocks(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    for srcs, ss in E.dense_sets():
        for q in (100, 98):
            p = params(jpeg_quality=q, jpeg_chroma_subsampling=ss)
            check_group(api, monkeypatch, srcs, [3] * len(srcs), prof, lambda s: oracle_lossy(s, q, subsampling=ss), p=p)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_dense_blocks(api, monkeypatch, prof):
    check_dense_blocks(api, monkeypatch, prof)


# ---- 5. crafted coefficients through a lossless transcode: every pattern of test_refine_lists_emul.PATTERNS occurs at both levels
def check_crafted(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    src, zz = E.crafted_file()
    for level in (0, 1):
        seen = set()
        for b in np.abs(zz.astype(np.int32)) >> level: seen |= E.block_patterns(b)
        for name in E.PATTERNS + ("all_history", "zrl_at_history", "new_at_63"):
            assert name in seen, (name, level, seen)
    srcs = [src, synth_jpeg(2, 64, 48, texture=30)]
    check_group(api, monkeypatch, srcs, [1, 3], prof, oracle_lossless, p=params(jpeg_optimize=True))


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_crafted(api, monkeypatch, prof):
    check_crafted(api, monkeypatch, prof)


# ---- 6. the pending-bits limit: with > 937 pending correction bits the EOB runs are cut (tail[], from which the packer rebuilds the blocks' H counts)
def check_pending_bits(api, monkeypatch, prof):
    from test_pipeline_emul import crafted_corrbit_stream
    E.set_profile(monkeypatch, prof)
    srcs = [crafted_corrbit_stream(), crafted_corrbit_stream(384, 640)]
    check_group(api, monkeypatch, srcs, [3, 3], prof, oracle_lossless, p=params(jpeg_optimize=True))


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_pending_bits(api, monkeypatch, prof):
    check_pending_bits(api, monkeypatch, prof)


# ---- 7. flat pictures: most blocks hold only their END entry, the EOB runs are long (k_ac_runs_long), an END entry emits the run's symbol and bits
def check_flat(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    srcs = [E.flat_jpeg(64, 64, 128), E.flat_jpeg(256, 256, 90, noisy_block=(100, 40))]
    check_group(api, monkeypatch, srcs, [3, 3], prof, oracle_lossy)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_flat(api, monkeypatch, prof):
    check_flat(api, monkeypatch, prof)


# ---- 8. a conditional search stage that only the first image asks for: work_active in k_list_refine_pack
def check_gated_stage(api, monkeypatch, prof, quality=80):
    E.set_profile(monkeypatch, prof)
    srcs, ncomps = E.gated_set()
    t, extra = check_group(api, monkeypatch, srcs, ncomps, prof, lambda s: oracle_lossy(s, quality), p=params(jpeg_quality=quality))
    assert t.n_search_extra > 0
    assert extra == 1, extra


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_emul_gated_stage(api, monkeypatch, prof):
    check_gated_stage(api, monkeypatch, prof)


# ---- 9. pools that overflow: the lists' regions start at a sixteenth of their estimate, the run repeats, the bytes are equal
def check_pools_that_overflow(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    monkeypatch.setenv("CSH_TEST_POOL_SHIFT", "4")
    srcs, ncomps = E.edge_set()
    check_group(api, monkeypatch, srcs, ncomps, prof, oracle_lossy)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_pools_that_overflow(api, monkeypatch, prof):
    check_pools_that_overflow(api, monkeypatch, prof)


# ---- 10. re-runs and size targeting
def check_run_twice_and_rerun(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    srcs, ncomps = E.edge_set()
    srcs, ncomps = srcs[3:], ncomps[3:]
    quals = [33, 97, 5, 60]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("CSH_REF_PACK", mode)
        b = api.batch(srcs, params())
        b.retain_dct()
        t1 = b.run(); first = b.fetch()
        t2 = b.run(); second = b.fetch()
        b.set_quality(quals)
        t3 = b.rerun_encode(); third = b.fetch()
        b.close()
        assert first == second
        for t, outs in ((t1, first), (t2, second), (t3, third)):
            assert t.n_ref_packed == (expected_packed(ncomps, outs, prof)[0] if mode == "1" else 0), (mode, t.n_ref_packed)
        got[mode] = (first, third)
    monkeypatch.delenv("CSH_REF_PACK", raising=False)
    assert got["1"] == got["0"]
    for src, o in zip(srcs, got["1"][0]):
        assert o == oracle_lossy(src)
    for src, o, q in zip(srcs, got["1"][1], quals):
        assert o == oracle_lossy(src, q), q


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_run_twice_and_rerun(api, monkeypatch, prof):
    check_run_twice_and_rerun(api, monkeypatch, prof)


def check_max_size(api, monkeypatch, prof):
    from test_pipeline_emul import reference_size_walk
    E.set_profile(monkeypatch, prof)
    srcs = [synth_jpeg(i, 160 + 16 * i, 120, subsampling=(0, 2, 1)[i % 3], texture=10 + 9 * i) for i in range(3)] + [synth_jpeg(9, 101, 67, texture=40)]
    monkeypatch.setenv("CSH_REF_PACK", "1")
    outs = api.batch_compress_to_size(srcs, params(), 4000)
    monkeypatch.setenv("CSH_REF_PACK", "0")
    ref = api.batch_compress_to_size(srcs, params(), 4000)
    monkeypatch.delenv("CSH_REF_PACK", raising=False)
    assert outs == ref
    for src, out in zip(srcs, outs):
        assert out == reference_size_walk(src, 4000)[1]


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_max_size(api, monkeypatch, prof):
    check_max_size(api, monkeypatch, prof)


# ---- 11. sequential output: no refinement scan, nothing packed from a list
def check_sequential(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    srcs, ncomps = E.edge_set()
    t, _ = check_group(api, monkeypatch, srcs, ncomps, prof, lambda s: oracle_lossy(s, progressive=0), progressive=False)
    assert t.n_ref_packed == 0


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_sequential(api, monkeypatch, prof):
    check_sequential(api, monkeypatch, prof)


# ---- 12. CSH_REF_LIST=0 switches the new path off by itself, whatever CSH_REF_PACK says
def check_ref_list_off(api, monkeypatch, prof):
    E.set_profile(monkeypatch, prof)
    srcs, ncomps = E.unaligned_set()
    monkeypatch.setenv("CSH_REF_LIST", "0")
    monkeypatch.setenv("CSH_REF_PACK", "1")
    outs, t = E.run_batch(api, srcs, params())
    assert t.n_ref_packed == 0 and t.n_list_refine == 0
    for src, o in zip(srcs, outs):
        assert o == oracle_lossy(src)


@pytest.mark.parametrize("prof", (None, "plain"))
def test_emul_ref_list_off(api, monkeypatch, prof):
    check_ref_list_off(api, monkeypatch, prof)


# ---- 13. emulation only: every launch's workgroups and lanes in reverse -- no file changes
def test_emul_back_to_front(api, monkeypatch):
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    api.L.csh_emul_set_reverse(1)
    try:
        for prof in PROFILES:
            check_chunk_edges(api, monkeypatch, prof)
            check_run_edges(api, monkeypatch, prof, 3)
            check_unaligned(api, monkeypatch, prof)
            check_dense_blocks(api, monkeypatch, prof)
    finally:
        api.L.csh_emul_set_reverse(0)
