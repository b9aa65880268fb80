"""The AC refinement scans coded from the compacted coefficient lists (k_aclist.hip k_list_refine), on the CPU emulation build.
Every check runs three ways: the files equal the oracle's byte for byte, they equal the same call under CSH_REF_LIST=0 (k_tokens' kind-0
chunks code the refinement scans from the tiles, as before; CSH_REF_LIST=1 names the list path whatever the default is), and csh_timing.n_list_refine says which path ran -- a run that silently took
the old path fails here.  The same bodies run on the MI355X in tests/test_refine_lists_gpu.py.

n_list_refine counts the refinement work items a run coded from lists.  The stock script (CSH_PROFILE=plain) has four per colour file (luma
2 -> 1 and 1 -> 0, Cb and Cr 1 -> 0) and two per grey file; the first stage of the scan search has six (luma 1 -> 0 and 2 -> 1, both chroma
components likewise) and two; the search's conditional stage ST_1B adds luma's 3 -> 2 for every image that asks for it."""
import ctypes
import io

import numpy as np
import pytest

from _util import emul_api, oracle_lossless, oracle_lossy, package
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


def refine_scans(ncomps, prof, progressive=True):
    """refinement work items every run codes: the stock script's, or those of the search's first stage"""
    if not progressive:
        return 0
    colour, grey = (4, 2) if prof == "plain" else (6, 2)
    return sum(colour if nc == 3 else grey for nc in ncomps)


def grey_jpeg(w, h, seed, texture=20, quality=90):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(synth_rgb(seed, w, h, texture)).convert("L").save(b, format="JPEG", quality=quality)
    return b.getvalue()


def noise_jpeg(w, h, seed, subsampling):
    """white noise at q 100: 63 list entries per block"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    b = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(b, format="JPEG", quality=100, subsampling=subsampling)
    return b.getvalue()


def flat_jpeg(w, h, value, noisy_block=None, seed=5):
    from PIL import Image
    a = np.full((h, w, 3), value, np.uint8)
    if noisy_block:
        y, x = noisy_block
        a[y:y + 8, x:x + 8] = np.random.default_rng(seed).integers(0, 255, (8, 8, 3))
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="JPEG", quality=92, subsampling=2)
    return b.getvalue()


def run_batch(api, srcs, p):
    b = api.batch(srcs, p)
    t = b.run()
    outs = b.fetch()
    b.close()
    return outs, t


def st1b_images(outs):
    """how many of the files went through the search's conditional stage ST_1B, read off the files themselves: the search tries luma at Al 3 exactly when Al 2
    beat Al 1 (jcmaster.c select_scans; scan_search.cpp), and then luma's band scans are coded at Al 2 or 3"""
    from oracle import oracle as O
    n = 0
    for o in outs:
        luma_first = [s for s in O.decode(o).scans() if tuple(s[0]) == (0,) and s[1] > 0 and s[3] == 0]
        n += 1 if luma_first and luma_first[0][4] >= 2 else 0
    return n


def check_counter(t, ncomps, outs, prof, progressive=True):
    """n_list_refine EQUALS the refinement scans of the script: what every run codes, plus luma's 3 -> 2 for every image of ST_1B (the scan search only)"""
    extra = st1b_images(outs) if (progressive and prof != "plain") else 0
    assert t.n_list_refine == refine_scans(ncomps, prof, progressive) + extra, (t.n_list_refine, refine_scans(ncomps, prof, progressive), extra, t.n_search_extra, prof)
    assert extra == 0 or t.n_search_extra > 0
    return extra


def check_group(api, monkeypatch, srcs, ncomps, prof, want, p=None, progressive=True):
    """one batch: the path each run took, the bytes of the old path, the oracle's bytes (want(src) -> bytes).  Returns the new path's timing and how many
    images went through ST_1B"""
    p = p or params(jpeg_progressive=progressive)
    monkeypatch.setenv("CSH_REF_LIST", "1")
    outs, t = run_batch(api, srcs, p)
    monkeypatch.setenv("CSH_REF_LIST", "0")
    ref, t0 = run_batch(api, srcs, p)
    monkeypatch.delenv("CSH_REF_LIST", raising=False)
    assert t0.n_list_refine == 0, "CSH_REF_LIST=0 must leave every refinement scan to k_tokens"
    assert t.n_search_extra == t0.n_search_extra
    for i, (src, o, r) in enumerate(zip(srcs, outs, ref)):
        assert isinstance(o, bytes), (i, o)
        assert o == r, ("lists != tiles", i, prof)
        assert o == want(src), ("!= oracle", i, prof)
    return t, check_counter(t, ncomps, outs, prof, progressive)


# ---- 1. chunk edges: grey pictures of 1, 255, 256, 257 and 272 blocks; 4:2:0 pictures with one and with five luma chunks
GREY_EDGES = [(8, 8), (120, 136), (128, 128), (8 * 257, 8), (136, 128)]
COLOUR_EDGES = [(128, 96, 45), (320, 240, 60)]


def edge_set():
    srcs = [grey_jpeg(w, h, 20 + i, texture=15 + 10 * i) for i, (w, h) in enumerate(GREY_EDGES)]
    srcs += [synth_jpeg(30 + i, w, h, subsampling=2, texture=tex) for i, (w, h, tex) in enumerate(COLOUR_EDGES)]
    return srcs, [1] * len(GREY_EDGES) + [3] * len(COLOUR_EDGES)


def check_chunk_edges(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    srcs, ncomps = edge_set()
    check_group(api, monkeypatch, srcs, ncomps, prof, oracle_lossy)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_chunk_edges(api, monkeypatch, prof):
    check_chunk_edges(api, monkeypatch, prof)


# ---- 2. real width != padded width: the lists come from k_nzlist, units run in raster order over the real width
def unaligned_set():
    cases = [(101, 67, 0), (97, 61, 80), (33, 31, 60), (1, 1, 0)]
    return [synth_jpeg(7 + k, w, h, subsampling=2, texture=tex) for k, (w, h, tex) in enumerate(cases)], [3] * len(cases)


def check_unaligned(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    srcs, ncomps = unaligned_set()
    check_group(api, monkeypatch, srcs, ncomps, prof, oracle_lossy)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_unaligned(api, monkeypatch, prof):
    check_unaligned(api, monkeypatch, prof)


# ---- 3. dense blocks: 63 entries per block straddle a lane's four entries and the step of 256; 63-bit correction words; mixed with sparse pictures
def dense_sets():
    return [([noise_jpeg(128, 128, 1, 0), noise_jpeg(144, 80, 2, 0), synth_jpeg(3, 128, 96, subsampling=0, texture=30)], 444),
            ([noise_jpeg(160, 96, 4, 2), synth_jpeg(5, 97, 61, texture=70), noise_jpeg(64, 48, 6, 2)], 420)]


def check_dense_blocks(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    for srcs, ss in dense_sets():
        for q in (100, 98):
            p = params(jpeg_quality=q, jpeg_chroma_subsampling=ss)
            check_group(api, monkeypatch, srcs, [3] * len(srcs), prof, lambda s: oracle_lossy(s, q, subsampling=ss), p=p)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_dense_blocks(api, monkeypatch, prof):
    check_dense_blocks(api, monkeypatch, prof)


# ---- 4. crafted coefficients, through a lossless transcode
PATTERNS = ("gap16", "gap32", "zrl_between_history", "zrl_at_history", "history_tail", "history_only", "new_at_63", "all_history", "empty")


def block_patterns(m):
    """which of PATTERNS a block shows in a refinement scan over 1..63; m[k]: the magnitude of coefficient k (zig-zag) at the scan's level.
    A walk in the order of jcphuff.c encode_mcu_AC_refine, written for the test: r counts the zeros of the gap, history coefficients do not"""
    found = set()
    new = [k for k in range(1, 64) if m[k] == 1]
    hist = [k for k in range(1, 64) if m[k] >= 2]
    if not new and not hist:
        return {"empty"}
    if not new:
        found.add("history_only")
    if len(hist) == 63:
        found.add("all_history")
    if new and new[-1] == 63:
        found.add("new_at_63")
    if new and any(k > new[-1] for k in hist):
        found.add("history_tail")
    prev = 0
    for n in new:
        r = zeros = history = 0
        history_before_16th = False
        for k in range(prev + 1, n + 1):
            if m[k] == 0:
                r += 1; zeros += 1
                if zeros == 16: history_before_16th = history > 0
                continue
            zrls = r // 16       # emitted at this coefficient: sixteen more zeros of the gap have gone by
            r -= 16 * zrls
            if zrls >= 2: found.add("gap32")
            if k != n:
                if zrls: found.add("zrl_at_history")
                if zeros >= 16 and history_before_16th: found.add("zrl_between_history")
                history += 1
        if zeros >= 16: found.add("gap16")
        prev = n
    return found


def crafted_blocks(rng):
    """zig-zag magnitudes-with-sign of the hand-made blocks, then random mixtures"""
    def blk(**at):
        b = np.zeros(64, np.int16)
        for k, v in at.items(): b[int(k[1:])] = v
        return b
    H = [2, -3, 3, -2, 5, -7]
    out = [blk(k20=1), blk(k40=-1), blk(k5=H[0], k21=H[1], k25=1), blk(k17=H[2], k20=-1), blk(k3=1, k10=H[3], k11=H[4], k30=H[5]), blk(k1=H[1], k7=H[0], k50=H[2]),
           blk(k2=H[4], k63=1), blk(), blk(k1=1, k2=-1, k63=-1), blk(k6=H[0], k23=H[1], k40=H[2], k41=1), blk()]
    full = rng.choice(np.array([-3, -2, 2, 3, 6], np.int16), 64); full[0] = 0
    out += [full, blk(), blk()]
    for dens in (0.1, 0.3, 0.6):
        for _ in range(30):
            b = np.zeros(64, np.int16)
            on = rng.random(64) < dens
            b[on] = rng.choice(np.array([-1, 1, 1, -1, 2, -2, 3, -5], np.int16), int(on.sum()))
            b[0] = 0
            out.append(b)
    return out


def crafted_file(seed=3, w=128, h=128):
    """a grey picture (256 blocks) whose AC coefficients are the crafted blocks (first half) and the same blocks with every magnitude doubled (second half):
    the 1 -> 0 scan meets the patterns in the first half, the 2 -> 1 scan in the second.  Returns the file and the zig-zag coefficients"""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    base = O.forward(rng.integers(0, 255, (h, w), dtype=np.uint8), O.params(quality=90))
    y = base.coefs_view(0)
    blocks = crafted_blocks(rng)
    blocks = blocks + [2 * b for b in blocks]
    assert len(blocks) <= y.shape[0] * y.shape[1]
    zz = np.zeros((y.shape[0] * y.shape[1], 64), np.int16)
    zz[:len(blocks)] = np.array(blocks)
    flat = y.reshape(-1, 64)
    flat[:, np.array(O.ZZ)[1:]] = zz[:, 1:]
    return base.encode(O.params(progressive=1, marker_style=0)), zz


def check_crafted(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    src, zz = crafted_file()
    for level in (0, 1):
        seen = {}
        for b in np.abs(zz.astype(np.int32)) >> level:
            for name in block_patterns(b): seen[name] = seen.get(name, 0) + 1
        for name in PATTERNS:
            assert seen.get(name, 0) >= 1, (name, level, seen)
    srcs = [src, synth_jpeg(2, 64, 48, texture=30)]
    check_group(api, monkeypatch, srcs, [1, 3], prof, oracle_lossless, p=params(jpeg_optimize=True))


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_crafted(api, monkeypatch, prof):
    check_crafted(api, monkeypatch, prof)


# ---- 5. the pending-bits limit: with > 937 pending correction bits the EOB runs are cut (tail[])
def check_pending_bits(api, monkeypatch, prof):
    from test_pipeline_emul import crafted_corrbit_stream
    set_profile(monkeypatch, prof)
    srcs = [crafted_corrbit_stream(), crafted_corrbit_stream(384, 640)]
    check_group(api, monkeypatch, srcs, [3, 3], prof, oracle_lossless, p=params(jpeg_optimize=True))


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_pending_bits(api, monkeypatch, prof):
    check_pending_bits(api, monkeypatch, prof)


# ---- 6. flat pictures: most blocks hold only their END entry, the EOB runs are long
def check_flat(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    srcs = [flat_jpeg(64, 64, 128), flat_jpeg(256, 256, 90, noisy_block=(100, 40))]
    check_group(api, monkeypatch, srcs, [3, 3], prof, oracle_lossy)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_flat(api, monkeypatch, prof):
    check_flat(api, monkeypatch, prof)


# ---- 7. a conditional search stage: some images ask for ST_1B (luma at Al 3 and its 3 -> 2 refinement), others do not
def gated_set():
    """(seed, texture) of 160 x 120 pictures at q 80, found by trying them on the emulation build: the first one's search finds luma's Al 2 cheaper than Al 1 and
    asks for Al 3 (ST_1B) in the default and in the scalar profile; the others' searches stop earlier (the last one's runs on into the late splits only)"""
    cases = [(4, 90), (0, 10), (0, 0), (1, 90)]
    return [synth_jpeg(sd, 160, 120, texture=tx) for sd, tx in cases], [3] * len(cases)


def check_gated_stage(api, monkeypatch, prof, quality=80):
    set_profile(monkeypatch, prof)
    srcs, ncomps = gated_set()
    p = params(jpeg_quality=quality)
    t, extra = check_group(api, monkeypatch, srcs, ncomps, prof, lambda s: oracle_lossy(s, quality), p=p)
    assert t.n_search_extra > 0
    assert extra == 1, extra   # the first image went through ST_1B, the others did not: work_active in k_list_refine


@pytest.mark.parametrize("prof", (None, "scalar"))
def test_emul_gated_stage(api, monkeypatch, prof):
    check_gated_stage(api, monkeypatch, prof)


# ---- 8. pools that overflow: the reservation fails, the run repeats, the bytes are equal
def check_pools_that_overflow(api, monkeypatch, prof):
    """every pool starts at a sixteenth of its estimate -- the coefficient lists' regions as well as the token regions, and one scale grows for all of them on a
    retry: the files are right after the retries, but nothing here tells whether it was k_list_refine's own reservation that failed first"""
    set_profile(monkeypatch, prof)
    monkeypatch.setenv("CSH_TEST_POOL_SHIFT", "4")
    srcs, ncomps = edge_set()
    check_group(api, monkeypatch, srcs, ncomps, prof, oracle_lossy)


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_pools_that_overflow(api, monkeypatch, prof):
    check_pools_that_overflow(api, monkeypatch, prof)


# ---- 9. re-runs and size targeting
def check_run_twice_and_rerun(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    srcs, ncomps = edge_set()
    srcs, ncomps = srcs[3:], ncomps[3:]
    quals = [33, 97, 5, 60]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("CSH_REF_LIST", mode)
        b = api.batch(srcs, params())
        b.retain_dct()
        t1 = b.run(); first = b.fetch()
        t2 = b.run(); second = b.fetch()
        b.set_quality(quals)
        t3 = b.rerun_encode(); third = b.fetch()
        b.close()
        assert first == second
        if mode == "1":
            assert check_counter(t1, ncomps, first, prof) == check_counter(t2, ncomps, second, prof)
            check_counter(t3, ncomps, third, prof)
        else:
            assert t1.n_list_refine == 0 and t2.n_list_refine == 0 and t3.n_list_refine == 0
        got[mode] = (first, third)
    monkeypatch.delenv("CSH_REF_LIST", raising=False)
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
    set_profile(monkeypatch, prof)
    srcs = [synth_jpeg(i, 160 + 16 * i, 120, subsampling=(0, 2, 1)[i % 3], texture=10 + 9 * i) for i in range(3)] + [synth_jpeg(9, 101, 67, texture=40)]
    monkeypatch.setenv("CSH_REF_LIST", "1")
    outs = api.batch_compress_to_size(srcs, params(), 4000)
    monkeypatch.setenv("CSH_REF_LIST", "0")
    ref = api.batch_compress_to_size(srcs, params(), 4000)
    monkeypatch.delenv("CSH_REF_LIST", raising=False)
    assert outs == ref
    for src, out in zip(srcs, outs):
        assert out == reference_size_walk(src, 4000)[1]


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_max_size(api, monkeypatch, prof):
    check_max_size(api, monkeypatch, prof)


# ---- 10. sequential output: no refinement scan, no list
def check_sequential(api, monkeypatch, prof):
    set_profile(monkeypatch, prof)
    srcs, ncomps = edge_set()
    t, _ = check_group(api, monkeypatch, srcs, ncomps, prof, lambda s: oracle_lossy(s, progressive=0), progressive=False)
    assert t.n_list_refine == 0


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_sequential(api, monkeypatch, prof):
    check_sequential(api, monkeypatch, prof)


# ---- 11. emulation only: every launch's workgroups and lanes in reverse -- where a slot's tokens land in the pool changes, no file does
def test_emul_back_to_front(api, monkeypatch):
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    api.L.csh_emul_set_reverse(1)
    try:
        for prof in PROFILES:
            check_chunk_edges(api, monkeypatch, prof)
            check_unaligned(api, monkeypatch, prof)
            check_dense_blocks(api, monkeypatch, prof)
    finally:
        api.L.csh_emul_set_reverse(0)
