"""List runs (k_aclist.hip): k_list_stats, k_list_pack and k_list_refine take one wave per run of up to CSH_LIST_RUN consecutive chunks
of a work item, not one per chunk.  On the CPU emulation build; the same bodies run on the MI355X in tests/test_list_runs_gpu.py.

Every check compares three things: the files with the oracle's, byte for byte; the files with the same call under CSH_LIST_RUN=1 (one wave per chunk: the
mapping before there were runs); and csh_timing.n_list_runs with the sum of ceil(chunks / R) over the progressive AC work items the run coded from the lists
-- a run that ignored the switch fails there.  Small pictures with R = 2 and 3 put many run boundaries into few blocks; every group runs once more with
CSH_LIST_RUN unset (R=None below: the default, what ships) on pictures of more than DEFAULT_RUN luma chunks, so that a full run and a remainder both occur.

The work items of a file are counted here from the plan's rules (batch_plan.cpp output_scans / plan_search_stages / plan_trellis) and from what the FILE
says about its search, not from anything the library reports:
  plain    the stock script: luma 1-5 and 6-63 at Al 2 and its two refinements (4), each chroma component 1-63 at Al 1 and its refinement (2)
  search   stage 1: per component the two band scans at Al 0, 1, 2 and the refinements 1 -> 0, 2 -> 1 (8); stage 2: the whole band, the splits at 2 and 5 (5);
           luma at Al 3 (its refinement and two band scans: 3) for a file whose luma ended at Al >= 2 (jcmaster.c: Al 3 is tried when 2 beat 1); the split
           at 12 (2) where the split at 8 led after the third -- the file's split is 8, 12 or 18 --, the split at 18 (2) where 12 then led -- 12 or 18;
           luma and chroma (both components together) apart
  default  the search, and the trellis quantiser's statistics scan (1 per component)"""
import ctypes
import io

import numpy as np
import pytest

from _util import emul_api, oracle_lossy, package
from gen_synth import synth_jpeg, synth_rgb

PROFILES = (None, "scalar", "plain")
DEFAULT_RUN = 8   # kernels.h CSH_LIST_RUN


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


def set_profile(monkeypatch, prof):
    if prof: monkeypatch.setenv("CSH_PROFILE", prof)
    else: monkeypatch.delenv("CSH_PROFILE", raising=False)


def set_run(monkeypatch, R):
    if R is None: monkeypatch.delenv("CSH_LIST_RUN", raising=False)
    else: monkeypatch.setenv("CSH_LIST_RUN", str(R))


def grey_jpeg(w, h, seed, texture=20, quality=90):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(synth_rgb(seed, w, h, texture)).convert("L").save(b, format="JPEG", quality=quality)
    return b.getvalue()


def noise_jpeg(w, h, seed, subsampling, quality):
    from PIL import Image
    rng = np.random.default_rng(seed)
    b = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(b, format="JPEG", quality=quality, subsampling=subsampling)
    return b.getvalue()


def flat_jpeg(w, h, value, grey=False):
    from PIL import Image
    img = Image.fromarray(np.full((h, w, 3), value, np.uint8))
    b = io.BytesIO()
    if grey: img.convert("L").save(b, format="JPEG", quality=92)
    else: img.save(b, format="JPEG", quality=92, subsampling=2)
    return b.getvalue()


# ---- the model of n_list_runs
def file_work_items(out, prof):
    """[(chunks, list-coded progressive AC work items)] per component of one output file"""
    from oracle import oracle as O
    d = O.decode(out)
    im, scans = d.im, d.scans()
    nch = [-(-(im.comp[c].real_bw * im.comp[c].real_bh) // 256) for c in range(im.ncomp)]
    if prof == "plain":
        return [(nch[c], 4 if c == 0 else 2) for c in range(im.ncomp)]
    items = []
    for c in range(im.ncomp):
        group = 0 if c == 0 else 1   # the search decides for both chroma components together: read Cb's scans
        first = [s for s in scans if tuple(s[0]) == (group,) and s[1] == 1 and s[3] == 0]
        assert len(first) == 1, (first, scans)
        split, Al = first[0][2], first[0][4]
        assert split in (63, 2, 8, 5, 12, 18), split
        n = 8 + 5
        if c == 0 and Al >= 2: n += 3
        if split in (8, 12, 18): n += 2
        if split in (12, 18): n += 2
        if prof is None: n += 1
        items.append((nch[c], n))
    return items


def expected_runs(outs, prof, R, progressive=True):
    if not progressive:
        return 0
    return sum(n * -(-nch // R) for o in outs for nch, n in file_work_items(o, prof))


def gated_items(outs, prof):
    """work items of the search's conditional stages among the files'"""
    return sum(n - 13 - (1 if prof is None else 0) for o in outs for _, n in file_work_items(o, prof))


def run_batch(api, srcs, p):
    b = api.batch(srcs, p)
    t = b.run()
    outs = b.fetch()
    b.close()
    return outs, t


def check_group(api, monkeypatch, srcs, prof, R, want=oracle_lossy, p=None, progressive=True):
    """one batch at R (None: the default) and at 1: the oracle's bytes, the same bytes, the run counts of both.  Returns the files"""
    p = p or params(jpeg_progressive=progressive)
    set_profile(monkeypatch, prof)
    set_run(monkeypatch, R)
    outs, t = run_batch(api, srcs, p)
    set_run(monkeypatch, 1)
    ref, t1 = run_batch(api, srcs, p)
    set_run(monkeypatch, None)
    for i, (src, o, r) in enumerate(zip(srcs, outs, ref)):
        assert isinstance(o, bytes), (i, o)
        assert o == r, ("runs != one wave per chunk", i, prof, R)
        assert o == want(src), ("!= oracle", i, prof, R)
    Rv = DEFAULT_RUN if R is None else R
    assert t.n_list_runs == expected_runs(outs, prof, Rv, progressive), (t.n_list_runs, expected_runs(outs, prof, Rv, progressive), prof, R)
    assert t1.n_list_runs == expected_runs(outs, prof, 1, progressive), (t1.n_list_runs, expected_runs(outs, prof, 1, progressive), prof)
    return outs


# the pictures of the cases at the default R: 528 x 256 is 66 x 32 = 2112 luma blocks, nine chunks -- a full run of eight and a run of one behind it; its 4:2:0
# chroma has 33 x 16 = 528 blocks, three chunks: one short run
BIG_W, BIG_H = 528, 256


# ---- 1. run boundaries: 4:2:0 pictures whose luma has 1, 2, 3 and 5 chunks (23 and 33 blocks a row: the real width is not the padded one)
BOUNDARY = [(16, 16, 30), (184, 120, 45), (184, 184, 25), (264, 264, 60)]


def boundary_set():
    return [synth_jpeg(40 + i, w, h, subsampling=2, texture=tex) for i, (w, h, tex) in enumerate(BOUNDARY)]


def check_boundaries(api, monkeypatch, prof, R):
    outs = check_group(api, monkeypatch, boundary_set(), prof, R)
    assert [file_work_items(o, prof)[0][0] for o in outs] == [1, 2, 3, 5]


@pytest.mark.parametrize("R", (2, 3))
@pytest.mark.parametrize("prof", PROFILES)
def test_emul_boundaries(api, monkeypatch, prof, R):
    check_boundaries(api, monkeypatch, prof, R)


# luma exactly 8 chunks (chroma 2), and 9 (chroma 3): at the default R a full run, and a full run with a run of one behind it
def check_default_run(api, monkeypatch, prof):
    outs = check_group(api, monkeypatch, big_set(), prof, None)
    assert [[nch for nch, _ in file_work_items(o, prof)] for o in outs] == [[8, 2, 2], [9, 3, 3]]


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_default_run(api, monkeypatch, prof):
    check_default_run(api, monkeypatch, prof)


# grey, 4:4:4 and 4:2:2, once each
def check_layouts(api, monkeypatch, prof, R=2):
    if R is None: gw, gh, w4, h4, w2, h2, chunks = BIG_W, BIG_H, BIG_W, BIG_H, BIG_W, BIG_H, ([9], [9, 9, 9], [9, 5, 5])
    else: gw, gh, w4, h4, w2, h2, chunks = 184, 120, 184, 120, 264, 136, ([2], [2, 2, 2], [3, 2, 2])
    outs = check_group(api, monkeypatch, [grey_jpeg(gw, gh, 60, texture=30)], prof, R)
    assert [nch for nch, _ in file_work_items(outs[0], prof)] == chunks[0]
    for ss, src, want in ((444, synth_jpeg(61, w4, h4, subsampling=0, texture=40), chunks[1]), (422, synth_jpeg(62, w2, h2, subsampling=1, texture=40), chunks[2])):
        outs = check_group(api, monkeypatch, [src], prof, R, want=lambda s: oracle_lossy(s, 80, subsampling=ss), p=params(jpeg_chroma_subsampling=ss))
        assert [nch for nch, _ in file_work_items(outs[0], prof)] == want, ss


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", PROFILES)
def test_emul_layouts(api, monkeypatch, prof, R):
    check_layouts(api, monkeypatch, prof, R)


# ---- 2. the window carried across chunks: noise at q 98 -- a run's bits slide the packer's LDS window several times and cross the chunk edges mid-word
def check_dense_window(api, monkeypatch, prof, R=3):
    q = 98
    srcs = [noise_jpeg(BIG_W, BIG_H, 7, 2, q) if R is None else noise_jpeg(184, 184, 7, 2, q)]
    check_group(api, monkeypatch, srcs, prof, R, want=lambda s: oracle_lossy(s, q), p=params(jpeg_quality=q))


@pytest.mark.parametrize("R", (3, None))
@pytest.mark.parametrize("prof", PROFILES)
def test_emul_dense_window(api, monkeypatch, prof, R):
    check_dense_window(api, monkeypatch, prof, R)


# ---- 3. flat pictures: lists of END entries only -- the EOB runs span chunks and runs; a last chunk of a single block
def check_flat(api, monkeypatch, prof, R=2):
    if R is None: srcs, chunks = [flat_jpeg(BIG_W, BIG_H, 128), flat_jpeg(8 * 2049, 8, 90, grey=True), grey_jpeg(8 * 2049, 8, 70, texture=25)], [9, 9, 9]
    else: srcs, chunks = [flat_jpeg(264, 264, 128), flat_jpeg(8 * 257, 8, 90, grey=True), grey_jpeg(8 * 257, 8, 70, texture=25)], [5, 2, 2]
    outs = check_group(api, monkeypatch, srcs, prof, R)
    assert [file_work_items(o, prof)[0][0] for o in outs] == chunks


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", PROFILES)
def test_emul_flat(api, monkeypatch, prof, R):
    check_flat(api, monkeypatch, prof, R)


# ---- 4. gated stages of the search: several images of which only some ask for them -- a run of an inactive work item does nothing
def gated_big_set():
    """(seed, texture) of 528 x 256 pictures at q 80, found like test_refine_lists_emul.gated_set's: some of their searches run into a conditional stage, others into none"""
    return [synth_jpeg(sd, BIG_W, BIG_H, texture=tx) for sd, tx in GATED_BIG]


GATED_BIG = [(4, 90), (0, 10), (0, 0), (1, 90)]


def check_gated_stage(api, monkeypatch, prof, R=2, quality=80):
    from test_refine_lists_emul import gated_set
    srcs = gated_big_set() if R is None else gated_set()[0]
    outs = check_group(api, monkeypatch, srcs, prof, R, want=lambda s: oracle_lossy(s, quality), p=params(jpeg_quality=quality))
    per_file = [gated_items([o], prof) for o in outs]
    assert any(per_file) and not all(per_file), per_file   # some files went through a conditional stage, others through none


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", (None, "scalar"))
def test_emul_gated_stage(api, monkeypatch, prof, R):
    check_gated_stage(api, monkeypatch, prof, R)


# ---- 5. pools that overflow: every pool starts at a sixteenth of its estimate -- lists without room (chunks without entries) and scans without room sit inside runs
def big_set():
    return [synth_jpeg(50, 512, 256, subsampling=2, texture=35), synth_jpeg(51, BIG_W, BIG_H, subsampling=2, texture=50)]


def check_pools_that_overflow(api, monkeypatch, prof, R=2):
    """The files are right, and the run counts, with pools sixteen times too small at the start.  NOT asserted: that a retry happened at all -- csh_timing
    has no count of them; with pools at a sixteenth of estimates that are a few times the need it is likely, not proven (tests/test_refine_lists_emul.py
    check_pools_that_overflow says the same of its own).  In a pass that had no room the emulation build's k_list_pack stops if a run gets ahead of its sized
    place ("Where k_list_pack's stores end"): these cases run under that check.  Nor does any GPU case tell a plain store on a run's last word from the atomicOr: that takes the
    neighbouring run to have written first, which only test_emul_back_to_front arranges, on the emulation build"""
    monkeypatch.setenv("CSH_TEST_POOL_SHIFT", "4")
    check_group(api, monkeypatch, big_set() if R is None else boundary_set(), prof, R)


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", PROFILES)
def test_emul_pools_that_overflow(api, monkeypatch, prof, R):
    check_pools_that_overflow(api, monkeypatch, prof, R)


# ---- 6. re-runs: run() twice on one batch; a re-quantisation re-run (the lists are built by k_nzlist, not by the transform)
def check_reruns(api, monkeypatch, prof, R=2):
    set_profile(monkeypatch, prof)
    srcs = big_set() if R is None else boundary_set()[1:]
    quals = [33, 97, 60][:len(srcs)]
    got = {}
    for run in (R, 1):
        set_run(monkeypatch, run)
        b = api.batch(srcs, params())
        b.retain_dct()
        t1 = b.run(); first = b.fetch()
        t2 = b.run(); second = b.fetch()
        b.set_quality(quals)
        t3 = b.rerun_encode(); third = b.fetch()
        b.close()
        assert first == second
        Rv = DEFAULT_RUN if run is None else run
        assert t1.n_list_runs == t2.n_list_runs == expected_runs(first, prof, Rv), (t1.n_list_runs, t2.n_list_runs, expected_runs(first, prof, Rv))
        assert t3.n_list_runs == expected_runs(third, prof, Rv), (t3.n_list_runs, expected_runs(third, prof, Rv))
        got[run] = (first, third)
    set_run(monkeypatch, None)
    assert got[R] == got[1]
    for src, o in zip(srcs, got[R][0]):
        assert o == oracle_lossy(src)
    for src, o, q in zip(srcs, got[R][1], quals):
        assert o == oracle_lossy(src, q), q


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", PROFILES)
def test_emul_reruns(api, monkeypatch, prof, R):
    check_reruns(api, monkeypatch, prof, R)


# ---- 7. sequential output: no list slots, no runs
def check_sequential(api, monkeypatch, prof, R=2):
    check_group(api, monkeypatch, big_set()[1:] if R is None else boundary_set()[:3], prof, R, want=lambda s: oracle_lossy(s, progressive=0), progressive=False)


@pytest.mark.parametrize("R", (2, None))
@pytest.mark.parametrize("prof", PROFILES)
def test_emul_sequential(api, monkeypatch, prof, R):
    check_sequential(api, monkeypatch, prof, R)


# ---- 8. emulation only: every launch's workgroups in reverse -- a run's last word meets the word its successor has written already
def test_emul_back_to_front(api, monkeypatch):
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    api.L.csh_emul_set_reverse(1)
    try:
        for prof in PROFILES:
            check_boundaries(api, monkeypatch, prof, 2)
            check_dense_window(api, monkeypatch, prof)
    finally:
        api.L.csh_emul_set_reverse(0)
