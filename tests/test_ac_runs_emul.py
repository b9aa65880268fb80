"""EOB runs resolved per 64-block word (k_entropy.hip k_ac_runs_words): one wave takes 16 consecutive slots of a stage, lane l reads the
record of slot cs0 + l / 4 and word 4 j + l % 4 of that slot's work item, and the wave walks its 64 words.  On the CPU emulation build; the same bodies run
on the MI355X in tests/test_ac_runs_gpu.py.

Every case compares each file with the oracle's, byte for byte, and with the same batch under CSH_AC_RUNS=slot (one wave per slot: the kernel before), in
the default, scalar and plain profiles, CSH_LIST_RUN at its default.  CASES below is the one list both files take their pictures from.

Which path a case takes is not left to its name: the emulation build counts the paths of the EOB-run kernels (csh_emul_ac_paths, k_entropy.hip) and every
case names the counters that must have moved in the run of the new kernel -- `need` in CASES, checked by test_emul_case in all three profiles:
  ordinary   runs stored on the common path (at most 14 blocks, or a first-pass run under 0x7FFF)
  serial     runs k_ac_runs_words resolved with eob_run_end / eob_run_serial (a refinement run of 15 to 512 blocks)
  cut937     sub-runs that eob_run_serial ended because more than 937 correction bits were pending
  long       runs appended to long_runs (end further than 8 words away) for k_ac_runs_long
  flush      frequency sums flushed because the work item changed inside a wave
  midwave    waves that begin at a slot which is not its work item's first
The block counts of the `edges` pictures (1, 63, 64, 65, 255, 256, 257, 1025) are asserted from the files' own headers."""
import ctypes
import io

import numpy as np
import pytest

from _util import emul_api, oracle_lossy, package

PROFILES = (None, "scalar", "plain")
PATHS = ("ordinary", "serial", "serial_refine", "cut937", "long", "flush", "midwave", "cut7fff")


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


def set_profile(monkeypatch, prof):
    if prof: monkeypatch.setenv("CSH_PROFILE", prof)
    else: monkeypatch.delenv("CSH_PROFILE", raising=False)


# ---- the tests' own pictures (grey: one component, so a scan's blocks are the picture's in raster order)
def grey_file(a, quality=92):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.asarray(a, np.uint8), "L").save(b, format="JPEG", quality=quality)
    return b.getvalue()


def busy(w, h, seed, amp=40):
    """noise of +- amp on a slow ramp: nearly every block codes something in every scan"""
    rng = np.random.default_rng(seed)
    ramp = np.add.outer(np.arange(h), np.arange(w)) * (60.0 / (w + h))
    return grey_file(np.clip(98 + ramp + rng.integers(-amp, amp + 1, (h, w)), 0, 255))


def spots(bw, bh, at, seed, amp=70):
    """flat but for the blocks (raster index) in `at`, which are noise: EOB runs from one spot to the next"""
    rng = np.random.default_rng(seed)
    a = np.full((8 * bh, 8 * bw), 128, np.int64)
    for i in at:
        y, x = divmod(i, bw)
        a[8 * y:8 * y + 8, 8 * x:8 * x + 8] += rng.integers(-amp, amp + 1, (8, 8))
    return grey_file(np.clip(a, 0, 255), quality=95)


def flat(w, h, value=128):
    return grey_file(np.full((h, w), value))


def heavy(bw, bh, every, seed):
    """every block carries the same few strong low frequencies (levels of 4 and more after quantisation: correction bits in every refinement scan, nothing new to
    code there), and every `every`-th block a little noise on top (something new): refinement runs of about `every` blocks, each with far more than 937 pending bits"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:8, 0:8]
    blk = np.zeros((8, 8))
    for (u, v, amp) in ((1, 0, 34), (0, 1, 30), (1, 1, 26), (2, 0, 22), (0, 2, 20), (2, 1, 18), (1, 2, 16), (3, 0, 14)):
        blk += amp * np.cos((2 * x + 1) * u * np.pi / 16) * np.cos((2 * y + 1) * v * np.pi / 16)
    a = np.tile(blk, (bh, bw)) + 128
    for i in range(every - 1, bw * bh, every):
        by, bx = divmod(i, bw)
        a[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] += rng.integers(-12, 13, (8, 8))
    return grey_file(np.clip(np.rint(a), 0, 255), quality=97)


def faint(w, h, seed, amp=3):
    rng = np.random.default_rng(seed)
    return grey_file(np.clip(128 + rng.integers(-amp, amp + 1, (h, w)), 0, 255), quality=95)


EDGE_SIZES = [(8, 8), (504, 8), (512, 8), (520, 8), (2040, 8), (2048, 8), (2056, 8), (328, 200)]
EDGE_BLOCKS = [1, 63, 64, 65, 255, 256, 257, 1025]
SPOTS_AT = (62, 63, 64, 65, 127, 128, 142, 157, 191)   # 128 -> 142: a run of 14 blocks, 142 -> 157: of 15; 191 -> the last block (205)


def gated_pictures():
    from test_refine_lists_emul import gated_set
    return [flat(264, 264, 90)] + gated_set()[0]


# name -> (pictures, jpeg quality, counters that must move with the new kernel, profiles)
CASES = {
    # block counts around the word and slot edges; eight work items per scan kind in one stage, so a wave holds several
    "edges": (lambda: [busy(w, h, 10 + i) for i, (w, h) in enumerate(EDGE_SIZES)], 80, ("ordinary", "flush"), PROFILES),
    # 520 x 520 = 4225 blocks = 17 slots per scan behind two files of one slot per scan: the wave edges fall inside the work items, at every offset
    "wave_edge": (lambda: [busy(64, 8, 20), busy(520, 8, 21), busy(520, 520, 22, amp=25)], 80, ("ordinary", "midwave", "flush"), PROFILES),
    # five pictures of 2, 3, 4, 5 and 3 slots per scan: the frequency flush at a change of work item, unit_base per lane
    "work_items": (lambda: [busy(184, 120, 30), busy(184, 184, 31), busy(264, 200, 32), busy(264, 264, 33), busy(208, 160, 34)], 80, ("ordinary", "flush"), PROFILES),
    # single noise blocks in a flat strip of 206 blocks: runs that end in the next word, of exactly 14 and 15 blocks, and one to the scan's last block;
    # the refinement scans' runs of 15 and more take eob_run_end / eob_run_serial across the word edges
    "word_edges": (lambda: [spots(206, 1, SPOTS_AT, 40), spots(103, 2, SPOTS_AT, 41, amp=25)], 80, ("ordinary", "serial_refine"), PROFILES),
    # one run over the whole scan: long_runs and k_ac_runs_long
    "flat": (lambda: [flat(520, 520), flat(264, 264, 60)], 80, ("long",), PROFILES),
    # refinement runs of 15 to about 500 blocks that carry correction bits: the 937-bit cut of eob_run_serial
    "corr_cut": (lambda: [heavy(65, 20, 97, 50), faint(520, 200, 51)], 80, ("serial_refine", "cut937"), PROFILES),
    # a conditional stage of the scan search that only some images ask for (work_active): a flat and busy pictures
    "gated": (gated_pictures, 80, ("ordinary",), (None, "scalar")),
}


def run_batch(api, srcs, p):
    b = api.batch(srcs, p)
    t = b.run()
    outs = b.fetch()
    b.close()
    return outs, t


def take_paths(api):
    """the emulation build's path counters since the last call, by name; None on the product library (it has none)"""
    if not hasattr(api.L, "csh_emul_ac_paths"):
        return None
    v = (ctypes.c_uint32 * 8)()
    api.L.csh_emul_ac_paths(v)
    return dict(zip(PATHS, v))


def blocks_of(out):
    from oracle import oracle as O
    d = O.decode(out)   # (owns what d.im points into)
    im = d.im
    return [im.comp[c].real_bw * im.comp[c].real_bh for c in range(im.ncomp)]


def check_case(api, monkeypatch, name, prof):
    make, quality, need, profs = CASES[name]
    assert prof in profs
    srcs = make()
    p = params(jpeg_quality=quality)
    set_profile(monkeypatch, prof)
    monkeypatch.delenv("CSH_LIST_RUN", raising=False)
    monkeypatch.delenv("CSH_AC_RUNS", raising=False)
    take_paths(api)
    outs, t = run_batch(api, srcs, p)
    paths = take_paths(api)
    monkeypatch.setenv("CSH_AC_RUNS", "slot")
    ref, _ = run_batch(api, srcs, p)
    slot_paths = take_paths(api)
    monkeypatch.delenv("CSH_AC_RUNS")
    for i, (src, o, r) in enumerate(zip(srcs, outs, ref)):
        assert isinstance(o, bytes), (name, i, o)
        assert o == r, ("per word != per slot", name, i, prof)
        assert o == oracle_lossy(src, quality), ("!= oracle", name, i, prof)
    if paths is not None:
        print(name, prof, paths)
        for k in need:
            assert paths[k] > 0, (name, prof, k, paths)
        assert slot_paths["flush"] == 0 and slot_paths["midwave"] == 0, slot_paths   # the switch did choose the other kernel
        for k in ("ordinary", "serial", "serial_refine", "cut937", "long", "cut7fff"):
            assert paths[k] == slot_paths[k], (name, prof, k, paths, slot_paths)
    if name == "edges":
        assert [blocks_of(o) for o in outs] == [[n] for n in EDGE_BLOCKS]
    if name == "wave_edge":
        assert blocks_of(outs[2]) == [4225]
    if name == "gated":
        assert t.n_search_extra >= 1, t.n_search_extra
    return outs


CASE_PROFILES = [(name, prof) for name in CASES for prof in CASES[name][3]]   # (the plain profile has no scan search: no gated stage)


@pytest.mark.parametrize("name,prof", CASE_PROFILES)
def test_emul_case(api, monkeypatch, name, prof):
    check_case(api, monkeypatch, name, prof)


# every launch's workgroups back to front: the sums of a wave meet counters its successors have added to already
def test_emul_back_to_front(api, monkeypatch):
    api.L.csh_emul_set_reverse.argtypes = [ctypes.c_int]
    api.L.csh_emul_set_reverse(1)
    try:
        for name in ("wave_edge", "corr_cut"):
            check_case(api, monkeypatch, name, None)
    finally:
        api.L.csh_emul_set_reverse(0)
