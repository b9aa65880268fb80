"""GIF inputs under CSH_GIF=lossy, on the emulation build: the candidate rows' tap against the model's lists, row by row; the route's bytes
against tests/_gif_lossy_model.py, byte for byte; what the output renders against the bound (alpha equal, every opaque pixel within D of the input's, on every
canvas); sizes against the exact route's; launch order, routing, the CLI, the entry points.  tests/test_zzz_gif_lossy_gpu.py runs the same checks on the device.
Every test fails without the route: CSH_GIF=lossy is refused there and csg_batch_create_lossy / csg_batch_read_near do not exist."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _gif_lossy_model as LM
import _gif_model as M
import _gif_write as W
import test_gif_emul as E
from _util import ROOT, emul_api, package

CW, CH = E.CW, E.CH
RAMP16 = [(6 * i, 6 * i, 6 * i) for i in range(16)]   # neighbours 108 apart (squared), the next ones 432


@pytest.fixture(scope="module")
def api():
    return emul_api()


# ------------------------------------------------------------------------------------------------ the inputs
def cube_colours(n, seed, lo=100, hi=140):
    rng = np.random.default_rng(seed)
    seen = []
    while len(seen) < n:
        c = tuple(int(v) for v in rng.integers(lo, hi, 3))
        if c not in seen:
            seen.append(c)
    return seen


@functools.lru_cache(maxsize=None)
def ramp16(cw=CW, ch=CH, seed=100):
    """noise over the indices 0..14 of a grey ramp, transparent index 15, three frames"""
    return E.naive(E.moving_block(15, 3, seed, cw, ch), RAMP16, transparent=15, cw=cw, ch=ch)


@functools.lru_cache(maxsize=None)
def cube256():
    """256 distinct colours of a cube of side 40, no transparent index, 70 x 70: at D = 20 most lists reach the cut at 63, at D = 99 every one does"""
    return E.naive(E.moving_block(256, 2, 101, 70, 70), cube_colours(256, 102), cw=70, ch=70)


@functools.lru_cache(maxsize=None)
def random256():
    return E.naive(E.moving_block(256, 2, 103, 70, 70), E.colours(256, 104), cw=70, ch=70)


@functools.lru_cache(maxsize=None)
def duplicates():
    """16 entries, the upper 8 repeat the lower 8: PACK writes the lower index, and no list may name an upper one"""
    return E.naive(E.moving_block(16, 2, 105), RAMP16[:8] + RAMP16[:8])


@functools.lru_cache(maxsize=None)
def transparent_among_near():
    """the ramp with the transparent index in its middle, at 7: indices 6 and 8 are painted all over, and 7 must neither replace them nor be replaced"""
    fr = [np.where(f >= 7, f + 1, f) for f in E.moving_block(15, 3, 106)]
    return E.naive(fr, RAMP16, transparent=7)


@functools.lru_cache(maxsize=None)
def tables_and_indices():
    """one global table under two transparent indices (frame 1: 15, frame 2: 3), then local tables of 4 and of 16 entries: the list is the table's, the
    exclusion the frame's, n the table's"""
    fr = E.moving_block(15, 3, 107)
    l4 = [(200 + 5 * i, 40, 40) for i in range(4)]
    l16 = [(30, 120 + 4 * i, 200) for i in range(16)]
    f = [W.frame(fr[0], disposal=1, delay=2, clears=254),
         W.frame(np.where(fr[1] != fr[0], fr[1], 15), disposal=1, transparent=15, delay=3, clears=254),
         W.frame(np.where((fr[2] != fr[1]) & (fr[2] != 3), fr[2], 3), disposal=1, transparent=3, delay=4, clears=254),
         W.frame(E.noise(15, 20, 4, 108), x=3, y=5, lct=l4, disposal=1, delay=5, clears=254),
         W.frame(E.noise(21, 23, 16, 109), x=25, y=19, lct=l16, disposal=1, delay=6, clears=254)]
    return W.gif(CW, CH, f, gct=RAMP16, loop=0)


def seam_cases():
    return {"181 x 17": ramp16(181, 17, 110), "64 x 49": ramp16(64, 49, 111)}


# ------------------------------------------------------------------------------------------------ the checks
def run_lossy(api, blobs, quality, **kw):
    b = api.gif_batch(blobs, E.params(gif_quality=quality, **kw), lossy=True)
    try:
        t = b.run()
        return b.fetch(), t
    finally:
        b.close()


@functools.lru_cache(maxsize=None)
def model(blob, chunk, quality):
    tally = {}
    out, raised = LM.optimise(blob, chunk, quality, tally=tally)
    return out, raised, tally.get("clears", 0)


@functools.lru_cache(maxsize=None)
def exact(blob, chunk):
    return M.optimise(blob, chunk)[0]


def check_rendering(name, src, out, D, pillow=False):
    a, b = M.canvases_rgba(out).astype(np.int64), M.canvases_rgba(src).astype(np.int64)
    assert a.shape == b.shape, name
    assert np.array_equal(a[..., 3], b[..., 3]), f"{name}: alpha differs"
    d2 = ((a[..., :3] - b[..., :3]) ** 2).sum(axis=-1)
    worst = int(d2[b[..., 3] == 255].max(initial=0))
    print(f"{name}: D^2 = {D * D}, worst squared distance {worst}")
    assert worst <= D * D, f"{name}: an opaque pixel lies {worst} (squared) from the input's, beyond {D * D}"
    if pillow:   # files of disposal 1 throughout, in and out
        pa, pb = E.pillow_canvases(out).astype(np.int64), E.pillow_canvases(src).astype(np.int64)
        assert np.array_equal(pa[..., 3], pb[..., 3]), f"{name}: alpha differs (Pillow)"
        assert int((((pa[..., :3] - pb[..., :3]) ** 2).sum(axis=-1))[pb[..., 3] == 255].max(initial=0)) <= D * D, f"{name}: beyond the bound (Pillow)"


def check_outputs(api, cases, quality, pillow=(), smaller=()):
    """the route's bytes are the model's; the output renders within D of the input; it is no larger than the exact route's file (smaller: strictly)"""
    names, blobs = list(cases), list(cases.values())
    outs, t = run_lossy(api, blobs, quality)
    D = LM.distance(quality)
    assert t.lossy_distance == D and t.n_failed == 0 and t.n_passed_palette == 0 and t.n_not_smaller == 0 and t.n_files == len(blobs)
    for name, src, out in zip(names, blobs, outs):
        assert not isinstance(out, Exception), (name, out)
        want, raised, _ = model(src, t.chunk_pixels, quality)
        assert raised is None, name
        assert out == want, f"{name} at quality {quality}: the bytes differ from the model's"
        check_rendering(name, src, out, D, name in pillow)
        dev = exact(src, t.chunk_pixels)
        print(f"{name} at quality {quality}: {len(src)} -> exact {len(dev)}, lossy {len(out)}")
        assert len(out) <= len(dev), f"{name}: larger than the exact route's file"
        if D == 0:
            assert out == dev, name
        if name in smaller:
            assert len(out) < len(dev), f"{name}: not smaller than the exact route's file"
    return dict(zip(names, outs)), t


def check_near(api, blob, quality, frames=(0,), cut=None):
    """the tap's rows of the tables the frames use equal the model's lists.  cut: at least that many rows reach the cap of 64 candidates"""
    b = api.gif_batch([blob], E.params(gif_quality=quality), lossy=True)
    try:
        b.run()
        for k in frames:
            rows, count = b.near(0, k)
            lists = LM.frame_lists(blob, k, quality)
            wrows, wcount = LM.near_arrays(lists)
            for i in range(256):
                assert count[i] == wcount[i] and np.array_equal(rows[i], wrows[i]), (f"frame {k}, row {i}", list(rows[i][:count[i]]), lists[i])
            if cut is not None:
                assert int((count == 64).sum()) >= cut
    finally:
        b.close()


def ramp_cases():
    return {"ramp16": ramp16(), "transparent among near colours": transparent_among_near(), "duplicates": duplicates(), "tables and indices": tables_and_indices()}


DISPOSAL_1 = ("ramp16", "transparent among near colours", "duplicates", "tables and indices", "cube256", "random256", "181 x 17", "64 x 49")


def check_ramp(api):
    for q in (100, 90):   # nothing is near: the exact route's file
        outs, _ = check_outputs(api, {"ramp16": ramp16()}, q)
        assert outs["ramp16"] == exact(ramp16(), 16384)
    check_outputs(api, ramp_cases(), 80, pillow=DISPOSAL_1, smaller=("ramp16",))
    check_outputs(api, ramp_cases(), 50, pillow=DISPOSAL_1, smaller=("ramp16",))


def check_cube(api):
    check_outputs(api, {"cube256": cube256()}, 80, pillow=DISPOSAL_1, smaller=("cube256",))
    check_outputs(api, {"cube256": cube256()}, 1, pillow=DISPOSAL_1, smaller=("cube256",))
    # a clear code behind a full table inside a lossy stream
    check_outputs(api, {"cube256": cube256()}, 95, pillow=DISPOSAL_1)
    check_outputs(api, {"random256": random256()}, 80, pillow=DISPOSAL_1)
    assert model(cube256(), 16384, 95)[2] > 0 and model(random256(), 16384, 80)[2] > 0, "no table fills any more: the case has stopped covering the clear code"


def check_near_taps(api):
    check_near(api, ramp16(), 80)
    lists = LM.frame_lists(ramp16(), 0, 80)
    assert lists[5] == [5, 4, 6] and lists[0] == [0, 1] and lists[14] == [14, 13, 15] and lists[15] == [15, 14]   # a tie resolves to the lower index; the list ignores the transparent index
    check_near(api, ramp16(), 50)
    assert max(len(v) for v in LM.frame_lists(ramp16(), 0, 50)) == 9
    check_near(api, ramp16(), 100)
    check_near(api, cube256(), 80, cut=128)
    check_near(api, cube256(), 1, cut=256)
    check_near(api, duplicates(), 50)
    lists = LM.frame_lists(duplicates(), 0, 50)
    assert all(v < 8 for b in range(8) for v in lists[b]) and all(lists[b] == [b] for b in range(8, 256))
    check_near(api, tables_and_indices(), 80, frames=(0, 2, 3, 4))
    assert [len(v) for v in LM.frame_lists(tables_and_indices(), 3, 80)[:6]] == [4, 4, 4, 4, 1, 1]


def check_seams(api, monkeypatch):
    monkeypatch.setenv("CSH_GIF_CHUNK", "1024")
    _, t = check_outputs(api, seam_cases(), 80, pillow=DISPOSAL_1, smaller=("181 x 17", "64 x 49"))
    assert t.chunk_pixels == 1024


def check_disposals(api):
    check_outputs(api, E.output_cases(), 50)


def test_emul_near_tap_equals_the_model(api):
    check_near_taps(api)


def test_emul_ramp_outputs_equal_the_model_within_the_bound(api):
    check_ramp(api)


def test_emul_cube_outputs_under_the_cut_and_a_full_table(api):
    check_cube(api)


def test_emul_chunk_seams(api, monkeypatch):
    check_seams(api, monkeypatch)


def test_emul_disposal_cases(api):
    check_disposals(api)


def test_emul_distance_0_is_the_exact_coder(api, monkeypatch):
    monkeypatch.setenv("CSH_GIF_CHUNK", "1024")
    outs, t = run_lossy(api, [ramp16(), cube256()], 100)
    assert t.lossy_distance == 0 and t.kernel_ms[7] == 0   # the exact route's launches
    for blob, out in zip((ramp16(), cube256()), outs):
        assert LM.optimise(blob, 1024, 100) == M.optimise(blob, 1024) == (out, None)
    # the figures of one 48 x 40 frame of the ramp: 100 / 80 / 50
    px = list(E.noise(CH, CW, 15, 112).flat)
    table = np.array([c[0] | (c[1] << 8) | (c[2] << 16) | 0xFF000000 for c in RAMP16], dtype=np.uint32)
    sizes = [len(LM.encode_chunks(px, 4, 16384, LM.near_lists(table, 16, LM.distance(q)), 15, 16)) for q in (100, 80, 50)]
    assert sizes[0] == len(M.encode_chunks(px, 4, 16384)) and sizes[0] > sizes[1] > sizes[2], sizes


# ------------------------------------------------------------------------------------------------ order independence
@pytest.mark.parametrize("switch", ["csh_emul_set_reverse", "csh_emul_set_jacobi"])
def test_emul_outputs_do_not_depend_on_the_launch_order(api, monkeypatch, switch):
    fn = getattr(api.L, switch)
    fn.argtypes = [ctypes.c_int]
    fn(1)
    try:
        check_near(api, ramp16(), 50)
        check_near(api, cube256(), 80)
        check_outputs(api, ramp_cases(), 50)
        check_outputs(api, {"cube256": cube256()}, 80)
        check_seams(api, monkeypatch)
    finally:
        fn(0)


# ------------------------------------------------------------------------------------------------ routing
def check_routing(api, monkeypatch):
    blobs = E.mixed_call() + [ramp16()]
    gifs = (2, 4)
    monkeypatch.delenv("CSH_GIF", raising=False)
    plain = api.cs_batch_compress(blobs, E.params())
    monkeypatch.setenv("CSH_GIF", "device")
    dev = api.cs_batch_compress(blobs, E.params())
    assert [dev[i] for i in gifs] == [exact(blobs[i], 16384) for i in gifs]
    assert api.cs_batch_compress(blobs, E.params(gif_quality=50)) == dev   # the exact route reads no quality
    monkeypatch.setenv("CSH_GIF", "lossy")
    assert api.cs_batch_compress(blobs, E.params(gif_quality=100)) == dev
    low = api.cs_batch_compress(blobs, E.params(gif_quality=50))
    assert [low[i] for i in gifs] == [model(blobs[i], 16384, 50)[0] for i in gifs] and len(low[4]) < len(dev[4])
    assert [low[i] for i in (0, 1, 3)] == [plain[i] for i in (0, 1, 3)]
    gif = blobs[4]
    assert api.compress_in_memory(gif, E.params(gif_quality=50)) == low[4]
    assert api.compress_in_memory(gif, E.params(gif_quality=0)) == api.compress_in_memory(gif, E.params(gif_quality=1)) == model(gif, 16384, 1)[0]
    assert api.compress_in_memory(gif, E.params(gif_quality=250)) == dev[4]
    with pytest.raises(Exception) as e:   # a resize of a GIF file is refused as before
        api.compress_in_memory(gif, E.params(width=24))
    assert e.value.code == E.UNSUPPORTED
    # the size walk: one run at the quality given, then the target rule
    want = low[4]
    assert api.batch_compress_to_size([gif], E.params(gif_quality=50), len(want), return_smallest=False) == [want]
    r = api.batch_compress_to_size([gif], E.params(gif_quality=50), len(want) - 1, return_smallest=False)[0]
    assert isinstance(r, Exception) and r.code == E.TOO_BIG
    assert api.batch_compress_to_size([gif], E.params(gif_quality=50), len(want) - 1, return_smallest=True) == [want]
    monkeypatch.setenv("CSH_GIF", "bogus")
    bogus = api.cs_batch_compress(blobs, E.params())
    assert all(isinstance(bogus[i], Exception) and bogus[i].code == E.UNSUPPORTED and "lossy" in str(bogus[i]) for i in gifs)


def test_emul_routing_under_lossy(api, monkeypatch):
    check_routing(api, monkeypatch)


def run_cli_over_a_gif(binary, tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    (src / "a.gif").write_bytes(ramp16())
    for flags, want in ((["-q", "50"], model(ramp16(), 16384, 50)[0]), (["--lossless"], exact(ramp16(), 16384))):
        out = tmp_path / ("out" + flags[0].strip("-"))
        r = subprocess.run([binary] + flags + ["-R", "-o", str(out), str(src)], capture_output=True, text=True, env=dict(os.environ, CSH_GIF="lossy"))
        assert r.returncode == 0, r.stderr
        assert (out / "a.gif").read_bytes() == want, flags


def test_emul_cli_under_lossy(api, tmp_path):
    run_cli_over_a_gif(E.EMUL_CLI, tmp_path)


def test_header_binding_and_libraries_agree_on_the_lossy_entry_points(api):
    hdr = open(os.path.join(ROOT, "include", "caesium_hip.h")).read()
    declared = set(re.findall(r"\b(csg_[a-z_0-9]+)\s*\(", hdr))
    for name in ("csg_batch_create_lossy", "csg_batch_read_near"):
        assert name in declared and name in package().binding.GIF_EXPORTS
        for lib in (api.L, ctypes.CDLL(package().library_path())):
            assert hasattr(lib, name), name
    assert "lossy_distance" in hdr and api.gif_kernel_names()[7] == "gif_near"
