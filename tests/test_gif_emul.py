"""GIF inputs under CSH_GIF=device, on the emulation build: the LZW decoder's tap against a decoder written from the GIF89a text, index for
index; the canvas tap against the model's composer (and Pillow where it composes alike); the optimiser's output against a Python statement of its rule, byte
for byte, and against what it must render; the fallbacks, the errors and the routing.  tests/test_zzz_gif_gpu.py runs the same checks on the device.
Every test but the unset-variable one fails without the route: CSH_GIF is unknown there and the csg_* symbols do not exist."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

import _gif_model as M
import _lzw_probe as L
import _gif_write as W
from _util import ROOT, emul_api, package

CW, CH = 48, 40
BAD_GIF, UNSUPPORTED, TOO_BIG = 50100, 10201, 10500
EMUL_CLI = os.path.join(ROOT, "tests", "emul", "caesiumclt_emul")


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


def colours(n, seed):
    rng = np.random.default_rng(seed)
    seen = []
    while len(seen) < n:
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        if c not in seen:
            seen.append(c)
    return seen


def noise(h, w, n, seed, low=0):
    return np.random.default_rng(seed).integers(low, n, (h, w))


# ------------------------------------------------------------------------------------------------ the decoder
def decoder_cases():
    """[(name, file, the indices written)]: one frame each, canvas = frame"""
    def one(name, idx, n, **kw):
        return name, W.gif(idx.shape[1], idx.shape[0], [W.frame(idx, **kw)], gct=colours(n, 1)), idx
    big = noise(70, 70, 256, 7)   # ~4900 codes at code size 8: the table fills once
    return [one("code size 2", noise(CH, CW, 4, 2), 4), one("code size 4", noise(CH, CW, 16, 3), 16), one("code size 8", noise(CH, CW, 256, 4), 256),
            one("clear on full", big, 256, clears="full"), one("deferred clear", big, 256, clears="never"),
            one("KwKwK runs", np.full((CH, CW), 3), 4), one("clear codes doubled", noise(CH, CW, 16, 5), 16, clears=50, double=True),
            one("no clear code in front", noise(CH, CW, 16, 6), 16, lead_clear=False),
            one("interlaced 1 x 1", noise(1, 1, 4, 8), 4, interlace=True), one("interlaced 5 x 9", noise(9, 5, 4, 9), 4, interlace=True),
            one("interlaced 48 x 40", noise(CH, CW, 16, 10), 16, interlace=True),
            one("sub-blocks of 1", noise(9, 11, 16, 11), 16, sub=1), one("sub-blocks of 255", noise(CH, CW, 256, 12), 256, sub=255),
            one("surplus data", noise(CH, CW, 16, 13), 16, surplus=b"\x55" * 7)]


def check_decoder(api):
    cases = decoder_cases()
    b = api.gif_batch([c[1] for c in cases])
    try:
        b.run()
        for i, (name, blob, idx) in enumerate(cases):
            want = M.frame_indices(M.parse(blob)["frames"][0])
            assert np.array_equal(want, idx), f"{name}: the model does not read what the writer wrote"
            assert np.array_equal(b.indices(i, 0, idx.shape[1], idx.shape[0]), want), name
    finally:
        b.close()


def test_emul_decoder_tap_equals_the_model(api):
    check_decoder(api)


# ------------------------------------------------------------------------------------------------ the canvases
def mixed_file(disposals):
    """six frames: local and global tables, partial rectangles at odd offsets that touch the right and the bottom edge, transparent pixels"""
    g, l1, l2 = colours(8, 20), colours(4, 21), colours(16, 22)
    def holes(idx, t, seed):
        idx = idx.copy()
        idx[np.random.default_rng(seed).random(idx.shape) < 0.4] = t
        return idx
    f = [W.frame(noise(CH, CW, 8, 23, low=1), disposal=disposals[0], delay=3),
         W.frame(holes(noise(7, 9, 8, 24, low=1), 0, 1), x=5, y=3, disposal=disposals[1], transparent=0, delay=4),
         W.frame(noise(7, 9, 4, 25), x=39, y=33, lct=l1, disposal=disposals[2], delay=5),
         W.frame(holes(noise(5, 13, 8, 26), 7, 2), x=11, y=7, disposal=disposals[3], transparent=7),
         W.frame(noise(3, 3, 16, 27), x=1, y=1, lct=l2, disposal=disposals[4], delay=1, interlace=True),
         W.frame(holes(noise(19, 31, 8, 28, low=1), 0, 3), x=17, y=21, disposal=disposals[5], transparent=0, delay=2)]
    return W.gif(CW, CH, f, gct=g, loop=0)


def pillow_canvases(blob):
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append(np.array(im.convert("RGBA")))
    return np.stack(out)


def check_canvases(api):
    every, plain = mixed_file([1, 2, 3, 0, 1, 2]), mixed_file([1, 0, 1, 0, 1, 0])
    got = api.gif_canvases([every, plain])
    assert np.array_equal(got[0], M.canvases_rgba(every))
    assert np.array_equal(got[1], M.canvases_rgba(plain))
    # Pillow is a witness for the file of disposals 0 / 1 alone: it fills a disposed rectangle with the background colour when no transparent index is in play,
    # where the model (and every browser) clears it to transparent
    assert np.array_equal(got[1], pillow_canvases(plain))


def test_emul_canvas_tap_equals_the_model_and_pillow(api):
    check_canvases(api)


# ------------------------------------------------------------------------------------------------ the output
def naive(frames_idx, gct, transparent=None, disposals=None, cw=CW, ch=CH, **kw):
    """the file written the naive way: whole-canvas frames, a clear code every 254 codes"""
    fr = [W.frame(idx, disposal=(disposals[k] if disposals else 1), transparent=transparent, delay=5 + k, clears=254) for k, idx in enumerate(frames_idx)]
    return W.gif(cw, ch, fr, gct=gct, loop=0, **kw)


def moving_block(n, nframes, seed, cw=CW, ch=CH):
    base = noise(ch, cw, n, seed)
    out = [base]
    for k in range(1, nframes):
        f = out[-1].copy()
        y, x = (3 + 5 * k) % (ch - 7), (2 + 9 * k) % (cw - 9)
        f[y:y + 7, x:x + 9] = noise(7, 9, n, seed + k)
        out.append(f)
    return out


def output_cases():
    g16, g256 = colours(16, 30), colours(256, 31)
    cases = {"moving block": naive(moving_block(15, 4, 32), g16, transparent=15), "single frame": naive(moving_block(15, 1, 33), g16),
             "a frame without change": naive([f for f in moving_block(15, 2, 34) for _ in (0, 1)], g16, transparent=15),
             "256 colours, no transparent index": naive(moving_block(256, 3, 35), g256)}
    # a transparent index behind the table's last entry that the output's code size still covers: 2 colours, code size 2, index 3
    fr = moving_block(2, 3, 38)
    cases["transparent index behind the table"] = naive([fr[0]] + [np.where(fr[k] != fr[k - 1], fr[k], 3) for k in (1, 2)], colours(2, 39), transparent=3)
    # un-painting: frame 0 is disposed of to transparent, the frames behind it paint a block each and leave the rest transparent
    fr = moving_block(15, 3, 36)
    for k in (1, 2):
        block = fr[k] != fr[k - 1] if k == 1 else fr[2] != fr[1]
        keep = fr[k].copy(); keep[:] = 15; keep[block] = fr[k][block]; keep[4 + k, 6] = 3
        fr[k] = keep
    cases["un-painting"] = naive(fr, g16, transparent=15, disposals=[2, 1, 1])
    # disposal 3: the block of frame 1 is taken back before frame 2 paints its own
    fr = moving_block(15, 3, 37)
    cases["disposal 3"] = naive([fr[0], np.where(fr[1] != fr[0], fr[1], 15), np.where(fr[2] != fr[1], fr[2], 15)], g16, transparent=15, disposals=[1, 3, 1])
    # the coder's dictionary look-up in its second step of 64 slots (tests/_lzw_probe.py; the replay proves each string does it): one row of 256 distinct colours, so
    # the coder is fed the string itself at code size 8.  (Nearly all of it codes as literals: the input is written in sub-blocks of one byte, so that the output is the smaller file.)
    for name, home, wraps in (("coder's second probe step", L.FIRST, False), ("coder's second probe step across the table's end", L.WRAPPING, True)):
        L.check(L.probe_string(home), 4096, wraps)
        idx = np.frombuffer(L.probe_string(home), np.uint8).astype(np.int64).reshape(1, -1)
        cases[name] = W.gif(idx.shape[1], 1, [W.frame(idx, disposal=1, delay=5, clears=254, sub=1)], gct=g256, loop=0)
    return cases


def seam_cases():
    """frames longer than three chunks at CSH_GIF_CHUNK=1024: 64 x 49, and 181 x 17 = 3 x 1024 + 5 pixels"""
    g = colours(16, 40)
    return {"64 x 49": naive(moving_block(15, 2, 41, 64, 49), g, transparent=15, cw=64, ch=49), "181 x 17": naive(moving_block(15, 2, 42, 181, 17), g, transparent=15, cw=181, ch=17)}


def run_batch(api, blobs, **kw):
    b = api.gif_batch(blobs, params(**kw))
    try:
        t = b.run()
        return b.fetch(), t
    finally:
        b.close()


def check_outputs(api, cases, pillow=()):
    names, blobs = list(cases), list(cases.values())
    outs, t = run_batch(api, blobs)
    assert t.n_failed == 0 and t.n_passed_palette == 0 and t.n_not_smaller == 0 and t.n_files == len(blobs)
    for name, src, out in zip(names, blobs, outs):
        assert not isinstance(out, Exception), (name, out)
        want, raised = M.optimise(src, t.chunk_pixels)
        assert raised is None, name
        assert out == want, f"{name}: the bytes differ from the model's"
        assert np.array_equal(M.canvases_rgba(out), M.canvases_rgba(src)), f"{name}: the output renders other canvases"
        if name in pillow:   # files of disposal 1 throughout, in and out
            assert np.array_equal(pillow_canvases(out), pillow_canvases(src)), name
        assert len(out) < len(src), name
    return dict(zip(names, outs)), t


def test_emul_outputs_equal_the_model_and_render_the_input(api):
    outs, t = check_outputs(api, output_cases(), pillow=("moving block", "single frame", "a frame without change", "256 colours, no transparent index", "transparent index behind the table"))
    assert t.chunk_pixels == 16384
    g = M.parse(outs["a frame without change"])
    assert [(f["w"], f["h"]) for f in g["frames"]][1] == (1, 1) and g["frames"][1]["x"] == 0
    g = M.parse(outs["un-painting"])
    assert g["frames"][0]["disposal"] == 2 and (g["frames"][1]["w"], g["frames"][1]["h"]) == (CW, CH)
    assert all(not f["interlace"] for f in g["frames"]) and outs["moving block"][:6] == b"GIF89a"


def test_emul_chunk_seams_and_the_bit_merge(api, monkeypatch):
    monkeypatch.setenv("CSH_GIF_CHUNK", "1024")
    outs, t = check_outputs(api, seam_cases(), pillow=("64 x 49", "181 x 17"))
    assert t.chunk_pixels == 1024


def test_emul_metadata_is_kept_under_keep_metadata_only(api):
    ext = [W.extension(0xFE, [b"a comment"]), W.extension(0xFF, [b"XMP DataXMP", b"<x/>"])]
    src = naive(moving_block(15, 3, 50), colours(16, 51), transparent=15, extensions=ext)
    (plain,), t = run_batch(api, [src])
    (kept,), _ = run_batch(api, [src], keep_metadata=True)
    assert plain == M.optimise(src, t.chunk_pixels)[0] and kept == M.optimise(src, t.chunk_pixels, keep_metadata=True)[0]
    assert b"a comment" not in plain and b"a comment" in kept and b"NETSCAPE2.0" in plain and len(kept) == len(plain) + sum(map(len, ext))


# ------------------------------------------------------------------------------------------------ fallbacks and errors
def check_fallbacks(api):
    fr = moving_block(15, 3, 60)
    # frame 0's colours are its own table's; frame 1 is taken back (disposal 3), so frame 2 would have to paint them from the global table
    foreign = W.gif(CW, CH, [W.frame(fr[0], lct=colours(16, 61), disposal=1, clears=254), W.frame(np.where(fr[1] != fr[0], fr[1], 15), disposal=3, transparent=15, clears=254),
                             W.frame(np.where(fr[2] != fr[1], fr[2], 15), disposal=1, transparent=15, clears=254)], gct=colours(16, 62))
    assert M.optimise(foreign, 16384) == (None, "palette")
    base = naive(fr, colours(16, 63), transparent=15)
    minimal = M.optimise(base, 16384)[0]
    text = W.gif(CW, CH, [W.frame(fr[0], clears=254)], gct=colours(16, 64), extensions=[W.extension(0x01, [bytes(12), b"glyphs"])])
    # a transparent index the output's code size cannot code: a 16-colour table (code size 4 out), data at code size 8, index 200.  Pillow reads it
    wide = W.gif(CW, CH, [W.frame(np.where(fr[k] != fr[k - 1], fr[k], 200) if k else fr[0], disposal=1, transparent=200, mcs=8, clears=254) for k in range(3)], gct=colours(16, 65))
    assert M.optimise(wide, 16384) == (None, "index")
    assert np.array_equal(pillow_canvases(wide), M.canvases_rgba(wide))
    outs, t = run_batch(api, [foreign, base, minimal, text, wide])
    assert outs[0] == foreign and outs[2] == minimal and outs[3] == text and outs[1] == minimal and outs[4] == wide
    assert (t.n_passed_palette, t.n_not_smaller, t.n_failed) == (2, 1, 0)
    b = api.gif_batch([wide])   # the taps still read such a file
    try:
        b.run()
        assert np.array_equal(np.stack([b.canvas(0, k) for k in range(3)]), M.canvases_rgba(wide))
    finally:
        b.close()


def test_emul_fallbacks_return_the_input(api):
    check_fallbacks(api)


def malformed_cases():
    g = colours(4, 70)
    idx = noise(CH, CW, 4, 71)
    good = W.gif(CW, CH, [W.frame(idx)], gct=g)
    bw = W.BitWriter(); bw.put(4, 3); bw.put(1, 3); bw.put(7, 3); bw.put(7, 4)   # clear, 1, 7 (the next free entry is 6)
    first = W.BitWriter(); first.put(4, 3); first.put(6, 3)                        # the first code behind a clear code must be a colour
    return {"truncated data": good[:len(good) // 2], "truncated table": good[:20], "rectangle leaves the canvas": W.gif(CW, CH, [W.frame(idx, x=1)], gct=g),
            "code size 1": W.gif(CW, CH, [W.frame(idx % 2, mcs=1)], gct=g), "code size 9": W.gif(CW, CH, [W.frame(idx, mcs=9)], gct=g),
            "no trailer": W.gif(CW, CH, [W.frame(idx)], gct=g, trailer=False), "no frame": W.gif(CW, CH, [], gct=g),
            "a code beyond the next free entry": W.gif(CW, CH, [W.frame(idx, data=bw.bytes())], gct=g),
            "a first code beyond the colours": W.gif(CW, CH, [W.frame(idx, data=first.bytes())], gct=g),
            "data ends early": W.gif(CW, CH, [W.frame(idx, data=W.lzw_encode(list(idx.flat)[:900], 2))], gct=g),
            "data ends without an end code": W.gif(CW, CH, [W.frame(idx, data=W.lzw_encode(list(idx.flat)[:900], 2, end=False))], gct=g)}


def check_malformed(api):
    good = naive(moving_block(15, 2, 72), colours(16, 73), transparent=15)
    cases = malformed_cases()
    blobs = [good]
    for bad in cases.values():
        blobs += [bad, good]
    for name, bad in cases.items():
        with pytest.raises(M.BadGif):
            M.compose(M.parse(bad))
    outs, t = run_batch(api, blobs)
    want = M.optimise(good, t.chunk_pixels)[0]
    for i, name in enumerate(cases):
        assert isinstance(outs[1 + 2 * i], Exception) and outs[1 + 2 * i].code == BAD_GIF, name
    assert all(o == want for o in outs[0::2]) and t.n_failed == len(cases)


def test_emul_malformed_files_fail_alone(api):
    check_malformed(api)


# ------------------------------------------------------------------------------------------------ routing
def mixed_call():
    from gen_synth import synth_jpeg, synth_png
    gif = naive(moving_block(15, 3, 80), colours(16, 81), transparent=15)
    return [synth_jpeg(0, 64, 48, texture=20), synth_png(2, 40, 30, "RGB", compress_level=1), gif, b"II*\x00" + bytes(64)]


def check_routing(api, monkeypatch):
    blobs = mixed_call()
    gif = blobs[2]
    monkeypatch.delenv("CSH_GIF", raising=False)
    plain = api.cs_batch_compress(blobs, params())
    assert plain[2] == gif and plain[3] == blobs[3]
    monkeypatch.setenv("CSH_GIF", "device")
    dev = api.cs_batch_compress(blobs, params())
    want = M.optimise(gif, 16384)[0]
    assert dev[2] == want and len(want) < len(gif) and [dev[i] for i in (0, 1, 3)] == [plain[i] for i in (0, 1, 3)]
    assert api.compress_in_memory(gif, params()) == want
    with pytest.raises(Exception) as e:   # a resize of a GIF file is refused as before
        api.compress_in_memory(gif, params(width=24))
    assert e.value.code == UNSUPPORTED
    # the size walk: one run, then the target rule on the optimised size
    assert api.batch_compress_to_size([gif], params(), len(want), return_smallest=False) == [want]
    r = api.batch_compress_to_size([gif], params(), len(want) - 1, return_smallest=False)[0]
    assert isinstance(r, Exception) and r.code == TOO_BIG and "no device path" not in str(r)
    assert api.batch_compress_to_size([gif], params(), len(want) - 1, return_smallest=True) == [want]
    monkeypatch.setenv("CSH_GIF", "bogus")
    bogus = api.cs_batch_compress(blobs, params())
    assert isinstance(bogus[2], Exception) and bogus[2].code == UNSUPPORTED and "CSH_GIF" in str(bogus[2])
    assert [bogus[i] for i in (0, 1, 3)] == [plain[i] for i in (0, 1, 3)]


def test_emul_routing_under_each_setting(api, monkeypatch):
    check_routing(api, monkeypatch)


@pytest.mark.parametrize("value", [None, "", "pass"])
def test_emul_gif_is_passed_through_without_the_variable(api, monkeypatch, value):
    """passes on the code before the route too, on purpose: the variable is opt-in"""
    if value is None:
        monkeypatch.delenv("CSH_GIF", raising=False)
    else:
        monkeypatch.setenv("CSH_GIF", value)
    blobs = mixed_call()
    outs = api.cs_batch_compress(blobs, params())
    assert outs[2] == blobs[2] and outs[3] == blobs[3] and not isinstance(outs[0], Exception) and not isinstance(outs[1], Exception)


def run_cli_over_a_gif(binary, tmp_path):
    gif = naive(moving_block(15, 3, 90), colours(16, 91), transparent=15)
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    (src / "a.gif").write_bytes(gif)
    r = subprocess.run([binary, "-q", "80", "-R", "-o", str(out), str(src)], capture_output=True, text=True, env=dict(os.environ, CSH_GIF="device"))
    assert r.returncode == 0, r.stderr
    assert (out / "a.gif").read_bytes() == M.optimise(gif, 16384)[0]


def test_emul_cli_writes_the_smaller_file(api, tmp_path):
    run_cli_over_a_gif(EMUL_CLI, tmp_path)


# ------------------------------------------------------------------------------------------------ order independence
@pytest.mark.parametrize("switch", ["csh_emul_set_reverse", "csh_emul_set_jacobi"])
def test_emul_outputs_do_not_depend_on_the_launch_order(api, monkeypatch, switch):
    fn = getattr(api.L, switch)
    fn.argtypes = [ctypes.c_int]
    fn(1)
    try:
        check_decoder(api)
        check_canvases(api)
        check_outputs(api, output_cases())
        monkeypatch.setenv("CSH_GIF_CHUNK", "1024")
        check_outputs(api, seam_cases())
    finally:
        fn(0)


def test_header_binding_and_libraries_agree_on_the_gif_entry_points(api):
    import re
    hdr = open(os.path.join(ROOT, "include", "caesium_hip.h")).read()
    declared = set(re.findall(r"\b(csg_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(package().binding.GIF_EXPORTS) and "CS_ERR_BAD_GIF = 50100" in hdr
    for lib in (api.L, ctypes.CDLL(package().library_path())):
        for name in sorted(declared):
            assert hasattr(lib, name), name
    assert api.gif_kernel_names()[:7] == ["gif_lzw_decode", "gif_anim_stats", "gif_anim_pack", "gif_lzw_encode", "gif_layout", "gif_frame_head", "gif_merge"]


def test_emul_an_oversize_canvas_is_refused_alone_and_counted_by_the_extent(api):
    """a canvas of more than 2^28 pixels has no device path: that file alone answers CS_ERR_UNSUPPORTED; cs_batch_extent counts a GIF as canvas x frames from
    its header and blocks (two such files exceed one group's pool estimate, two files whose header says nothing do not)"""
    g = colours(4, 95)
    huge = W.gif(30000, 30000, [W.frame(noise(2, 2, 4, 96))], gct=g)
    good = naive(moving_block(15, 2, 97), colours(16, 98), transparent=15)
    outs, t = run_batch(api, [huge, good])
    assert isinstance(outs[0], Exception) and outs[0].code == UNSUPPORTED and outs[1] == M.optimise(good, t.chunk_pixels)[0]
    wide = W.gif(65535, 65535, [W.frame(noise(2, 2, 4, 96))], gct=g)
    assert api.batch_extent([(len(wide), wide)] * 2) == 1 and api.batch_extent([(len(good), good)] * 2) == 2
    assert api.batch_extent([(64, b"GIF89a" + bytes(7))] * 2) == 2
