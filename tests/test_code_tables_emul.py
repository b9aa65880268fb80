"""The prefix codes in the files this library writes follow from the symbols those files code: every DEFLATE block's three codes, every lossless WebP
code and its code-length code, every table of a baseline JPEG are read back with readers written from the format specifications (tests/_deflate_read.py,
tests/_vp8l_parse.py, tests/_jpeg_read.py), the symbols each one codes are counted, and the transmitted lengths must be exactly what tests/_prefix_model.py
(T.81 K.2, written from the standard) makes of those counts.  The byte-parity tests compare the same files with the oracle, which is the same authors'
restatement of the same algorithm; this one compares them with the standard, on pictures skewed enough for the length limit to bind.  The functions take the
library: tests/test_zzz_code_tables_gpu.py runs them on the MI355X."""
import functools
import io

import numpy as np
import pytest
from PIL import Image

import _deflate_read as DR
import _jpeg_read as JR
import _prefix_model as M
import _vp8l_parse as V
from _util import emul_api, package, png_cases
from gen_synth import synth_jpeg
from test_webp_lossless_refs_emul import vp8l_mode

LADDER_SEED = 20240607


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


# ---------------------------------------------------------------------------------------------------- the pictures
@functools.lru_cache(None)
def ladder(width=256, height=256, steps=16):
    """8-bit grey: value (11 i + 3) % 256 occurs 2^i times for i = 0 .. steps - 1, the rest of the picture is the last value, all of it shuffled: a histogram whose
    Huffman code is steps - 1 bits deep before the end-of-block symbol and the matches are counted"""
    v = np.concatenate([np.full(1 << i, (11 * i + 3) % 256, np.uint8) for i in range(steps)])
    v = np.concatenate([v, np.full(width * height - len(v), v[-1], np.uint8)])
    return np.random.default_rng(LADDER_SEED).permutation(v).reshape(height, width)


def _saved(im, fmt, **kw):
    b = io.BytesIO()
    im.save(b, fmt, **kw)
    return b.getvalue()


@functools.lru_cache(None)
def ladder_png():
    return _saved(Image.fromarray(ladder(), "L"), "PNG")


@functools.lru_cache(None)
def png_inputs():
    small = dict(png_cases())
    return (("ladder_256x256", ladder_png()),) + tuple((n, small[n]) for n in ("RGB_200x150_3chunks", "RGBA_97x61", "palette_rgb_few"))


def depth_of(counts, limit):
    return M.limited_lengths(counts, limit)[1]


# ---------------------------------------------------------------------------------------------------- DEFLATE
def check_png_codes(name, png):
    """every dynamic block of the file: lit/len and distance lengths from the block's own symbols at limit 15, the code-length code from the header's own symbols
    at limit 7 -> (dynamic blocks, the unlimited lit/len depths)"""
    blocks, _ = DR.read_png(png)
    depths = []
    for k, b in enumerate(blocks):
        if b.btype != 2: continue
        what = f"{name}, block {k}"
        assert tuple(b.ll_len) == M.limited_lengths(b.ll_count, 15)[0], f"{what}: the literal/length code"
        assert tuple(b.d_len) == M.limited_lengths(b.d_count, 15)[0], f"{what}: the distance code"
        assert tuple(b.cl_len) == M.limited_lengths(b.cl_count, 7)[0], f"{what}: the code-length code"
        depths.append(depth_of(b.ll_count, 15))
    return sum(1 for b in blocks if b.btype == 2), depths


def run_deflate(api):
    """lossless PNG at levels 2 and 3 and the lossy PNG path.  A file that comes back unchanged (the "not smaller: return the input" rule) carries its writer's
    tables, not ours, and is left out -- counted, and never the ladder.  The ladder makes the lit/len limit bind: 15 used values of frequencies 1, 2, 4 ..
    plus the end-of-block symbol give an unlimited depth above 15 in at least one block (measured on the oracle: 1 block at 256 x 256)."""
    names, blobs = [n for n, _ in png_inputs()], [b for _, b in png_inputs()]
    left_out, dynamic, deepest = [], 0, {}
    for label, p in (("level 2", params(png_optimize=True, png_optimization_level=2)), ("level 3", params(png_optimize=True, png_optimization_level=3)),
                     ("lossy q80", params(png_optimize=False, png_optimization_level=3, png_quality=80))):
        outs = api.cs_batch_compress(blobs, p)
        for name, src, out in zip(names, blobs, outs):
            assert isinstance(out, bytes), (label, name, out)
            if out == src:
                left_out.append((label, name))
                continue
            n, depths = check_png_codes(f"{label}, {name}", out)
            dynamic += n
            deepest[(label, name)] = max(depths, default=0)
    print("DEFLATE: %d dynamic blocks checked; returned unchanged and left out: %s; deepest unlimited lit/len code per file: %s" % (dynamic, left_out, deepest))
    assert not [x for x in left_out if x[1].startswith("ladder")], left_out
    assert dynamic >= len(names)
    assert max(d for (_, n), d in deepest.items() if n.startswith("ladder")) > 15, "the ladder does not make the lit/len limit bind"


def test_emul_deflate_tables(api, capsys):
    with capsys.disabled():
        run_deflate(api)


# ---------------------------------------------------------------------------------------------------- lossless WebP
@functools.lru_cache(None)
def webp_inputs():
    """lossless WebP sources: the ladder as a grey picture, the ladder's histogram over 16 palette colours (an indexed picture: the colour-indexing transform packs
    two indices a byte), two pictures of the groups battery"""
    import test_webp_lossless_groups_emul as G
    from test_webp_lossless_palette_emul import source_of
    g = ladder()
    pal = np.random.default_rng(5).integers(0, 256, (256, 3), dtype=np.uint8)
    pics = dict(G.pictures())
    return (("ladder_256x256", source_of(np.dstack([g, g, g]))), ("ladder_indexed_256x256", source_of(pal[g])),
            ("halves_64x96", source_of(pics["halves_64x96"])), ("texture5", source_of(pics["texture5"])))


FIXED_DESCRIPTION = (4,) * 16 + (0, 0, 0)   # vp8l_pack.h Vp8lPut::code: the literal coder's descriptions give every length 0 .. 15 four bits and use no runs


def check_vp8l_codes(name, blob):
    """-> (codes checked, code-length codes checked, the deepest unlimited depth among the codes).  A description is either the literal coder's constant one --
    it states how many lengths it lists, and its code-length code is FIXED_DESCRIPTION, built from no histogram -- or the refs coder's, whose code-length code
    must follow from the code-length symbols the description uses, at limit 7"""
    st = V.parse(blob)
    checked, described, deepest = 0, 0, 0
    for where, group, which, c in st.codes:
        if c.simple or sum(1 for v in c.count if v) < 2: continue
        what = f"{name}: {where} group {group} code {which}"
        want, depth = M.limited_lengths(c.count, 15)
        assert tuple(c.lengths) == want, what
        if c.cl_counted:
            assert tuple(c.cl_lengths) == FIXED_DESCRIPTION, f"{what}: its description counts its lengths and is not the constant one"
        else:
            assert tuple(c.cl_lengths) == M.limited_lengths(c.cl_count, 7)[0], f"{what}: its code-length code"
            described += 1
        checked += 1
        deepest = max(deepest, depth)
    return checked, described, deepest


def run_vp8l(api):
    """plain, refs, palette and groups: every normally coded prefix code with at least two used symbols, and its code-length code.

    The limit binds here too, in every mode: the ladder as a grey picture (256 x 256, 2^16 pixels) gives the literal coder a green code 16 bits deep before the
    limit, and the 320 x 240 texture5 picture of the groups battery gives the refs / palette / groups coders codes 16 and 17 bits deep (emulation build; the depths
    are printed and the condition is asserted below).  The indexed ladder stays at 15: its indices are packed two to a byte before they are counted."""
    names, blobs = [n for n, _ in webp_inputs()], [b for _, b in webp_inputs()]
    for mode in ("plain", "refs", "palette", "groups"):
        with vp8l_mode(mode):
            outs = api.cs_batch_compress(blobs, params(webp_lossless=True))
        total, described, deepest = 0, 0, {}
        for name, out in zip(names, outs):
            assert isinstance(out, bytes), (mode, name, out)
            n, d, deepest[name] = check_vp8l_codes(f"{mode}, {name}", out)
            total, described = total + n, described + d
        print("VP8L %s: %d codes checked, %d of them with a code-length code of their own; deepest unlimited depth per file: %s" % (mode, total, described, deepest))
        assert total >= 2 * len(names) and (described >= 4 or mode == "plain")
        assert max(deepest.values()) > 15, f"{mode}: no code of any file has an unlimited depth above 15"


def test_emul_vp8l_tables(api, capsys):
    with capsys.disabled():
        run_vp8l(api)


# ---------------------------------------------------------------------------------------------------- baseline JPEG
JPEG_TEXTURED = (640, 480, 100.0)


@functools.lru_cache(None)
def jpeg_inputs():
    from test_webp_emul import webp_cases
    w, h, tex = JPEG_TEXTURED
    small = dict(webp_cases())
    return (("ladder_420", _saved(Image.fromarray(np.dstack([ladder()] * 3), "RGB"), "JPEG", quality=92, subsampling=2)),
            ("textured_420_%dx%d" % (w, h), synth_jpeg(9, w, h, texture=tex))) + tuple((n, small[n]) for n in ("420_160x96", "422_50x34", "grey_80x60"))


def check_jpeg_tables(name, blob):
    """-> {(class, id): unlimited depth}"""
    info = JR.read(blob)
    depths = {}
    for key, (bits, vals) in sorted(info.tables.items()):
        wbits, wvals, _, _, depth = M.jpeg_table(info.counts[key])
        assert depth <= 32
        assert (list(wbits), list(wvals)) == (bits, vals), f"{name}: the {'AC' if key[0] else 'DC'} table {key[1]}"
        depths[key] = depth
    return depths


def run_jpeg(api):
    """--jpeg-baseline (one sequential scan, optimal tables), grey and 4:2:0: each DHT is the model's table of the symbols its scan codes with it.
    The AC limit: the 640 x 480 picture of texture 100, the first size tried, makes it bind: the luma AC table's unlimited code is 18 bits deep, the chroma AC
    table's exactly 16 (emulation build; printed and asserted below).  The smaller pictures stay at 15 and under."""
    names, blobs = [n for n, _ in jpeg_inputs()], [b for _, b in jpeg_inputs()]
    outs = api.cs_batch_compress(blobs, params(jpeg_progressive=False))
    deepest = {}
    for name, out in zip(names, outs):
        assert isinstance(out, bytes), (name, out)
        deepest[name] = check_jpeg_tables(name, out)
    print("JPEG: unlimited depth per table (class, id): %s" % deepest)
    assert len(deepest["grey_80x60"]) == 2 and len(deepest["ladder_420"]) == 4
    assert max(d for (cls, _), d in deepest["textured_420_%dx%d" % JPEG_TEXTURED[:2]].items() if cls == 1) > 16, "no AC table binds the 16-bit limit"


def test_emul_jpeg_tables(api, capsys):
    with capsys.disabled():
        run_jpeg(api)
