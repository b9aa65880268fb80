"""WebP INPUTS, the stream shapes libwebp's encoder never writes.  The VP8 and VP8L decoders (vp8_dec.h, vp8l_dec.h, k_webp_dec.hip) are held to libwebp
sample for sample, but every stream of tests/test_webp_decode_emul.py came out of libwebp's own encoder, which uses a narrow slice of both formats.  Here
the streams are written by tests/_vp8_write.py and tests/_vp8l_write.py, field by field and token by token: every frame-header field of VP8 (filter type,
level, sharpness, filter deltas, 1 / 2 / 4 / 8 token partitions, segments in absolute and delta mode, the five quantiser index deltas, the skip flag off
and on, coefficient-probability updates), every prediction mode at every edge, macroblocks that code nothing without being skipped; for VP8L every form
of code description, codes of every depth, 2 .. 24 prefix-code groups that collide in the decoder's eight cache slots, a group count past the point
where the decoder stops building 256-entry tables and one past its arena, colour caches of 1 .. 11 bits, the four transforms in every order and tile
size, all 14 predictor modes at the picture's edges, copies at all 120 neighbourhood codes, and the ALPH chunk's four filters over both methods.

Judge: libwebp through Pillow, np.asarray(Image.open(...).convert("RGB" | "RGBA")), exact equality of every sample.  libwebp must decode EVERY generated
stream: one it refuses is a bug of the writer, not a skipped case.  All blobs of a test go to ONE webp_decode call (pictures are the parallel axis).
tests/test_zzz_webp_streams_gpu.py runs the same cases through the product library on the device."""
import functools
import io
import itertools

import numpy as np
import pytest
from PIL import Image

import _vp8_write as V
import _vp8l_write as L
from _util import emul_api
from gen_synth import synth_rgb


@pytest.fixture(scope="module")
def api():
    return emul_api()


def judge(name, blob):
    try:
        return np.asarray(Image.open(io.BytesIO(blob)).convert("RGBA"))
    except Exception as e:   # noqa: BLE001 -- whatever Pillow raises for a stream libwebp refuses
        pytest.fail("libwebp refuses %s (%s): the writer wrote something invalid" % (name, e))


def same_picture(got, want):
    """want: libwebp's RGBA.  An opaque picture comes back as RGB, one with transparency as RGBA"""
    if isinstance(got, Exception):
        return False
    if (want[:, :, 3] == 255).all():
        want = want[:, :, :3]
    return got.shape == want.shape and np.array_equal(got, want)


def check(api, cases):
    wants = [judge(name, blob) for name, blob in cases]
    outs = api.webp_decode([blob for _, blob in cases])
    bad = [(name, got if isinstance(got, Exception) else "pixels differ") for (name, _), got, want in zip(cases, outs, wants) if not same_picture(got, want)]
    assert not bad, (len(bad), len(cases), bad[:8])


# =====================================================================================================================================  VP8

SIZES = [(48, 32), (70, 41), (33, 47), (80, 64)]   # 3 x 2 .. 5 x 4 macroblocks, most of them off the 16-grid


def frame(seed, size, amplitude=None, mb_kw=None, **hdr):
    rng = np.random.default_rng(seed)
    kw = dict(mb_kw or {})
    kw.setdefault("amplitude", [1.0, 0.2, 0.05, 0.02][seed % 4] if amplitude is None else amplitude)   # (small residuals: differences near the filter's thresholds)
    hdr.setdefault("base_q", int(rng.integers(0, 30)))
    return V.random_frame(rng, size[0], size[1], mb_kw=kw, **hdr)


@functools.lru_cache(None)
def vp8_filter_cases():
    """both filter types x levels {0, 1, 14, 15, 39, 40, 63} (the two hev thresholds from both sides) x sharpness 0 .. 7 (the > 4 shift, the 9 - sharp cap)"""
    out = []
    for simple in (0, 1):
        for level in (0, 1, 14, 15, 39, 40, 63):
            for sharp in range(8):
                k = len(out)
                out.append(("filter simple%d level%d sharp%d" % (simple, level, sharp), frame(1000 + k, SIZES[k % 4], simple=simple, level=level, sharpness=sharp)))
    return out


@functools.lru_cache(None)
def vp8_lf_delta_cases():
    """ref_delta[0] and mode_delta[0], positive and negative, the sum driven below 0 and above 63, i4 and i16 macroblocks both present; the other six deltas
    (inter frames' business) set and without effect; the flag set with nothing sent"""
    out = []
    for k, (level, ref0, mode0) in enumerate([(10, -20, None), (10, None, -20), (60, 10, None), (60, None, 10), (30, -63, 63), (30, 63, -63), (30, 5, -3), (1, -1, None),
                                              (1, None, -1), (62, 1, 1), (20, -19, 0), (20, -10, -10), (50, 13, 1), (33, -20, 30), (40, None, None), (15, 0, -1), (39, 0, 1)]):
        for simple in (0, 1):
            lf = {"update": 1, "ref": [ref0, 7, -9, 63], "mode": [mode0, -63, 5, None]}
            out.append(("lf_delta level%d ref%s mode%s simple%d" % (level, ref0, mode0, simple),
                        frame(2000 + 2 * k + simple, SIZES[k % 4], simple=simple, level=level, sharpness=k % 8, lf_delta=lf, mb_kw={"p_i4": 0.5})))
    out.append(("lf_delta nothing sent", frame(2100, SIZES[1], level=25, lf_delta={"update": 0})))
    return out


@functools.lru_cache(None)
def vp8_partition_cases():
    """1 / 2 / 4 / 8 token partitions over 9 macroblock rows (partitions get 2, 2, 1 ... rows): the 3-byte size table, the row's partition, the hand-back of its
    reader at the end of the row; with rows that are skipped whole, so that some partitions carry no token at all; one partition longer than 65535 bytes"""
    out = []
    for log2 in range(4):
        n = 1 << log2
        for j, skip_rows in enumerate([(), {1: (0, 1, 2, 3, 4, 5, 6, 7, 8), 2: (1, 3, 5, 7), 4: (1, 5), 8: (3,)}[n], {1: (4,), 2: (0, 2, 4, 6, 8), 4: (0, 4, 8, 3, 7), 8: (0, 8, 5)}[n]]):
            for size in ((41, 140), (70, 139)):
                out.append(("partitions %d skip_rows %s %dx%d" % (n, skip_rows, size[0], size[1]),
                            frame(3000 + len(out), size, log2_parts=log2, level=20 * (j & 1), mb_kw={"skip_rows": skip_rows})))
    # the third byte of a partition's size: 8 x 8 macroblocks, every coefficient in the largest category at probabilities that make each branch cost a byte
    mbs = []
    for k in range(64):
        mb = V.MB(i4=1, bmodes=[(k + b) % 10 for b in range(16)], uvmode=k % 4)
        mb.levels[:24] = 67 + (np.arange(24 * 16).reshape(24, 16) + k) % 3
        mb.levels[:24, 1::2] *= -1
        mbs.append(mb)
    blob = V.write_frame(128, 128, mbs, log2_parts=1, base_q=0, level=9, coef_updates={i: 255 for i in range(1056)})
    first = int.from_bytes(blob[20:23], "little") >> 5
    assert int.from_bytes(blob[30 + first:33 + first], "little") >= 1 << 16
    out.append(("partitions 2, the first of more than 64 KiB", blob))
    return out


@functools.lru_cache(None)
def vp8_segment_cases():
    """segment map sent or not, values absolute or deltas, quantisers and filter levels that clamp at both ends (0 and 127 / 117 for the chroma DC index / 63),
    map probabilities including 0 and 255, the segment header with nothing sent (absolute zeros)"""
    out = []
    sets = [(1, 50, 30, [0, 127, 64, None], [0, 63, 20, None]), (1, 50, 30, [127, 3, None, 120], [63, None, 1, 40]), (1, 50, 30, [-5, 127, -127, 3], [-1, 63, -63, 2]),
            (0, 10, 30, [-30, 127, 0, 5], [-40, 40, None, 3]), (0, 120, 5, [20, -127, None, -7], [-5, 63, -1, 20]),
            (0, 64, 60, [-64, 63, -65, 64], [3, 4, -60, -61]), (0, 0, 1, [None, 1, 126, 127], [None, -1, 62, 63])]
    probs = [None, (0, 255, 128), (255, 0, 1), (128, 128, 128), (1, 1, 254), (0, 0, 0), (255, 255, 255), (None, 7, None)]
    for k, (absolute, base_q, level, quant, levels) in enumerate(sets):
        for update_map in (0, 1):
            for j in range(len(probs) if update_map else 1):
                seg = {"update_map": update_map, "update_data": 1, "abs": absolute, "quant": quant, "level": levels, "probs": probs[j]}
                qd = [(0, 0, 0, 0, 0), (0, 0, 0, 15, 0), (0, 0, 0, -15, 0), (5, -5, 5, 12, -12)][(k + j) % 4]
                out.append(("segments abs%d base_q%d map%d probs%s q_delta%s" % (absolute, base_q, update_map, probs[j], qd),
                            frame(4000 + len(out), SIZES[len(out) % 4], segment=seg, base_q=base_q, level=level, simple=j & 1, q_delta=qd)))
    for update_map in (0, 1):
        seg = {"update_map": update_map, "update_data": 0, "probs": (100, 50, 200)}
        out.append(("segments nothing sent map%d" % update_map, frame(4900 + update_map, SIZES[1], segment=seg, base_q=50, level=30)))
    return out


@functools.lru_cache(None)
def vp8_index_delta_cases():
    """each of the five quantiser index deltas (y1 dc, y2 dc, y2 ac, uv dc, uv ac) at +-15 with the base index near 0 and near 127: the clamps at both ends,
    the 117 clamp of the chroma DC index, the floor of 8 under the y2 ac step"""
    out = []
    for which in range(5):
        for d in (-15, 15):
            for base in (0, 3, 110, 124, 127):
                qd = [0] * 5
                qd[which] = d
                out.append(("index delta %d = %d at base %d" % (which, d, base), frame(5000 + len(out), SIZES[len(out) % 4], base_q=base, q_delta=tuple(qd), level=10 * (len(out) % 3))))
    for k, qd in enumerate([(15, 15, 15, 15, 15), (-15, -15, -15, -15, -15), (1, -2, 3, -4, 5), (-15, 15, -15, 15, -15)]):
        for base in (2, 60, 113, 126):
            out.append(("index deltas %s at base %d" % (qd, base), frame(5500 + len(out), SIZES[len(out) % 4], base_q=base, q_delta=qd)))
    return out


@functools.lru_cache(None)
def vp8_skip_cases():
    """use_skip 0 and 1, skip_p in {0, 1, 255} (and a plain one), many macroblocks whose skip flag is clear but that code nothing -- libwebp's decoder leaves
    their inner edges unfiltered, i16 macroblocks with a Y2 block of nothing but zero tokens included -- with the filter on, both types"""
    out = []
    for simple in (0, 1):
        for use_skip, skip_p in ((0, 0), (1, 0), (1, 1), (1, 255), (1, 128)):
            for j in range(3):
                out.append(("skip use%d p%d simple%d #%d" % (use_skip, skip_p, simple, j),
                            frame(6000 + len(out), SIZES[len(out) % 4], amplitude=[0.3, 0.05, 0.02][j], use_skip=use_skip, skip_p=skip_p, simple=simple,
                                  level=[20, 45, 8][j], sharpness=j, mb_kw={"p_empty": 0.45, "p_skip": 0.2})))
    return out


@functools.lru_cache(None)
def vp8_probability_cases():
    """coefficient-probability updates: none, all of them, and 0 / 1 / 255 at the branch nodes (end of block, zero, one)"""
    out = []
    rng = np.random.default_rng(7)
    for k in range(4):
        out.append(("probabilities none #%d" % k, frame(7000 + k, SIZES[k % 4])))
        out.append(("probabilities all #%d" % k, frame(7010 + k, SIZES[k % 4], coef_updates={i: int(v) for i, v in enumerate(rng.integers(0, 256, 1056))})))
        out.append(("probabilities all extreme #%d" % k, frame(7020 + k, SIZES[k % 4], coef_updates={i: int(v) for i, v in enumerate(rng.choice([0, 1, 255], 1056))})))
        out.append(("probabilities branch nodes #%d" % k, frame(7030 + k, SIZES[k % 4], coef_updates={i: int(rng.choice([0, 1, 255])) for i in range(1056) if i % 11 < 3})))
        out.append(("probabilities some #%d" % k, frame(7040 + k, SIZES[k % 4], coef_updates={int(i): int(rng.integers(0, 256)) for i in rng.choice(1056, 200, replace=False)})))
    return out


@functools.lru_cache(None)
def vp8_mode_cases():
    """modes drawn uniformly: each of the ten 4 x 4 modes and the four 16 x 16 / chroma modes at every edge class within a few frames (127 / 129 borders, the
    top-right samples of sub-block rows 1 - 3, the right-most macroblock); prediction alone (everything skipped), with residuals, filtered and not;
    frames of a single macroblock, a single row and a single column; the colour-space, clamp and version bits, which change nothing"""
    out = []
    for k, size in enumerate([(48, 32), (70, 41), (80, 64), (16, 16), (1, 1), (17, 1), (1, 17), (64, 48), (33, 47), (15, 70), (100, 15)]):
        for j in range(4):
            out.append(("modes %dx%d #%d" % (size[0], size[1], j),
                        frame(8000 + len(out), size, level=[0, 30, 0, 12][j], simple=j >> 1 & 1, color_space=j & 1, clamp=j >> 1 & 1, version=j,
                              mb_kw={"p_i4": 0.65, "p_skip": [1.0, 0.5, 0.1, 0.3][j]})))
    return out


def libwebp_knob_cases():
    """libwebp's own encoder with the knobs Pillow leaves alone: simple filter, sharpness 3 .. 7, 2 / 4 / 8 partitions, 1 .. 4 segments -- realistic content
    under the header shapes above.  None where no libwebp with the encoder API loads"""
    try:
        from libwebp_pin import libwebp_encode, libwebps
        libs = libwebps()
    except Exception:   # noqa: BLE001 -- no oracle build, no library
        libs = []
    if not libs:
        return None
    W = libs[-1][1]
    out = []
    # WebPConfig fields by index: 6 segments, 8 filter_strength, 9 filter_sharpness, 10 filter_type (0 simple), 18 partitions (log2)
    for k, cfg in enumerate([{"10": 0}, {"10": 0, "9": 3, "8": 80}, {"9": 4}, {"9": 5, "8": 100}, {"9": 7, "8": 20}, {"18": 1}, {"18": 2, "6": 1}, {"18": 3, "6": 2}, {"6": 3, "18": 3, "9": 6}]):
        rgb = np.ascontiguousarray(synth_rgb(500 + k, 150, 141, texture=10.0 * (k % 4)))
        out.append(("libwebp %s" % cfg, libwebp_encode(W, rgb, [40, 75, 90][k % 3], **cfg)))
    return out


@functools.lru_cache(None)
def vp8_wide_case():
    """a frame of 129 x 65 macroblocks: wider than 2048 samples, where the device's reconstruction has rows r and r + 64 in flight together on one scratch slot"""
    yy, xx = np.mgrid[0:1040, 0:2064]
    rgb = np.dstack([(xx // 8 + yy // 16) % 256, (xx // 3 * 5 + yy) % 256, ((xx // 64) * 37 + (yy // 64) * 11) % 256]).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(b, format="WEBP", quality=30, method=0)
    return [("wide 2064x1040", b.getvalue())]


def test_emul_vp8_filter_types_levels_and_sharpness(api):
    check(api, vp8_filter_cases())


def test_emul_vp8_filter_deltas(api):
    check(api, vp8_lf_delta_cases())


def test_emul_vp8_token_partitions(api):
    check(api, vp8_partition_cases())


def test_emul_vp8_segments(api):
    check(api, vp8_segment_cases())


def test_emul_vp8_quantiser_index_deltas(api):
    check(api, vp8_index_delta_cases())


def test_emul_vp8_skip_flag_and_empty_macroblocks(api):
    check(api, vp8_skip_cases())


def test_emul_vp8_coefficient_probability_updates(api):
    check(api, vp8_probability_cases())


def test_emul_vp8_prediction_modes_at_the_edges(api):
    check(api, vp8_mode_cases())


def test_emul_vp8_libwebp_encoder_knobs(api):
    cases = libwebp_knob_cases()
    if cases is None:
        pytest.skip("no libwebp with the encoder API loads here")
    check(api, cases)


def test_emul_vp8_frame_wider_than_2048(api):
    check(api, vp8_wide_case())


def test_vp8_writer_holds_its_own_bounds():
    """the writer refuses content beyond the transform bounds, and its boolean encoder never starts a partition with 0xFF"""
    mb = V.MB(i4=1)
    mb.levels[0][0] = 2047
    with pytest.raises(AssertionError):
        V.write_frame(16, 16, [mb], base_q=127)
    mb = V.MB(i4=0)
    mb.levels[3][1:] = 70
    with pytest.raises(AssertionError):
        V.write_frame(16, 16, [mb], base_q=0)
    e = V.BoolEnc()
    for _ in range(64):
        e.put(1, 1)   # the interval's upper end, as far as it goes
    assert e.finish()[0] != 0xFF


# =====================================================================================================================================  VP8L

def argb(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64)


def sub_shape(w, h, bits):
    return ((h + (1 << bits) - 1) >> bits, (w + (1 << bits) - 1) >> bits)


def lossless(seed, w, h, *, transforms=(), cache_bits=0, meta=None, make=None, events=None, ev_kw=None, alpha_used=1, info=None):
    rng = np.random.default_rng(seed)
    xs = L.packed_width(w, transforms)
    if events is None:
        events = L.random_events(rng, xs, h, cache_bits=cache_bits, **(ev_kw or {}))
    make = make or L.default_code_maker(rng)
    return L.vp8l_file(L.write_stream(w, h, events, make, transforms=transforms, cache_bits=cache_bits, meta=meta, alpha_used=alpha_used,
                                      sub_make=L.default_code_maker(rng), info=info))


def colliding_groups(n, shape):
    """group of every tile such that neighbouring tiles alternate between groups 8 (and 16) apart: they share a slot of the decoder's 8-slot cache"""
    t = np.arange(shape[0] * shape[1])
    g = (t // 3) % 8 + 8 * (t % 3) if n > 16 else (t // 2) % 8 + 8 * (t % 2) if n > 8 else t % n
    g = g % n
    g[-1] = n - 1
    return g.reshape(shape)


@functools.lru_cache(None)
def vp8l_group_cases():
    """2, 9 and 24 prefix-code groups, assigned so that g and g + 8 (and g + 16) alternate tile to tile: a conflict refill of the decoder's direct-mapped slots at
    every tile; tile sizes 4 .. 32; copies that run across tiles and rows and re-pick the group behind them"""
    out = []
    for n in (2, 9, 24):
        for prec, (w, h) in ((2, (67, 21)), (3, (130, 40)), (4, (256, 70)), (5, (255, 128))):
            for cb in (0, 6):
                out.append(("groups %d tile bits %d cache %d" % (n, prec, cb),
                            lossless(9000 + len(out), w, h, cache_bits=cb, meta=(prec, colliding_groups(n, sub_shape(w, h, prec))), ev_kw={"p_copy": 0.2})))
    return out


# the decoder's prefix-code arena, in 16-bit units, as vp8l_dec.h sizes and fills it (vp8l_arena_bytes, vp8l_entropy, lsetup_pixels, lbuild)
def arena_model(stream_bytes, groups):
    """groups: per group the number of coded symbols of its five codes -> (groups built without 256-entry tables, fits)"""
    cap = (4 * 1024 * 1024 + 16 * stream_bytes) // 2 - 2328 // 2 - 8    # vp8l_arena_bytes / 2 less the code-length scratch
    used = 270 * len(groups)                                            # (sizeof(LGroup) + 1) / 2 = 5 codes of 108 bytes
    if used > cap:
        return 0, False
    without = 0
    for nsyms in groups:
        tables = 0
        for n in nsyms:
            want_lut = used + 4096 < cap - cap // 4                      # lsetup_pixels: tables while a quarter of the arena is free
            if n <= 1:
                continue                                                # a single symbol: nothing stored
            if used + n > cap:
                return without, False
            used += n
            if want_lut and used + 257 <= cap:
                used += (used & 1) + 256
                tables += 1
        without += tables < sum(1 for n in nsyms if n > 1)
    return without, True


def pooled_maker(rng, variants, needs, maxlen=15, flat=False):
    """the codes of group g are those of variant g % variants: few distinct codes to write, many groups to hold.  needs[k]: the symbols every variant of code k
    must have; flat: every symbol of the alphabet, at two neighbouring lengths, rotated per variant"""
    base = L.default_code_maker(rng, maxlen=maxlen, extra=(0, 0), forms=False)
    pool = {}

    def make(g, k, need, alphabet):
        key = (g % variants, k)
        if key not in pool:
            if flat:
                fl = L.flat_lengths(alphabet)
                r = (7 * key[0]) % alphabet
                pool[key] = L.Code(fl[r:] + fl[:r], "normal", rle=True)
            else:
                pool[key] = L.Code(base(g, k, needs[k], alphabet).lengths, "normal", rle=True, counted=True)   # (a short description: the arena grows with the file)
        return pool[key]
    return make


def many_groups(seed, ngroups, cache_bits, flat):
    """256 x 128 pixels in 2048 tiles of 4 x 4 that walk through ngroups groups; -> (file, groups built without tables, fits the arena) by arena_model"""
    rng = np.random.default_rng(seed)
    w, h = 256, 128
    gmap = (np.arange(2048) % ngroups).reshape(32, 64)
    events = L.random_events(rng, w, h, cache_bits=cache_bits, p_copy=0.5, p_cache=0.1, lengths=[1, 2, 3, 5, 8, 13, 21], dcodes=[1, 2, 3, 4, 9, 121, 130, 120 + 5 * w],
                             values=None if flat else argb(rng, 12) & np.uint64(0x0F0F0F0F))   # (many copies: a short file -- the arena grows with the file)
    needs = [set() for _ in range(5)]
    for ev in events:
        for k, s in L.event_symbols(ev):
            needs[k].add(s)
    for k in range(5):   # symbols in a few clusters: short descriptions
        needs[k] |= set(range(17 if k < 4 else 8)) | ({256, 257, 258, 259, 260, 280, 281} if k == 0 else set())
    info = {}
    stream = L.write_stream(w, h, events, pooled_maker(rng, 11, needs, flat=flat), cache_bits=cache_bits, meta=(2, gmap), sub_make=L.default_code_maker(rng), info=info)
    without, fits = arena_model(len(stream), [[len(c.codes) for c in g] for g in info["groups"]])
    return L.vp8l_file(stream), without, fits


# group counts for 256 x 128 pixels, each held to what it is meant to reach by arena_model on the stream actually written
PAST_TABLES_GROUPS = 1900      # small codes (about 17 symbols each, lengths up to 15): the tables stop near 1500 groups, and all of them still fit
PAST_TABLES_FULL_GROUPS = 750  # full alphabets (2328 + 3 x 256 + 40 symbols with an 11-bit cache): the tables stop near 560 groups
PAST_ARENA_GROUPS = 1100       # full alphabets: about 850 groups fit


@functools.lru_cache(None)
def vp8l_past_tables_case():
    out = []
    for n, cache_bits, flat in ((PAST_TABLES_GROUPS, 2, False), (PAST_TABLES_FULL_GROUPS, 11, True)):
        blob, without, fits = many_groups(77, n, cache_bits, flat)
        assert fits and without >= 100, (n, without, fits)   # the last hundreds of groups are read length by length
        out.append(("groups %d, %d of them without tables" % (n, without), blob))
    return out


@functools.lru_cache(None)
def vp8l_past_arena_case():
    blob, without, fits = many_groups(78, PAST_ARENA_GROUPS, 11, flat=True)
    assert not fits, (without, fits)
    return [("groups %d beyond the arena" % PAST_ARENA_GROUPS, blob)]


@functools.lru_cache(None)
def vp8l_bits_cases():
    """meta-prefix tile bits 2 .. 9 (tiles larger than the picture among them) crossed with colour-cache bits 1 .. 11"""
    out = []
    for cb in range(1, 12):
        for prec in ((cb % 8) + 2, ((cb + 3) % 8) + 2):
            w, h = [(70, 41), (256, 37), (131, 128), (19, 90)][(cb + prec) % 4]
            shape = sub_shape(w, h, prec)
            gmap = np.random.default_rng(cb * 16 + prec).integers(0, 5, shape)
            gmap.flat[0] = 4
            out.append(("cache bits %d tile bits %d %dx%d" % (cb, prec, w, h), lossless(9500 + len(out), w, h, cache_bits=cb, meta=(prec, gmap), ev_kw={"p_cache": 0.3})))
    return out


def form_maker(rng, form, maxlen=15):
    """every code of the picture in one form of description, where the code's symbols allow it (else a normal code from a random tree)"""
    base = L.default_code_maker(rng, maxlen=maxlen, forms=False, extra=(0, 0) if form.startswith(("simple", "twice", "single")) else (3, 30))

    def make(g, k, need, alphabet):
        syms = sorted(need) or [int(rng.integers(0, 2))]
        lengths = [0] * alphabet
        if form in ("simple1", "simple1_8", "twice", "single_normal", "single_counted") and len(syms) == 1 and syms[0] < 256:
            lengths[syms[0]] = 1 if form.startswith(("simple", "twice")) else int(rng.integers(1, 15))
            if form == "single_normal":
                return L.Code(lengths, "normal", rle=bool(g & 1))
            if form == "single_counted":
                return L.Code(lengths, "normal", rle=bool(g & 1), counted=syms[0] >= 1)
            return L.Code(lengths, "simple", first_1bit=False if form == "simple1_8" else None, twice=form == "twice")
        if form in ("simple2", "simple2_8", "simple2_swap") and len(syms) <= 2 and max(syms) < 256:
            while len(syms) < 2:
                syms = sorted(set(syms) | {int(rng.integers(0, min(alphabet, 256)))})
            lengths[syms[0]] = lengths[syms[1]] = 1
            return L.Code(lengths, "simple", first_1bit=False if form == "simple2_8" else None, swap=form == "simple2_swap" and syms[1] >= 2)
        if form in ("full", "full_reversed", "full_plain", "full_counted"):
            # every symbol of the alphabet.  Shorter lengths first: for 256 symbols all are 8 -- repeat code 16 BEFORE any length was sent (it repeats 8) -- and the
            # last repeat ends exactly at the alphabet's end; reversed: the longer lengths first, the run of the shorter ones ends the alphabet
            fl = L.flat_lengths(alphabet)
            return L.Code(fl[::-1] if form == "full_reversed" else fl, "normal", rle=form != "full_plain", counted=form == "full_counted")
        c = base(g, k, syms, alphabet)
        if form == "zero_runs":      # runs of zeros through 17 / 18 up to the alphabet's very end (no max_symbol)
            return L.Code(c.lengths, "normal", rle=True, counted=False)
        if form == "counted":
            return L.Code(c.lengths, "normal", rle=bool(g & 1), counted=True)
        if form == "plain":
            return L.Code(c.lengths, "normal", rle=False, counted=False)
        return c
    return make


@functools.lru_cache(None)
def vp8l_code_cases():
    """codes of maximum length 15, with all symbols <= 8 bits, with a mix straddling 8 (the 256-entry table and the walk behind it); every form of description:
    simple with a 1-bit and an 8-bit symbol, two symbols in both orders, two EQUAL symbols, a normal code with a single used symbol (any length), normal codes
    with and without max_symbol, with and without repeat codes, repeat code 16 in front of any non-zero length, runs that end exactly at the alphabet's end"""
    out = []
    few = {"values": [0xFF000000, 0xFF000100, 0xFF010001, 0x01000000, 0xFF800000]}
    for maxlen in (15, 8, 11, 9, 1):
        for j in range(3):
            rng = np.random.default_rng(9700 + len(out))
            mk = L.default_code_maker(rng, maxlen=max(maxlen, 2), extra=(20, 200) if maxlen > 1 else (0, 0), forms=maxlen == 1)
            vals = {"values": argb(rng, 300)} if maxlen > 1 else few
            out.append(("codes maxlen %d #%d" % (maxlen, j), lossless(9700 + len(out), 61, 33, cache_bits=[0, 4, 10][j], make=mk, ev_kw=vals)))
    for form in ("simple1", "simple1_8", "twice", "single_normal", "single_counted", "simple2", "simple2_8", "simple2_swap", "full", "full_reversed", "full_plain", "full_counted",
                 "zero_runs", "counted", "plain"):
        for j, vals in enumerate([{"values": [0xFF000000]}, {"values": [0x01010101, 0x01010101]}, few, {"values": [0xFF000000, 0xFF00FF00], "p_copy": 0.0}, {}]):
            rng = np.random.default_rng(9800 + len(out))
            cb = [0, 0, 3, 0, 11][j]
            gm = np.arange(16 * 9).reshape(9, 16) % 3 if j == 2 else None
            out.append(("codes %s #%d" % (form, j), lossless(9800 + len(out), 61, 33, cache_bits=cb, make=form_maker(rng, form), ev_kw=vals, meta=(2, gm) if gm is not None else None)))
    return out


def transform_of(rng, kind, w, h, bits=None, ncolors=None):
    if kind == "green":
        return ("green",)
    if kind == "palette":
        return ("palette", argb(rng, ncolors or int(rng.choice([2, 3, 5, 17]))))
    bits = bits or int(rng.integers(2, 5))
    return (kind, bits, argb(rng, sub_shape(w, h, bits)))


def with_transforms(seed, w, h, kinds, **kw):
    """a picture with the named transforms in that stream order (each sub-image at the width the stream has at that point)"""
    rng = np.random.default_rng(seed)
    tr, xs = [], w
    for kind in kinds:
        k, arg = (kind, {}) if isinstance(kind, str) else kind
        t = transform_of(rng, k, xs, h, **arg)
        tr.append(t)
        xs = L.packed_width(xs, [t])
    return lossless(seed + 1, w, h, transforms=tr, ev_kw={"values": argb(rng, 400), "p_copy": 0.1}, **kw)


@functools.lru_cache(None)
def vp8l_transform_order_cases():
    """every subset of the four transforms in every order, each at most once: 65 pictures; colour indexing read AFTER the predictor among them (the inverse
    then runs on the other one of the decoder's two frames)"""
    out = []
    kinds = ("predictor", "cross", "green", "palette")
    for n in range(5):
        for order in itertools.permutations(kinds, n):
            w, h = [(13, 9), (37, 20)][len(out) % 2]
            out.append(("transforms %s" % "+".join(order), with_transforms(10000 + 2 * len(out), w, h, order)))
    return out


@functools.lru_cache(None)
def vp8l_palette_cases():
    """palettes of 1, 2, 3, 4, 5, 16, 17 and 256 colours (8 / 4 / 2 / 1 pixels per sample), the indices random bytes: most lie beyond a small palette; alone, in
    front of and behind a predictor, widths that do not fill the last packed sample"""
    out = []
    for n in (1, 2, 3, 4, 5, 16, 17, 256):
        for j, kinds in enumerate([[("palette", {"ncolors": n})], [("palette", {"ncolors": n}), "predictor"], ["predictor", ("palette", {"ncolors": n})],
                                   ["green", ("palette", {"ncolors": n}), "cross"]]):
            w, h = [(1, 1), (7, 5), (9, 14), (33, 12), (64, 3)][(n + j) % 5]
            out.append(("palette %d colours, order %d, %dx%d" % (n, j, w, h), with_transforms(10500 + 2 * len(out), w, h, kinds)))
    return out


@functools.lru_cache(None)
def vp8l_tile_bits_cases():
    """predictor and cross-colour tile bits 2 .. 9, tiles larger than the picture among them"""
    out = []
    for bits in range(2, 10):
        for w, h in ((70, 41), (200, 70), (3, 140)):
            out.append(("tile bits %d %dx%d" % (bits, w, h), with_transforms(11000 + 2 * len(out), w, h, [("predictor", {"bits": bits}), ("cross", {"bits": 2 + (bits + 3) % 8})])))
    return out


@functools.lru_cache(None)
def vp8l_predictor_cases():
    """every predictor mode 0 .. 13 (and 14, 15, which libwebp reads as mode 0) in tiles that touch row 0, column 0 and the last column; widths 1, 2, 7, 8, 9 and
    100: under, at and over the wave front's chunk of 8, and several chunks in flight; the other bits of the mode image are noise"""
    out = []
    for w in (1, 2, 7, 8, 9, 100):
        for k in range(16):
            rng = np.random.default_rng(11500 + len(out))
            h = [11, 5, 14, 9][k % 4]
            ty, tx = np.indices(sub_shape(w, h, 2))
            modes = (k + 5 * ty + tx) % 16
            data = (argb(rng, modes.shape) & ~np.uint64(0xF00)) | (modes.astype(np.uint64) << np.uint64(8))
            ev = L.literals(argb(rng, (h, w))) if k % 2 else None
            out.append(("predictor width %d modes from %d" % (w, k), lossless(11500 + len(out), w, h, transforms=[("predictor", 2, data)], events=ev,
                                                                              ev_kw={"values": argb(rng, 50)})))
    return out


def copy_events(rng, xs, ys, cache_bits, far):
    """literals until a copy fits, then copies at distance codes 1 .. 120 in turn and some beyond, lengths 1 .. 4096 in turn, a literal or a cache index in between"""
    total, pos, out = xs * ys, 0, []
    codes = list(range(1, 121)) + far
    lengths = itertools.cycle([1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33, 64, 100, 257, 1000, 4096, 2, 11])
    vals = argb(rng, 40)
    done = 0
    while pos < total:
        dc = codes[done % len(codes)]
        if done == len(codes) and pos >= 4200 and total - pos >= 2 * 4096:   # a large picture: the longest copy from further back than its length, once
            out.append(("copy", 4096, 120 + 4200)); pos += 4096
            done += 1
        elif L.plane_distance(dc, xs) <= pos:
            ln = min(next(lengths), total - pos)
            if done < len(codes):   # the first round through the codes has to fit into the picture
                ln = max(1, min(ln, (total - pos) // (2 * (len(codes) - done))))
            out.append(("copy", ln, dc)); pos += ln
            done += 1
            if pos < total and rng.random() < 0.5:
                out.append(("cache", int(rng.integers(0, 1 << cache_bits))) if cache_bits and rng.random() < 0.5 else ("lit", int(rng.choice(vals)))); pos += 1
        else:
            out.append(("lit", int(rng.choice(vals)))); pos += 1
    return out


@functools.lru_cache(None)
def vp8l_copy_cases():
    """copies of length 1 .. 4096 at every one of the 120 neighbourhood codes -- in narrow pictures many of them map to a distance below 1, which reads as 1 --
    and at a few long distances, across rows and tiles (the group is picked again behind each), overlapping (distance < length) and not, cache references between them"""
    out, seen = [], set()
    for w, h in ((5, 200), (3, 300), (17, 90), (64, 64), (256, 128), (9, 120), (1, 700)):
        for cb in (0, 5):
            rng = np.random.default_rng(12000 + len(out))
            ev = copy_events(rng, w, h, cb, [121, 122, 120 + w, 120 + 2 * w + 1, 120 + 8 * w + 3, 120 + 20 * w])
            assert {e[2] for e in ev if e[0] == "copy"} >= set(range(1, 121)), (w, h)
            seen |= {(e[1], e[1] > L.plane_distance(e[2], w)) for e in ev if e[0] == "copy"}
            prec = 2 + len(out) % 3
            gmap = np.random.default_rng(len(out)).integers(0, 12, sub_shape(w, h, prec))
            gmap.flat[0] = 11
            out.append(("copies %dx%d cache %d" % (w, h, cb), lossless(12000 + len(out), w, h, cache_bits=cb, events=ev, meta=(prec, gmap))))
    assert {(1, False), (4096, True), (4096, False), (2, True), (257, False)} <= seen   # (length, overlapping)
    return out


@functools.lru_cache(None)
def alph_cases():
    """the ALPH chunk of a lossy file: its four filters x the raw and the compressed method x two sizes (one of width 1); the compressed plane also behind a
    predictor and behind a palette (libwebp has an 8-bit path of its own for the latter)"""
    out = []
    for w, h in ((1, 37), (45, 23)):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(70 + w, w, h, texture=10.0), "RGB").save(b, format="WEBP", quality=70)
        lossy = b.getvalue()
        for filt in range(4):
            rng = np.random.default_rng(13000 + len(out))
            out.append(("alph %dx%d filter %d raw" % (w, h, filt), L.alph_file(w, h, lossy, filt, 0, rng.integers(0, 256, w * h, dtype=np.uint8).tobytes())))
            for j, kinds in enumerate([[], ["predictor"], [("palette", {"ncolors": 6})]]):
                tr, xs = [], w
                for kind in kinds:
                    k, arg = (kind, {}) if isinstance(kind, str) else kind
                    tr.append(transform_of(rng, k, xs, h, **arg))
                    xs = L.packed_width(xs, tr[-1:])
                vals = (rng.integers(0, 256, 30).astype(np.uint64) << np.uint64(8)) | (np.uint64(0xFF000000) if j == 2 else argb(rng, 30) & np.uint64(0xFFFF00FF))
                ev = L.random_events(rng, xs, h, cache_bits=0 if j == 2 else 3, values=vals)
                stream = L.write_stream(w, h, ev, L.default_code_maker(rng), transforms=tr, cache_bits=0 if j == 2 else 3, headerless=True, sub_make=L.default_code_maker(rng))
                out.append(("alph %dx%d filter %d compressed %s" % (w, h, filt, kinds), L.alph_file(w, h, lossy, filt, 1, stream)))
    return out


def test_emul_vp8l_colliding_groups(api):
    check(api, vp8l_group_cases())


def test_emul_vp8l_groups_past_the_table_threshold(api):
    check(api, vp8l_past_tables_case())


def test_emul_vp8l_groups_past_the_arena(api):
    """the one file a decoder may refuse: more groups than its arena holds.  Refused with the unsupported-feature error or decoded like libwebp -- never other
    pixels -- and its neighbours in the batch untouched"""
    (name, blob), = vp8l_past_arena_case()
    side = vp8l_bits_cases()[:2]
    want = judge(name, blob)
    outs = api.webp_decode([side[0][1], blob, side[1][1]])
    assert same_picture(outs[0], judge(*side[0])) and same_picture(outs[2], judge(*side[1]))
    assert (isinstance(outs[1], Exception) and outs[1].code == 10201) or same_picture(outs[1], want), outs[1]


def test_emul_vp8l_cache_bits_and_meta_tile_bits(api):
    check(api, vp8l_bits_cases())


def test_emul_vp8l_code_depths_and_description_forms(api):
    check(api, vp8l_code_cases())


def test_emul_vp8l_transforms_in_every_order(api):
    check(api, vp8l_transform_order_cases())


def test_emul_vp8l_palette_sizes(api):
    check(api, vp8l_palette_cases())


def test_emul_vp8l_transform_tile_bits(api):
    check(api, vp8l_tile_bits_cases())


def test_emul_vp8l_predictor_modes_at_the_edges(api):
    check(api, vp8l_predictor_cases())


def test_emul_vp8l_copies_at_every_distance_code(api):
    check(api, vp8l_copy_cases())


def test_emul_alph_filters_and_methods(api):
    cases = alph_cases()
    check(api, cases)
    assert any(judge(n, b)[:, :, 3].min() < 255 for n, b in cases)


def test_vp8l_writer_describes_codes_as_asked():
    """the description forms the cases above rely on are really in the streams: tests/_vp8l_parse.py (an independent reader) sees the repeat code 16 as the very
    first code-length symbol, the max_symbol field, and codes with a single symbol"""
    from _vp8l_parse import parse
    rng = np.random.default_rng(3)
    blob = lossless(1, 20, 10, make=form_maker(rng, "full"), ev_kw={"p_copy": 0.0})
    info = parse(blob)
    red = [c for where, g, which, c in info.codes if where == "argb" and which == 1][0]
    assert red.lengths == [8] * 256 and red.cl_lengths is not None and red.cl_count[16] == 43 and sum(red.cl_count) == 43 and not red.cl_counted
    blob = lossless(2, 20, 10, make=form_maker(rng, "counted"), ev_kw={"p_copy": 0.0})
    assert all(c.cl_counted for where, g, which, c in parse(blob).codes if where == "argb" and c.cl_lengths is not None)
    blob = lossless(3, 20, 10, make=form_maker(rng, "twice"), ev_kw={"values": [0xFF000000], "p_copy": 0.0})
    assert all(c.single is not None for where, g, which, c in parse(blob).codes if where == "argb")
