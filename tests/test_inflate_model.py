"""The inflate catalogue (tests/_inflate_cases.py) on the CPU, against referees that share no code with the oracle: zlib (and the
system's libdeflate where there is one) for the streams, Pillow and the numpy unfilter model for the pixels.  Then the oracle's decode
against the model, and its refusals."""
import ctypes as C
import ctypes.util
import io
import zlib

import numpy as np
import pytest

import _deflate as D
import _inflate_cases as IC
from oracle import oracle as O

PIL = pytest.importorskip("PIL.Image")


def zlib_output(z):
    """what zlib makes of a stream fed a byte at a time, up to its first error or its end: (bytes, error or None, end of stream seen)"""
    d = zlib.decompressobj()
    out = bytearray()
    for i in range(len(z)):
        try:
            out += d.decompress(z[i:i + 1])
        except zlib.error as e:
            return bytes(out), e, False
        if d.eof:
            break
    return bytes(out), None, d.eof


def libdeflate():
    name = ctypes.util.find_library("deflate")
    if not name:
        return None
    L = C.CDLL(name)
    L.libdeflate_alloc_decompressor.restype = C.c_void_p
    L.libdeflate_zlib_decompress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.libdeflate_free_decompressor.argtypes = [C.c_void_p]
    return L


def libdeflate_rc(L, z, cap):
    dec = L.libdeflate_alloc_decompressor()
    try:
        buf = C.create_string_buffer(cap + 1024)
        n = C.c_size_t()
        return L.libdeflate_zlib_decompress(dec, z, len(z), buf, cap + 1024, C.byref(n))
    finally:
        L.libdeflate_free_decompressor(dec)


@pytest.fixture(scope="module")
def valid():
    return IC.cached_valid()


@pytest.fixture(scope="module")
def invalid():
    return IC.cached_invalid()


def model_rows(c):
    return D.unfilter(c.raw, c.width, c.height, c.ctype, c.depth)


def test_writer_round_trips_through_zlib(valid):
    for c in valid:
        out, err, eof = zlib_output(c.z)
        assert err is None or not c.complete, (c.name, err)
        assert out == c.data[:len(out)] and len(out) >= len(c.raw), c.name   # the writer meant what zlib reads, to the image's last byte at least
        if c.complete:
            assert eof and zlib.decompress(c.z) == c.data, c.name
    L = libdeflate()
    if L is not None:   # the complete streams are valid for libdeflate too (0: LIBDEFLATE_SUCCESS)
        for c in valid:
            if c.complete and not c.name.startswith("tail_after"):
                assert libdeflate_rc(L, c.z, len(c.data)) == 0, c.name


def test_canonical_codes_follow_the_rfc():
    # RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111
    assert D.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]
    fixed = D.canonical(D.FIXED_LIT)
    assert fixed[0] == 0b00110000 and fixed[143] == 0b10111111 and fixed[144] == 0b110010000 and fixed[256] == 0 and fixed[280] == 0b11000000


def test_model_equals_pillow_on_every_valid_case(valid):
    for c in valid:
        im = PIL.open(io.BytesIO(c.png))
        im.load()
        want = D.pillow_view(model_rows(c), c.width, c.height, c.ctype, c.depth)
        got = np.asarray(im)
        assert got.shape == want.shape and np.array_equal(got, want), c.name


def test_oracle_rows_equal_the_model(valid):
    for c in valid:
        P = O.png_decode(c.png)
        assert np.array_equal(P.rows(), model_rows(c)), c.name
        if c.irreducible:
            assert P.reduce() == 0, c.name


# where libdeflate is more lenient than zlib on purpose: it takes up to 288 / 32 code lengths and lets the last repeat run past them
# (into slack it fills with zeros), and it decodes both halves of a single length-1 code as that codeword's symbol, so whatever it says
# about the *_bit1 streams comes from further on (their trailer is what the writer meant, not what such a decode gives).  zlib refuses
# all of these where the damage is, and so do the oracle and the device
LIBDEFLATE_LENIENT = {"hlit_287", "hlit_288", "hdist_31", "hdist_32", "repeat_past_end", "single_litlen_len1_bit1", "single_dist_len1_bit1"}


def test_invalid_streams_have_the_defect_they_are_named_for(invalid):
    """the code lengths the damaged block holds (block 1: every invalid stream starts with a good fixed block) are what the name says"""
    where = {"litlen": "lit", "dist": "dist", "codelen": "cl"}
    for c in invalid:
        kind, _, alphabet = c.name.partition("_")
        if kind not in ("oversub", "incomplete", "single"):
            continue
        alphabet = alphabet.split("_")[0]
        lens = [l for l in c.d.blocks[1][where[alphabet]] if l]
        if kind == "oversub":
            assert D.kraft(lens) > 1 << 15, c.name
        elif kind == "incomplete":
            assert D.kraft(lens) < 1 << 15 and len(lens) > 1, c.name
        else:
            n = int(c.name.split("_")[2][3:])
            assert lens == [n], c.name


def test_invalid_streams_are_refused_before_the_last_byte(invalid):
    L = libdeflate()
    for c in invalid:
        out, err, eof = zlib_output(c.z)
        assert len(out) < len(c.raw), (c.name, len(out), len(c.raw), err)
        if c.expect is None:   # truncated: no error, the stream runs out
            assert err is None and not eof, (c.name, err)
        else:
            assert err is not None and c.expect in str(err), (c.name, err)
        if L is not None and c.name not in LIBDEFLATE_LENIENT:
            assert libdeflate_rc(L, c.z, len(c.data)) != 0, c.name
        with pytest.raises(O.PngError):
            O.png_decode(c.png)
        with pytest.raises(OSError):   # libpng (Pillow) refuses them too
            PIL.open(io.BytesIO(c.png)).load()


def test_worst_convergence_stream_keeps_every_guess_off_the_true_walk(valid):
    """the case's point, checked so it cannot quietly go: the 255 codeword is 1^11, and for 64 and for CSP_HUFF_WAVES * 64 lanes no lane's
    first guess (the walk from CSP_HUFF_PRE bits in front of its stretch) lands on a true token boundary, in every round of the block"""
    g = IC.geometry()
    c = next(c for c in valid if c.name == "worst_convergence")
    blk = c.d.blocks[0]
    lit = blk["lit"]
    assert lit[255] == 11 and D.canonical(lit)[255] == (1 << 11) - 1 and D.kraft(lit) == 1 << 15
    starts = [t[0] for t in c.d.toks]
    run0, eob = starts[1], blk["eob"]
    assert all(t[1] == 11 for t in c.d.toks[1:]) and eob - run0 == 11 * 30000
    bits = np.unpackbits(np.frombuffer(c.d.getvalue(), np.uint8), bitorder="little")
    assert bits[run0:eob].all()
    true = set(starts) | {eob}
    for lanes in sorted({64, g["lanes"]}):
        base, rounds = blk["start"], 0
        while base < eob:
            wrong = 0
            for lane in range(1, lanes):
                s0 = base + g["sub"] * lane
                if s0 >= eob:
                    break
                q = s0 - g["pre"]
                while q < s0:
                    q += 11   # every walk inside the run reads 11 ones at a time
                assert q not in true, (lanes, rounds, lane)
                wrong += 1
            assert rounds or wrong == lanes - 1
            rounds += 1
            nxt = base + lanes * g["sub"]
            base = min((t for t in true if t >= nxt), default=eob + 1)
        assert rounds >= 3, (lanes, rounds)


def test_catalogue_reaches_every_item(valid, invalid):
    hit = set()
    for c in valid:
        hit |= IC.facts(c)
    missing = [k for k in IC.VALID_ITEMS if k not in hit]
    assert not missing, missing
    hit = set()
    for c in invalid:
        hit |= c.items
    missing = [k for k in IC.INVALID_ITEMS if k not in hit]
    assert not missing, missing
    print("catalogue: %d valid cases (%d items), %d invalid (%d items)" % (len(valid), len(IC.VALID_ITEMS), len(invalid), len(IC.INVALID_ITEMS)))
