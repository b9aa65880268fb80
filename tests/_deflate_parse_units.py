"""What tests/test_deflate_parse_units_emul.py and tests/test_zzz_deflate_parse_units_gpu.py share: the bodies that put one build of the unit library's
csdu_lz_chunk / csdu_deep_chunk (tests/devunit/du_png_parse.cpp: lz_chunk and deep_chunk on arbitrary bytes) and one build of the product through the battery of
tests/test_deflate_parse_model.py, against tests/_deflate_parse_model.py.  Every comparison is exact."""
import functools

import numpy as np

import _deflate_parse_model as M
import _deflate_read as R
from test_deflate_parse_model import battery

FRONT = BACK = 64
# png_parse.h: the layout of a workgroup's scratch area, and of a candidate word
CAND_OFF, CHOICE_OFF, TAKEN_OFF, SCRATCH = 0, 262144, 327680 + 131584, 524288
NSYM = 316
PASSES = (1, 5, 15)


def padded(data, complement):
    """the stream with 64 bytes in front and behind that invite a wrong answer: in front the stream's first bytes over and over, ending where the stream begins (a
    fixed-distance compare that forgot `d <= p` finds its match there), behind it the last bytes continued (a common-prefix count not cut to what is left runs
    on); complement: both the other way round"""
    head, tail = data[:8], data[-8:]
    front, back = (head * FRONT)[-FRONT:], (tail * BACK)[:BACK]
    if complement:
        front, back = bytes(b ^ 255 for b in front), bytes(b ^ 255 for b in back)
    assert len(front) == FRONT and len(back) == BACK and FRONT + len(data) + BACK <= 96 * 1024
    return np.frombuffer(front + data + back, np.uint8).copy()


def tokens_of(data, s, e, ln, dist, lit, taken, what):
    """the per-position record of a sink as a token list; the visited positions must be exactly those a walk over the tokens reaches"""
    assert np.array_equal(lit, np.frombuffer(data[s:e], np.uint8)), f"{what}: the literal of a position is not its byte"
    assert set(np.unique(taken).tolist()) <= {0, 1}
    out, off = [], 0
    while off < e - s:
        assert taken[off], f"{what}: position {s + off} is not visited"
        out.append((int(ln[off]), int(dist[off])) if ln[off] else (0, int(lit[off])))
        off += max(int(ln[off]), 1)
    assert off == e - s, f"{what}: the last token runs past the chunk's end"
    assert int(taken.sum()) == len(out), f"{what}: positions inside a match are marked visited"
    return out


def same_tokens(what, got, want):
    if got != want:
        k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        raise AssertionError(f"{what}: token {k} is {got[k:k + 3]}, the model says {want[k:k + 3]} ({len(got)} tokens, the model {len(want)})")


def run_lz(lib, buf, total, s, e):
    n = e - s
    ln, dist, lit, taken = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint8), np.empty(n, np.uint8)
    lib.run("csdu_lz_chunk", buf, ("z", FRONT), ("z", total), ("z", s), ("z", e), ln, dist, lit, taken)
    return ln, dist, lit, taken


def run_deep(lib, buf, total, s, e, iters, fill):
    n = e - s
    ln, dist, lit, taken = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint8), np.empty(n, np.uint8)
    scratch, hist = np.empty(SCRATCH, np.uint8), np.empty(NSYM, np.uint32)
    lib.run("csdu_deep_chunk", buf, ("z", FRONT), ("z", total), ("z", s), ("z", e), iters, fill, ln, dist, lit, taken, scratch, hist)
    per_position = lambda a: a.reshape(512, 64).T.reshape(-1)[:n]   # [place in the segment][segment] -> chunk order
    word = per_position(scratch[CAND_OFF:CAND_OFF + 262144].view(np.uint64))
    assert not (word >> np.uint64(58)).any()
    cand = [tuple(int(x) for x in c) for c in zip(word & np.uint64(511), (word >> np.uint64(9)) & np.uint64(0xFFFF), (word >> np.uint64(25)) & np.uint64(511), (word >> np.uint64(34)) & np.uint64(0xFFFF))]
    byte = ((word >> np.uint64(50)) & np.uint64(255)).astype(np.uint8)
    choice = per_position(scratch[CHOICE_OFF:CHOICE_OFF + 65536].view(np.uint16)).astype(np.int64).tolist()
    marks = scratch[TAKEN_OFF:TAKEN_OFF + n].copy()
    return (ln, dist, lit, taken), cand, byte, choice, marks, hist.astype(np.int64).tolist()


def check_entry(lib, name):
    """one stream of the battery, every chunk: lz_chunk == greedy; the candidates in the scratch area == candidates; and at 1, 5 and 15 passes the choices ==
    the model's last pass, S.hist == its counts, the sink's tokens == deep.  Twice, between paddings and over scratch contents that differ in every bit."""
    data = dict(battery())[name]
    total = len(data)
    bufs = [padded(data, False), padded(data, True)]
    for s, e in M.chunks_of(total):
        sinks = [run_lz(lib, buf, total, s, e) for buf in bufs]
        for a, b in zip(*sinks): assert np.array_equal(a, b), f"{name}, chunk {s}: lz_chunk depends on what lies around the stream"
        same_tokens(f"{name}, chunk {s}, lz_chunk", tokens_of(data, s, e, *sinks[0], f"{name}, chunk {s}, lz_chunk"), M.greedy(data, s, e))
        want_cand = M.candidates(data, s, e)
        for iters in PASSES:
            what = f"{name}, chunk {s}, deep_chunk at {iters} passes"
            runs = [run_deep(lib, buf, total, s, e, iters, fill) for buf, fill in zip(bufs, (0x00, 0xFF))]
            for a, b in zip(runs[0][0], runs[1][0]): assert np.array_equal(a, b), f"{what}: the tokens depend on the padding or on the scratch area's old contents"
            for a, b, part in zip(runs[0][1:], runs[1][1:], ("candidates", "candidate bytes", "choices", "visit marks", "S.hist")):
                assert np.array_equal(a, b), f"{what}: the {part} depend on the padding or on the scratch area's old contents"
            sink, cand, byte, choice, marks, hist = runs[0]
            assert np.array_equal(byte, np.frombuffer(data[s:e], np.uint8)), f"{what}: the candidate word's byte"
            if cand != want_cand:
                k = next(i for i, (x, y) in enumerate(zip(cand, want_cand)) if x != y)
                raise AssertionError(f"{what}: the candidates of position {s + k} are {cand[k]}, the model says {want_cand[k]}")
            last = M.passes(data, s, e, iters)[-1]
            if choice != last["choice"]:
                k = next(i for i, (x, y) in enumerate(zip(choice, last["choice"])) if x != y)
                raise AssertionError(f"{what}: the choice at position {s + k} is {choice[k]}, the model says {last['choice'][k]}")
            assert hist == last["counts"][0] + last["counts"][1], f"{what}: S.hist is not the last pass's counts"
            assert np.array_equal(marks, sink[3]), f"{what}: the visit marks and the sink's visited lanes"
            same_tokens(what, tokens_of(data, s, e, *sink, what), M.deep(data, s, e, iters))


def check_refusals(lib):
    """the entries take what the functions take: a chunk of at most 32768 bytes that starts at a multiple of 32768 inside the stream"""
    data = dict(battery())["words_36000"]
    buf, total = padded(data, False), len(data)
    n = 32768
    o32, o8, scratch, hist = np.empty(n + 8, np.uint32), np.empty(n + 8, np.uint8), np.empty(SCRATCH, np.uint8), np.empty(NSYM, np.uint32)
    for s, e in ((0, 32769), (64, 128), (65536, 65537), (0, total + 1), (32768, 32768)):
        assert lib.call("csdu_lz_chunk", buf, ("z", FRONT), ("z", total), ("z", s), ("z", e), o32, o32, o8, o8) == -1
        assert lib.call("csdu_deep_chunk", buf, ("z", FRONT), ("z", total), ("z", s), ("z", e), 5, 0, o32, o32, o8, o8, scratch, hist) == -1
    assert lib.call("csdu_lz_chunk", buf, ("z", 63), ("z", total), ("z", 0), ("z", 64), o32, o32, o8, o8) == -1
    assert lib.call("csdu_deep_chunk", buf, ("z", FRONT), ("z", total), ("z", 0), ("z", 64), 0, 0, o32, o32, o8, o8, scratch, hist) == -1


@functools.lru_cache(None)
def whole_files():
    """pictures through the product at -o3: an indexed one whose chunks take the parse, and one row of 40000 grey pixels from the "words" stream (two chunks, the
    second short)"""
    from _util import raw_png
    from test_png_emul import deep_parse_cases
    rng = np.random.default_rng(7)
    text = (rng.integers(0, 3, 20000) + 97).astype(np.uint8)
    row = np.concatenate([text[o:o + 40] for o in rng.integers(0, 20000 - 40, 1000)])
    return [("indexed_160x120", dict(deep_parse_cases())["indexed_160x120"]), ("words_grey_40000x1", raw_png(row.reshape(1, 40000, 1), 0))]


def check_whole_file(api, name):
    """what ships is the unit's parse: the hist pass, the codes pass and the emit pass of the product all used it, or the file would not read back as the model's tokens"""
    from _util import package
    png = dict(whole_files())[name]
    out = api.compress_in_memory(png, package().default_parameters(png_optimize=True, png_optimization_level=3))
    blocks, data = R.read_png(out)
    chunks = M.chunks_of(len(data))
    assert [b.btype for b in blocks] == ([2, 0] * len(chunks))[:-1]
    kinds = set()
    for b, (s, e) in zip(blocks[::2], chunks):
        kinds.add(M.chunk_kind(data, s, e, 5))
        same_tokens(f"{name}, chunk {s}", b.tokens, M.chunk_tokens(data, s, e, 5))
    assert "deep" in kinds, f"{name}: no chunk of the file takes the min-cost-path parse"
    return len(chunks)
