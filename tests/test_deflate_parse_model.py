"""The LZ parse of the PNG row's DEFLATE coder -- the greedy tokenizer (png_lz.h) and the min-cost-path parse (png_parse.h) -- is this project's own design, and
oracle/png_oracle.c (tokenize, deep_parse, deflate_chunk) its only statement: the same authors' restatement of the same algorithm.  tests/_deflate_parse_model.py
states it a third time, from the prose, stage by stage; this file proves the model and the statement on a battery of streams a filtered PNG never produces:

  * the oracle's streams, read back token by token (tests/_deflate_read.py), are the model's, at 0, 5 and 15 passes;
  * what follows from the definition of a match alone -- true copies, distances inside the stream and the window, maximal lengths, nothing across a chunk's or a
    segment's end -- holds for every candidate and token, checked on the bytes and not through the model's own functions;
  * every pass's path is the cheapest among its own edges, by a search organised the other way round (relaxation forwards, and pushed backwards along incoming
    edges, over an explicit edge list), ties broken towards the literal and the shorter length;
  * the battery reaches what it is for (counted by the model, never by the code under test).

No GPU.  tests/test_deflate_parse_units_emul.py and tests/test_zzz_deflate_parse_units_gpu.py put both builds of the kernels' functions through the same battery."""
import collections
import functools
import zlib

import numpy as np
import pytest

import _deflate_parse_model as M
import _deflate_read as R
from oracle import oracle as O

ITERS = (0, 5, 15)


@functools.lru_cache(None)
def battery():
    """[(name, stream)], seeded; each the smallest shape that reaches its edge"""
    rng = np.random.default_rng(20261020)
    noise = lambda n, k=256, base=0: bytes((rng.integers(0, k, n) + base).astype(np.uint8))
    out = []
    for n in (1, 3, 4, 7, 8, 9):   # no 4- or 8-byte key, less than a match left
        out.append((f"same_{n}", b"\x5a" * n))
        out.append((f"distinct_{n}", bytes(range(17, 17 + n))))
    for n in (300, 511, 512, 513, 32768, 32769):   # one key per tile, the 258 cap, segment cuts, the kept-greedy rule
        out.append((f"run_{n}", b"\x07" * n))
    for k in (2, 3, 5, 7):   # the fixed distances where fewer than 8 bytes lie in front
        out.append((f"period_{k}", bytes(range(200, 200 + k)) * (40 // k + 1)))
    out.append(("noise4_3000", noise(3000, 4)))
    out.append(("white_600", noise(600)))
    block, fill = noise(700, 128, 128), noise(32768, 2)   # a filler of few keys leaves the block's in the tables
    out.append(("seam_32768", block + fill[700:] + block + block[:300]))
    # (and three bytes far back: two words of one 4-byte key agree in three bytes only where the chunk ends after the third -- here at 32765, from 20000)
    mark = bytearray(block + fill[700:] + b"\x01" + block + block[:300])
    mark[20000:20004], mark[32765:32768] = b"\xc9\xca\xcb\x01", b"\xc9\xca\xcb"
    out.append(("seam_32769", bytes(mark)))
    late = noise(40, 128, 128)
    out.append(("starts_at_32767", fill[:32767] + late + fill[:500] + late + fill[:100]))
    out.append(("period37_then_noise", noise(37) * 400 + noise(5000)))
    text = noise(20000, 3, 97)
    words = lambda n: b"".join(text[o:o + 40] for o in rng.integers(0, 20000 - 40, -(-n // 40)))[:n]
    out.append(("words_36000", words(36000)))
    three = noise(32768 + 9, 3)
    for k in range(1, 10):   # a last chunk shorter than a tile and than a key
        out.append((f"noise3_32768+{k}", three[:32768 + k]))
    out.append(("words_513", words(513)))   # a last segment of one byte
    out.append(("words_32257", words(32768 - 511)))   # the last lane's segment holds one byte
    key = noise(12, 128, 128)
    out.append(("ten_copies", b"".join(key + noise(288, 128) for _ in range(10))))   # the 4-way and the 8-way row of one key fill up and push out
    assert len({n for n, _ in out}) == len(out)
    return out


NAMES = [n for n, _ in battery()]
stream = dict(battery()).__getitem__


def replay(tokens, front):
    out = bytearray(front)
    for n, x in tokens:
        if n:
            assert 1 <= x <= len(out), "a distance in front of the stream"
            for _ in range(n): out.append(out[-x])
        else:
            out.append(x)
    return bytes(out[len(front):])


# ---------------------------------------------------------------------------------------------------- the model against the oracle, and the stream's structure
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("name", NAMES)
def test_the_oracles_tokens_are_the_models(name, iters):
    data = stream(name)
    z = O.deflate_zlib(data, iters)
    assert zlib.decompress(z) == data
    blocks, back = R.read(z[2:-4])
    assert back == data
    chunks = M.chunks_of(len(data))
    # ceil(n / 32768) dynamic blocks, each but the last followed by one empty stored block
    assert [b.btype for b in blocks] == ([2, 0] * len(chunks))[:-1] and [b.final for b in blocks] == [0] * (len(blocks) - 1) + [1]
    for b, (s, e) in zip(blocks[::2], chunks):
        assert replay(b.tokens, data[:s]) == data[s:e], f"{name}: the block of chunk {s} does not produce exactly the chunk (a match across its end?)"
        want = M.chunk_tokens(data, s, e, iters)
        if b.tokens != want:
            k = next((i for i, (x, y) in enumerate(zip(b.tokens, want)) if x != y), min(len(want), len(b.tokens)))
            raise AssertionError(f"{name}, {iters} passes, chunk {s} ({M.chunk_kind(data, s, e, iters)}): token {k} is {b.tokens[k:k + 3]}, the model says {want[k:k + 3]}")


# ---------------------------------------------------------------------------------------------------- from the definition of a match
def check_copy(data, p, n, d, what):
    assert 3 <= n <= 258 and 1 <= d <= min(p, 32768), f"{what} at {p}: ({n}, {d})"
    for k in range(n):
        assert data[p + k] == data[p + k - d], f"{what} at {p}: ({n}, {d}) is no copy at byte {k}"


def maximal(data, p, n, d, limit):
    return n == min(258, limit - p) or (n < min(258, limit - p) and data[p + n] != data[p + n - d])


@pytest.mark.parametrize("name", NAMES)
def test_candidates_and_tokens_are_true_maximal_copies(name):
    data = stream(name)
    for s, e in M.chunks_of(len(data)):
        for off, (n0, d0, n1, d1) in enumerate(M.candidates(data, s, e)):
            p = s + off
            if n0:
                check_copy(data, p, n0, d0, "c0")
                assert maximal(data, p, n0, d0, e)
            if n1:
                assert n1 > n0 and d1 != d0
                if n0:
                    check_copy(data, p, n1, d1, "c1")
                    assert d1 > d0   # the nearest is c0
                else:   # nothing reaches 3 bytes: the longest offer stands alone and no path uses it
                    assert n1 < 3 and 1 <= d1 <= min(p, 32768) and data[p:p + n1] == data[p - d1:p - d1 + n1]
                assert maximal(data, p, n1, d1, e)
        p = s
        for n, d in M.greedy(data, s, e):
            if n:
                check_copy(data, p, n, d, "greedy token")
                assert maximal(data, p, n, d, e), f"greedy token ({n}, {d}) at {p} stops early"
            p += max(n, 1)
        assert p == e
        if M.chunk_kind(data, s, e, 1) == "greedy":
            continue
        for iters in (1, 5, 15):
            p = s
            for n, d in M.deep(data, s, e, iters):
                if n:
                    seg_end = min(e, s + ((p - s) // 512 + 1) * 512)
                    check_copy(data, p, n, d, "deep token")
                    assert p + n <= seg_end, f"deep token ({n}, {d}) at {p} crosses a multiple of 512 from the chunk's start"
                    assert n <= 16 or maximal(data, p, n, d, seg_end)
                p += max(n, 1)
            assert p == e


# ---------------------------------------------------------------------------------------------------- the path is the cheapest among its own edges
def edge_list(data, s, e, cand):
    """every edge of every segment: arrays (from, to, length, distance code or -1 for a literal, byte); a node is segment * 513 + place, so that a segment's end is
    not the next one's start.  At a position: the literal; c0 at 3..min(len0, 16) and at len0; c1 at len0 + 1..min(len1, 16) and at len1; lengths first cut to what
    is left of the segment"""
    rows = []
    for off in range(e - s):
        seg, i = divmod(off, 512)
        left = min(512, e - s - seg * 512) - i
        node = seg * 513 + i
        rows.append((node, node + 1, 1, -1, data[s + off]))
        n0, d0, n1, d1 = cand[off]
        n0, n1 = min(n0, left), min(n1, left)
        if n0 < 3:
            continue
        mine = {}
        for n in list(range(3, min(n0, 16) + 1)) + [n0]: mine[n] = d0
        if n1 > n0:
            for n in list(range(n0 + 1, min(n1, 16) + 1)) + [n1]: mine[n] = d1
        for n, d in mine.items():
            rows.append((node, node + n, n, M.dist_code(d), 0))
    return np.array(rows, np.int64).T


@pytest.mark.parametrize("name", NAMES)
def test_every_pass_takes_the_cheapest_path(name):
    data = stream(name)
    for s, e in M.chunks_of(len(data)):
        if M.chunk_kind(data, s, e, 1) == "greedy":
            continue
        cand = M.candidates(data, s, e)
        src, dst, length, dcode, byte = edge_list(data, s, e, cand)
        nseg = -(-(e - s) // 512)
        place_src, place_dst = src % 513, dst % 513
        by_src, by_dst = np.argsort(place_src, kind="stable"), np.argsort(-place_dst, kind="stable")
        cut_src = np.searchsorted(place_src[by_src], np.arange(514))
        cut_dst = np.searchsorted(-place_dst[by_dst], -np.arange(513, -1, -1))
        starts = np.arange(nseg) * 513
        ends = starts + np.minimum(512, (e - s) - 512 * np.arange(nseg))
        offs = np.arange(e - s)
        node_of = (offs // 512) * 513 + offs % 512
        edge = {(a, n): j for j, (a, n) in enumerate(zip(src.tolist(), length.tolist()))}
        for k, ps in enumerate(M.passes(data, s, e, 15)):
            lit_cost, len_cost, dist_cost = (np.array(c, np.int64) for c in ps["costs"])
            w = np.where(dcode < 0, lit_cost[byte], len_cost[length] + dist_cost[np.maximum(dcode, 0)])
            far = np.int64(1) << 40
            # forwards: the cheapest way from a segment's start to every node, relaxing the edges that leave place 0, 1, 2, ..
            reach = np.full(nseg * 513, far)
            reach[starts] = 0
            for i in range(512):
                g = by_src[cut_src[i]:cut_src[i + 1]]
                np.minimum.at(reach, dst[g], reach[src[g]] + w[g])
            # backwards: the cheapest way from every node to its segment's end, pushed along the edges that arrive at place 512, 511, ..
            togo = np.full(nseg * 513, far)
            togo[ends] = 0
            for j in range(513):
                g = by_dst[cut_dst[j]:cut_dst[j + 1]]
                np.minimum.at(togo, src[g], w[g] + togo[dst[g]])
            assert np.array_equal(reach[ends], togo[starts])
            assert int((w + togo[dst]).max()) < 1 << 23, "a cost that `<< 9` would push out of 32 bits"
            # the chosen path costs that much, and its first step at EVERY position is the least (cost, length): the literal, then the shorter
            choice = np.array(ps["choice"], np.int64)
            through = w + togo[dst]
            least = np.full(nseg * 513, far)
            np.minimum.at(least, src, through)
            assert np.array_equal(least[node_of], togo[node_of])
            tied = through == least[src]
            first = np.full(nseg * 513, 1 << 20, np.int64)
            np.minimum.at(first, src[tied], length[tied])
            assert np.array_equal(first[node_of], choice), f"{name}, chunk {s}, pass {k}: a first step that is not the literal-then-shorter among the cheapest"
            for seg in range(nseg):
                node, paid = int(starts[seg]), 0
                while node != ends[seg]:
                    n = int(choice[(node // 513) * 512 + node % 513])
                    paid += int(w[edge[(node, n)]])   # (a KeyError: the choice is no edge)
                    node += n
                assert paid == reach[ends[seg]], f"{name}, chunk {s}, pass {k}, segment {seg}: the path costs {paid}, the cheapest {reach[ends[seg]]}"


# ---------------------------------------------------------------------------------------------------- what the battery reaches
def test_the_battery_reaches_what_it_is_for():
    st, kinds, seen = collections.Counter(), collections.Counter(), collections.Counter()
    for name, data in battery():
        for s, e in M.chunks_of(len(data)):
            tokens = M.chunk_tokens(data, s, e, 5)
            kind = M.chunk_kind(data, s, e, 5)
            kinds[kind] += 1
            M.greedy(data, s, e, st)
            seen["distance_32768"] += sum(1 for n, d in tokens if n and d == 32768)
            seen["length_258"] += sum(1 for n, d in tokens if n == 258)
            if kind == "greedy":
                continue
            cand, off = M.candidates(data, s, e, st), 0
            for n, d in M.deep(data, s, e, 5):
                if n:
                    n0, d0, n1, d1 = cand[off]
                    left = min(512, e - s - off // 512 * 512) - off % 512
                    if n > 16 and d == d1 and n > min(n0, left): seen["long_from_c1"] += 1
                    if n <= 16 and n < min(n0 if d == d0 and n <= n0 else n1, left): seen["short_of_its_candidate"] += 1
                off += max(n, 1)
            seen["c1_at_32768"] += sum(1 for c in cand if 32768 in (c[1], c[3]))
    assert kinds["greedy"] and kinds["deep"] and kinds["kept"], kinds
    for what in ("distance_32768", "length_258", "long_from_c1", "short_of_its_candidate", "c1_at_32768"):
        assert seen[what], (what, seen)
    for what in ("lazy", "literals_cheaper", "three_bytes_too_far", "greedy_row_full", "row4_full", "row8_full", "tile_on_one_key", "fixed_match_at_p_below_8",
                 "match_in_last_seven", "candidate_in_last_seven", "walk_cut_by_distance"):
        assert st[what], (what, dict(st))
