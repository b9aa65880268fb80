"""A model of the PNG row's DEFLATE parse -- which tokens a chunk becomes -- in Python integers, written from the prose statement of the coder: the comment
blocks above tokenize() and deep_parse() in oracle/png_oracle.c, DESIGN section 7, and the header comments of png_lz.h and png_parse.h.  It calls neither the
oracle nor either build of the kernels; the only thing it shares with anyone is the format tables of RFC 1951 (tests/_deflate_read.py).  One function per
stage, so that a disagreement names its stage:

    greedy(data, start, end)                 the tokens of the chunk data[start:end] under the greedy tokenizer
    candidates(data, start, end)             per position (len0, d0, len1, d1)
    costs(lit_len_counts, dist_counts, first_pass)   -> (lit_cost[256], len_cost[259], dist_cost[30]) in 1/16 bit
    path(data, start, end, cand, costs)      -> (choice per position, (lit_len_counts, dist_counts))
    deep(data, start, end, iters)            the tokens after `iters` passes;  passes(...) keeps every pass (its costs, choices and counts)
    estimate(tokens), chunk_tokens(data, start, end, iters), chunk_kind(...)

`data` is the whole stream (its length is the coder's `total`), `start` a multiple of 32768, a token (0, byte) or (length, distance).

The statement, as this file reads it.
  greedy: tiles of 64 positions from the chunk's start.  A table of 2^9 keys (a multiplicative hash of 4 bytes) x 4 positions, most recent first; of a tile's
  positions with one key only the last enters, after the tile; the 32 KiB in front of the chunk enter the same way first; a position whose 4 bytes do not lie
  inside the stream has no key; the position 32767 behind the chunk's start never enters.  A position's match: of the distances 1, 2, 3, 4, 6, 8 that do not
  reach in front of the stream the one that agrees longest within 8 bytes (ties: the nearer), extended if all 8 agree; then the key's positions, most recent
  first, until one is more than 32768 back, each replacing the best only if strictly longer.  Nothing under 3 bytes; 3 bytes only within distance 8; a match of 3..8
  bytes only if its literals would cost at least MATCH_BASE16 + 16 x the distance's extra bits (a literal: the piecewise-linear 16 log2(chunk bytes / count),
  16..240).  Matches end at the chunk's end.  The walk: a match yields to a strictly longer one at the next position of the same tile.
  candidates: the same with two tables of 2^11 keys (4 bytes x 4 positions, 8 bytes x 8 positions) and tiles of 256.  Offers: of the fixed distances f0, the
  nearest that agrees in >= 3 of 8 bytes (at that length), and f1, the greedy rule's; every table position within 32768.  c0 = the nearest offer of >= 3 bytes,
  c1 = the longest offer (ties: the nearer), dropped unless longer than c0.  (So where nothing reaches 3 bytes c1 may stand alone with 1 or 2: no path uses it.)
  An offer's length is the true common length at its distance, cut to the chunk's end and 258: two offers at one distance never differ, and whether an equal
  distance replaces c0 or c1 cannot show.
  costs / path / passes: see the functions.
"""
import bisect
import collections
import functools

import numpy as np

from _deflate_read import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA

CHUNK = WINDOW = 32768
FIXED = (1, 2, 3, 4, 6, 8)
MATCH_BASE16, MATCH_RULE_MAXLEN = 320, 8
SEG, CAP, DEEP_START, DEEP_DIV = 512, 16, 64, 512
M32 = (1 << 32) - 1

LEN_CODE = [None] * 3 + [bisect.bisect_right(LEN_BASE, n) - 1 for n in range(3, 259)]


def dist_code(d):
    return bisect.bisect_right(DIST_BASE, d) - 1


def ilog16(q):
    """16 log2(q / 256), piecewise linear: the exponent and the four bits under the leading one"""
    e = q.bit_length() - 1
    return 16 * (e - 8) + (((q << 4) >> e) & 15)


def cost16_of(count, total):
    return min(max(ilog16((total << 8) // count), 1), 240)


# ---------------------------------------------------------------------------------------------------- what the stages share
def _window(data, start, end):
    """what a chunk's parse can depend on, as a stream of its own: the 32 KiB in front of the chunk, the chunk, and up to 8 bytes behind it (whether the last
    positions have a 4- or 8-byte key).  -> (bytes, the chunk's start and end in it)"""
    data = bytes(data)
    assert start % CHUNK == 0 and start < end <= len(data) and end - start <= CHUNK
    lo = max(0, start - WINDOW)
    return data[lo:min(len(data), end + 8)], start - lo, end - lo


def _keys(v, width, bits):
    """the key of every position whose `width` bytes lie inside v"""
    b = np.frombuffer(v, np.uint8).astype(np.uint64)
    n = len(v) - width + 1
    if n <= 0:
        return []
    word = lambda at: sum(b[at + k:at + k + n] << np.uint64(8 * k) for k in range(4))
    h = (word(0) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    if width == 8:
        h ^= (word(4) * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    return (h >> np.uint64(32 - bits)).tolist()


def common(v, p, q, most):
    """how many of the `most` bytes at p are those at q"""
    if most <= 0 or v[p] != v[q]:
        return 0
    a, b = v[p:p + most], v[q:q + most]
    if a == b:
        return most
    lo, hi = 1, most   # a[:lo] == b[:lo], a[:hi] != b[:hi]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[:mid] == b[:mid]: lo = mid
        else: hi = mid
    return lo


class Table:
    """key -> the positions that entered, most recent first, at most `ways`"""

    def __init__(self, keys, ways, never):
        self.keys, self.ways, self.never, self.rows = keys, ways, never, {}

    def key(self, p):
        return self.keys[p] if p < len(self.keys) else None

    def enter(self, t0, t1):
        """the tile [t0, t1): per key its last position.  -> how many keys the tile held"""
        last = {}
        for p in range(t0, min(t1, len(self.keys))):
            last[self.keys[p]] = p
        for k, p in last.items():
            if p != self.never:
                self.rows[k] = ([p] + self.rows.get(k, []))[:self.ways]
        return len(last)

    def within(self, p, st, name):
        """the positions of p's key, most recent first, up to the first that is more than the window back"""
        k, out = self.key(p), []
        if k is None:
            return out
        row = self.rows.get(k, ())
        for q in row:
            if p - q > WINDOW:
                st["walk_cut_by_distance"] += 1
                break
            out.append(q)
        if len(out) == self.ways:
            st[name] += 1
        return out


def _fixed(v, p, most, st):
    """-> (f0, f1) as (length, distance) or None.  `most`: what is left of the chunk, at most 258"""
    seen = [(common(v, p, p - d, min(8, most)), d) for d in FIXED if d <= p]
    f0 = next(((n, d) for n, d in seen if n >= 3), None)
    n, d = max(seen, key=lambda x: (x[0], -x[1]), default=(0, 0))
    if not n:
        return None, None
    if p < 8 and n >= 3:
        st["fixed_match_at_p_below_8"] += 1
    if n == 8 and most > 8:
        n = common(v, p, p - d, most)
    return f0, (n, d)


# ---------------------------------------------------------------------------------------------------- the greedy tokenizer
@functools.lru_cache(maxsize=None)
def _greedy(v, s, e):
    st = collections.Counter()
    table = Table(_keys(v, 4, 9), 4, s + WINDOW - 1)
    for t0 in range(0, s, 64):
        table.enter(t0, t0 + 64)
    count = collections.Counter(v[s:e])
    lit16 = {b: min(max(ilog16(((e - s) << 8) // c), 16), 240) for b, c in count.items()}
    tokens, at = [], s
    for t0 in range(s, e, 64):
        t1, found = min(t0 + 64, e), {}
        for p in range(t0, t1):
            most = min(258, e - p)
            _, f1 = _fixed(v, p, most, st)
            n, d = f1 or (0, 0)
            for q in table.within(p, st, "greedy_row_full"):
                m = common(v, p, q, most)
                if m > n: n, d = m, p - q
            if n < 3:
                continue
            if n == 3 and d > 8:
                st["three_bytes_too_far"] += 1
                continue
            if n <= MATCH_RULE_MAXLEN and sum(lit16[b] for b in v[p:p + n]) < MATCH_BASE16 + 16 * DIST_EXTRA[dist_code(d)]:
                st["literals_cheaper"] += 1
                continue
            found[p] = (n, d)
            if p + 8 > len(v): st["match_in_last_seven"] += 1
        if table.enter(t0, t1) == 1 and t1 - t0 == 64:
            st["tile_on_one_key"] += 1
        while at < t1:
            m = found.get(at)
            if m and at + 1 < t1 and found.get(at + 1, (0, 0))[0] > m[0]:
                st["lazy"] += 1
                m = None
            tokens.append(m or (0, v[at]))
            at += m[0] if m else 1
    return tokens, st


def greedy(data, start, end, stats=None):
    tokens, st = _greedy(*_window(data, start, end))
    if stats is not None: stats.update(st)
    return list(tokens)


# ---------------------------------------------------------------------------------------------------- the candidates of the min-cost-path parse
@functools.lru_cache(maxsize=None)
def _candidates(v, s, e):
    st = collections.Counter()
    t4, t8 = Table(_keys(v, 4, 11), 4, s + WINDOW - 1), Table(_keys(v, 8, 11), 8, s + WINDOW - 1)
    for t0 in range(0, s, 256):
        t4.enter(t0, t0 + 256)
        t8.enter(t0, t0 + 256)
    out = []
    for t0 in range(s, e, 256):
        t1 = min(t0 + 256, e)
        for p in range(t0, t1):
            most = min(258, e - p)
            f0, f1 = _fixed(v, p, most, st)
            offers = {f[1]: f[0] for f in (f0, f1) if f}   # distance -> length (f1 after f0: at one distance the extended length stands)
            for q in t4.within(p, st, "row4_full") + t8.within(p, st, "row8_full"):
                if p - q not in offers:
                    offers[p - q] = common(v, p, q, most)
            n0, d0 = next(((offers[d], d) for d in sorted(offers) if offers[d] >= 3), (0, 0))
            n1, d1 = max(((n, d) for d, n in offers.items() if n), key=lambda x: (x[0], -x[1]), default=(0, 0))
            if n1 <= n0: n1, d1 = 0, 0
            out.append((n0, d0, n1, d1))
            if n0 and p + 8 > len(v): st["candidate_in_last_seven"] += 1
        t4.enter(t0, t1)
        t8.enter(t0, t1)
    return out, st


def candidates(data, start, end, stats=None):
    cand, st = _candidates(*_window(data, start, end))
    if stats is not None: stats.update(st)
    return list(cand)


# ---------------------------------------------------------------------------------------------------- costs
def costs(lit_len_counts, dist_counts, first_pass):
    """1/16 bit per literal, per length 3..258 and per distance code, from a parse's counts: 16 log2(total / count) within 1..240, a symbol that did not occur
    as if it had occurred half a time, the extra bits on top; every distance code 80 when the parse had no match.  first_pass: there is no parse yet -- the counts are
    the chunk's bytes, and both symbols of a match cost DEEP_START"""
    tl, td = sum(lit_len_counts), sum(dist_counts)
    sym = lambda f, t: cost16_of(f, t) if f else cost16_of(1, 2 * t)
    lit = [sym(lit_len_counts[b], tl) for b in range(256)]
    ln = [0] * 3 + [(DEEP_START if first_pass else sym(lit_len_counts[257 + LEN_CODE[n]], tl)) + 16 * LEN_EXTRA[LEN_CODE[n]] for n in range(3, 259)]
    ds = [(DEEP_START if first_pass else 80 if td == 0 else sym(dist_counts[c], td)) + 16 * DIST_EXTRA[c] for c in range(30)]
    return lit, ln, ds


# ---------------------------------------------------------------------------------------------------- the path
def path(data, start, end, cand, cost):
    """per segment of 512 bytes (from the chunk's start) the cheapest way to its end: to_end[i] = min over the literal, c0 at the lengths 3..min(len0, 16) and at
    len0, c1 at len0 + 1..min(len1, 16) and at len1 -- every length first cut to what is left of the segment -- by the least
    key (to_end << 9 | length) -- so the literal, then the shorter length, among equals.  All segments side by side in numpy (int64).
    -> (the choice at every position, (lit_len_counts, dist_counts) of the path from every segment's start, end-of-block counted once)"""
    lit_cost, len_cost, dist_cost = (np.array(c, np.int64) for c in cost)
    n = end - start
    nseg = -(-n // SEG)
    c = np.zeros((nseg * SEG, 4), np.int64)
    c[:n] = np.array(cand, np.int64).reshape(n, 4)
    byte = np.zeros(nseg * SEG, np.int64)
    byte[:n] = np.frombuffer(bytes(data[start:end]), np.uint8)
    grid = lambda a: a.reshape(nseg, SEG).T   # [place in the segment][segment]
    size = np.minimum(SEG, n - SEG * np.arange(nseg))
    left = np.maximum(size[None, :] - np.arange(SEG)[:, None], 0)
    n0, n1 = np.minimum(grid(c[:, 0]), left), np.minimum(grid(c[:, 2]), left)
    code = np.searchsorted(np.array(DIST_BASE), np.maximum(c[:, [1, 3]], 1), side="right") - 1
    dc0, dc1 = dist_cost[grid(code[:, 0])], dist_cost[grid(code[:, 1])]
    has0 = n0 >= 3
    has1 = has0 & (n1 > n0)
    kk = np.arange(3, CAP + 1)[None, :, None]
    short_ok = has0[:, None, :] & ((kk <= n0[:, None, :]) | (has1[:, None, :] & (kk <= n1[:, None, :])))
    short_fix = len_cost[3:CAP + 1][None, :, None] + np.where(kk <= n0[:, None, :], dc0[:, None, :], dc1[:, None, :])
    big = np.int64(1) << 60
    to_end = np.zeros((SEG + CAP + 1, nseg), np.int64)
    choice = np.ones((SEG, nseg), np.int64)
    seg = np.arange(nseg)
    for i in range(SEG - 1, -1, -1):
        best = ((to_end[i + 1] + lit_cost[grid(byte)[i]]) << 9) | 1
        key = ((to_end[i + 3:i + CAP + 1] + short_fix[i]) << 9) | kk[0]
        best = np.minimum(best, np.where(short_ok[i], key, big).min(axis=0))
        for nn, dc, ok in ((n0[i], dc0[i], has0[i] & (n0[i] > CAP)), (n1[i], dc1[i], has1[i] & (n1[i] > CAP))):
            if ok.any():
                key = ((to_end[np.minimum(i + nn, SEG), seg] + len_cost[np.minimum(nn, 258)] + dc) << 9) | nn
                best = np.minimum(best, np.where(ok, key, big))
        live = left[i] > 0
        to_end[i] = np.where(live, best >> 9, 0)
        choice[i] = np.where(live, best & 511, 1)
    flat = choice.T.reshape(-1)[:n].tolist()
    ll, dd = [0] * 286, [0] * 30
    for _, tok in _walk(data, start, end, cand, flat):
        if tok[0]:
            ll[257 + LEN_CODE[tok[0]]] += 1
            dd[dist_code(tok[1])] += 1
        else:
            ll[tok[1]] += 1
    ll[256] = 1
    return flat, (ll, dd)


def _walk(data, start, end, cand, choice):
    """(offset in the chunk, token) along the chosen path, segment by segment"""
    n = end - start
    for s0 in range(0, n, SEG):
        i, s1 = s0, min(s0 + SEG, n)
        while i < s1:
            k = choice[i]
            if k == 1:
                yield i, (0, data[start + i])
            else:
                yield i, (k, cand[i][1] if k <= min(cand[i][0], s1 - i) else cand[i][3])
            i += k
        assert i == s1, "a choice crosses its segment's end"


_PASSES = {}


def passes(data, start, end, iters):
    """every pass of the parse: [{"costs", "choice", "counts"}].  The first prices by the chunk's byte counts, each later one by the counts of the one before"""
    v, s, e = _window(data, start, end)
    done = _PASSES.setdefault((v, s, e), [])
    cand = _candidates(v, s, e)[0]
    while len(done) < iters:
        if done:
            c = costs(*done[-1]["counts"], first_pass=False)
        else:
            ll = [0] * 286
            for b in v[s:e]: ll[b] += 1
            c = costs(ll, [0] * 30, first_pass=True)
        choice, counts = path(v, s, e, cand, c)
        done.append({"costs": c, "choice": choice, "counts": counts})
    return done[:iters]


def deep(data, start, end, iters):
    assert iters >= 1
    v, s, e = _window(data, start, end)
    return [tok for _, tok in _walk(v, s, e, _candidates(v, s, e)[0], passes(data, start, end, iters)[-1]["choice"])]


# ---------------------------------------------------------------------------------------------------- which parse a chunk keeps
def counts_of(tokens):
    ll, dd = [0] * 286, [0] * 30
    for n, x in tokens:
        if n:
            ll[257 + LEN_CODE[n]] += 1
            dd[dist_code(x)] += 1
        else:
            ll[x] += 1
    ll[256] = 1
    return ll, dd


def estimate(tokens):
    """what a block of these tokens takes, in 1/16 bit: the entropy of its two alphabets (end-of-block counted once) by cost16_of, and the extra bits"""
    ll, dd = counts_of(tokens)
    tl, td = sum(ll), sum(dd)
    return (sum(f * (cost16_of(f, tl) + (16 * LEN_EXTRA[i - 257] if i > 256 else 0)) for i, f in enumerate(ll) if f)
            + sum(f * (cost16_of(f, td) + 16 * DIST_EXTRA[i]) for i, f in enumerate(dd) if f))


def chunk_kind(data, start, end, iters):
    """"greedy": too few matches for the parse (matches * 512 < tokens), or no passes asked for; "deep"; "kept": the parse was made and did not promise less"""
    g = greedy(data, start, end)
    if iters < 1 or sum(1 for t in g if t[0]) * DEEP_DIV < len(g):
        return "greedy"
    return "deep" if estimate(deep(data, start, end, iters)) < estimate(g) else "kept"


def chunk_tokens(data, start, end, iters):
    return deep(data, start, end, iters) if chunk_kind(data, start, end, iters) == "deep" else greedy(data, start, end)


def chunks_of(n):
    return [(s, min(s + CHUNK, n)) for s in range(0, n, CHUNK)]
