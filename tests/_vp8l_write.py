"""A WebP lossless (VP8L) stream WRITER for the tests, from the WebP Lossless Bitstream Specification: an LSB-first bit writer, canonical prefix codes
from chosen lengths with every form of code description selectable (simple with one or two symbols and a 1-bit or 8-bit first symbol; normal with or
without the max_symbol field; the repeat codes 16 / 17 / 18 where the lengths allow them, or none at all), the transforms in any order, the meta
prefix image, and the pixel layer as a list of events:

    ("lit", argb)   ("copy", length, distance_code)   ("cache", index)

The writer needs no forward transforms and tracks no pixels: any residual image with any transform parameters is a valid stream, and libwebp's decoder
says what it decodes to.  Only the position is tracked, so that a copy reaches neither in front of the picture nor behind it.
The 120-entry distance map is tests/_vp8l_parse.py's (the specification's table)."""
import numpy as np

from _vp8l_parse import CODE_LENGTH_ORDER, DISTANCE_MAP


class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, nbits):
        assert 0 <= v < (1 << nbits)
        self.acc |= v << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def bytes(self):
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """{symbol: (code bits as they go into the stream -- most significant code bit first --, length)}"""
    used = sorted((l, s) for s, l in enumerate(lengths) if l)
    out, code, prev = {}, 0, 0
    for l, s in used:
        code <<= l - prev
        prev = l
        out[s] = (int(format(code, "0%db" % l)[::-1], 2), l)
        code += 1
    if len(used) > 1:
        assert sum(1 << (15 - l) for l, _ in used) == 1 << 15, "not a complete code"
    return out


def tree_lengths(rng, nsym, maxlen, deep=False):
    """lengths of a complete code of nsym >= 2 leaves, none longer than maxlen; deep: a chain down to maxlen first (needs nsym > maxlen)"""
    assert 2 <= nsym <= (1 << maxlen)
    leaves = [1, 1]
    if deep and nsym > maxlen:
        while max(leaves) < maxlen:
            d = leaves.pop(leaves.index(max(leaves)))
            leaves += [d + 1, d + 1]
    while len(leaves) < nsym:
        cand = [i for i, d in enumerate(leaves) if d < maxlen]
        d = leaves.pop(int(rng.choice(cand)))
        leaves += [d + 1, d + 1]
    return leaves


def flat_lengths(nsym):
    """the complete code of nsym leaves with two neighbouring lengths (all one length when nsym is a power of two)"""
    hi = max(1, int(nsym - 1).bit_length())
    short = (1 << hi) - nsym
    return [hi - 1] * short + [hi] * (nsym - short)


class Code:
    """a prefix code and how it is described.  form: "simple" or "normal"; for normal codes rle (use the repeat codes) and counted (write max_symbol)"""

    def __init__(self, lengths, form="normal", rle=True, counted=False, first_1bit=None, swap=False, twice=False):
        self.lengths, self.form, self.rle, self.counted, self.first_1bit, self.swap, self.twice = list(lengths), form, rle, counted, first_1bit, swap, twice
        self.codes = canonical(lengths)
        self.single = len(self.codes) == 1
        self._desc = None

    def put(self, bw, sym):
        assert sym in self.codes, ("symbol without a code", sym)
        if not self.single:
            bw.put(*self.codes[sym])

    def tokens(self):
        """the lengths as code-length symbols [(symbol, extra value, extra bits)]"""
        L, out, i, prev = self.lengths, [], 0, 8
        end = len(L)
        if self.counted:
            while end > 0 and L[end - 1] == 0:
                end -= 1
        while i < end:
            v, r = L[i], 1
            while i + r < end and L[i + r] == v:
                r += 1
            if not self.rle:
                out.append((v, 0, 0)); i += 1
                continue
            if v == 0:
                if r >= 11:
                    k = min(r, 138); out.append((18, k - 11, 7))
                elif r >= 3:
                    k = r; out.append((17, k - 3, 3))
                else:
                    k = 1; out.append((0, 0, 0))
                i += k
                continue
            if v != prev:
                out.append((v, 0, 0)); prev = v; i += 1; r -= 1
            while r >= 3:
                k = min(r, 6); out.append((16, k - 3, 2)); i += k; r -= k
            for _ in range(r):
                out.append((v, 0, 0)); i += 1
        return out

    def describe(self, bw):
        if self._desc is None:   # (a code shared by many groups is described once and replayed)
            rec = []
            self._describe(type("Rec", (), {"put": staticmethod(lambda v, n: rec.append((v, n)))}))
            self._desc = rec
        for v, n in self._desc:
            bw.put(v, n)

    def _describe(self, bw):
        if self.form == "simple":
            syms = sorted(self.codes)
            assert len(syms) <= 2 and max(syms) < 256
            if self.swap:
                syms = syms[::-1]
            if self.twice:
                assert len(syms) == 1
                syms = syms * 2   # the same symbol named twice: a code with one symbol
            one_bit = syms[0] < 2 if self.first_1bit is None else self.first_1bit
            assert not one_bit or syms[0] < 2
            bw.put(1, 1); bw.put(len(syms) - 1, 1); bw.put(0 if one_bit else 1, 1); bw.put(syms[0], 1 if one_bit else 8)
            if len(syms) == 2:
                bw.put(syms[1], 8)
            return
        toks = self.tokens()
        hist = [0] * 19
        for s, _, _ in toks:
            hist[s] += 1
        used = [s for s in range(19) if hist[s]]
        cl = [0] * 19
        if len(used) == 1:
            cl[used[0]] = 1
        else:
            for s, l in zip(sorted(used, key=lambda s: -hist[s]), sorted(flat_lengths(len(used)))):
                cl[s] = l
        ncl = max(4, 1 + max(i for i in range(19) if cl[CODE_LENGTH_ORDER[i]]))
        bw.put(0, 1); bw.put(ncl - 4, 4)
        for i in range(ncl):
            bw.put(cl[CODE_LENGTH_ORDER[i]], 3)
        if self.counted:
            assert len(toks) >= 2
            nb = 2
            while (len(toks) - 2) >> nb:
                nb += 2
            bw.put(1, 1); bw.put((nb - 2) // 2, 3); bw.put(len(toks) - 2, nb)
        else:
            bw.put(0, 1)
        ccodes = canonical(cl)
        for s, x, xb in toks:
            if len(used) > 1:
                bw.put(*ccodes[s])
            bw.put(x, xb)


def prefix_of(v):
    """LZ77 prefix coding of a length or distance code v >= 1: (prefix symbol, extra value, extra bits)"""
    if v <= 4:
        return v - 1, 0, 0
    d = v - 1
    h = d.bit_length() - 1
    return 2 * h + ((d >> (h - 1)) & 1), d & ((1 << (h - 1)) - 1), h - 1


def plane_distance(dcode, xs):
    if dcode > 120:
        return dcode - 120
    dx, dy = DISTANCE_MAP[dcode - 1]
    return max(1, dx + dy * xs)


def event_symbols(ev):
    """what an event needs of the five codes: [(which code, symbol)]"""
    if ev[0] == "lit":
        v = ev[1]
        return [(0, (v >> 8) & 255), (1, (v >> 16) & 255), (2, v & 255), (3, v >> 24)]
    if ev[0] == "copy":
        return [(0, 256 + prefix_of(ev[1])[0]), (4, prefix_of(ev[2])[0])]
    return [(0, 256 + 24 + ev[1])]


def default_code_maker(rng, maxlen=15, extra=(0, 12), forms=True):
    """-> make(group, which, needed symbols, alphabet) -> Code: the needed symbols and some more, lengths from a random tree, and a description form drawn
    from those the symbols allow"""
    def make(g, k, need, alphabet):
        need = set(need)
        want = len(need) + int(rng.integers(extra[0], extra[1] + 1))
        while len(need) < min(max(want, 1), alphabet):
            need.add(int(rng.integers(0, alphabet)))
        syms = sorted(need)
        lengths = [0] * alphabet
        if len(syms) == 1:
            lengths[syms[0]] = int(rng.integers(1, 8))
            if forms and syms[0] < 256 and rng.random() < 0.6:
                return Code(lengths, "simple", first_1bit=False if rng.random() < 0.5 else None, twice=rng.random() < 0.3)
            return Code(lengths, "normal", rle=rng.random() < 0.7, counted=rng.random() < 0.5 and syms[0] >= 1)
        if len(syms) == 2 and forms and syms[1] < 256 and rng.random() < 0.7:
            lengths[syms[0]] = lengths[syms[1]] = 1
            return Code(lengths, "simple", first_1bit=False if rng.random() < 0.5 else None, swap=rng.random() < 0.5 and syms[1] >= 2)
        ml = maxlen
        while (1 << ml) < len(syms):
            ml += 1
        tl = tree_lengths(rng, len(syms), ml, deep=rng.random() < 0.5)
        rng.shuffle(tl)
        for s, l in zip(syms, tl):
            lengths[s] = int(l)
        counted = rng.random() < 0.4
        return Code(lengths, "normal", rle=rng.random() < 0.7, counted=counted)
    return make


def encode_image(bw, xs, ys, events, make, *, cache_bits=0, meta=None, level0=True, sub_make=None):
    """one entropy-coded image: colour-cache bits, (level0) the meta prefix image -- meta = (bits, group of every tile as an (mh, mw) array) --, the codes of
    every group, the events"""
    bw.put(1 if cache_bits else 0, 1)
    if cache_bits:
        bw.put(cache_bits, 4)
    ngroups, prec, gmap = 1, 0, None
    if level0:
        bw.put(1 if meta else 0, 1)
        if meta:
            prec, gmap = meta
            gmap = np.asarray(gmap)
            assert gmap.shape == ((ys + (1 << prec) - 1) >> prec, (xs + (1 << prec) - 1) >> prec)
            bw.put(prec - 2, 3)
            ngroups = int(gmap.max()) + 1
            sub = sub_make or make
            encode_image(bw, gmap.shape[1], gmap.shape[0], [("lit", int(g) << 8) for g in gmap.reshape(-1)], sub, level0=False)
    else:
        assert not meta
    cache_size = (1 << cache_bits) if cache_bits else 0
    alpha = [256 + 24 + cache_size, 256, 256, 256, 40]
    total, pos = xs * ys, 0
    need = [[set() for _ in range(5)] for _ in range(ngroups)]
    where = []
    for ev in events:
        g = int(gmap[(pos // xs) >> prec, (pos % xs) >> prec]) if gmap is not None else 0
        where.append(g)
        for k, s in event_symbols(ev):
            need[g][k].add(s)
        if ev[0] == "copy":
            assert 1 <= ev[1] <= 4096 and plane_distance(ev[2], xs) <= pos and pos + ev[1] <= total, ("copy out of the picture", ev, pos)
            pos += ev[1]
        else:
            assert ev[0] != "cache" or ev[1] < cache_size
            pos += 1
    assert pos == total, (pos, total)
    groups = []
    for g in range(ngroups):
        codes = [make(g, k, need[g][k], alpha[k]) for k in range(5)]
        for c in codes:
            c.describe(bw)
        groups.append(codes)
    for ev, g in zip(events, where):
        c = groups[g]
        if ev[0] == "lit":
            for k, s in event_symbols(ev):
                c[k].put(bw, s)
        elif ev[0] == "copy":
            s, x, xb = prefix_of(ev[1])
            c[0].put(bw, 256 + s); bw.put(x, xb)
            s, x, xb = prefix_of(ev[2])
            c[4].put(bw, s); bw.put(x, xb)
        else:
            c[0].put(bw, 256 + 24 + ev[1])
    return groups


def literals(values):
    return [("lit", int(v)) for v in np.asarray(values).reshape(-1)]


def random_events(rng, xs, ys, *, cache_bits=0, p_copy=0.15, p_cache=0.1, dcodes=None, lengths=None, values=None):
    """literals from `values` (an array of ARGB values to draw from; default: few distinct ones per channel), copies at the given distance codes and lengths
    where they fit, cache indices anywhere below the cache size"""
    total, pos, out = xs * ys, 0, []
    if values is None:
        ch = [rng.integers(0, 256, 6) for _ in range(4)]
        values = [(int(rng.choice(ch[0])) << 24) | (int(rng.choice(ch[1])) << 16) | (int(rng.choice(ch[2])) << 8) | int(rng.choice(ch[3])) for _ in range(64)]
    dcodes = list(range(1, 121)) + [121, 122, 125, 120 + xs, 120 + 3 * xs + 1] if dcodes is None else dcodes
    lengths = [1, 2, 3, 4, 5, 7, 8, 9, 16, 31, 64, 65, 130, 700, 4096] if lengths is None else lengths
    while pos < total:
        r = rng.random()
        if r < p_copy and pos:
            dc = int(rng.choice(dcodes))
            ln = min(int(rng.choice(lengths)), total - pos)
            if plane_distance(dc, xs) <= pos:
                out.append(("copy", ln, dc)); pos += ln
                continue
        if r > 1 - p_cache and cache_bits:
            out.append(("cache", int(rng.integers(0, 1 << cache_bits)))); pos += 1
            continue
        out.append(("lit", int(values[int(rng.integers(0, len(values)))]))); pos += 1
    return out


def write_stream(width, height, events, make, *, transforms=(), cache_bits=0, meta=None, headerless=False, alpha_used=1, sub_make=None, info=None):
    """a VP8L stream.  transforms, in stream order: ("predictor", bits, data) / ("cross", bits, data) with data an array of ARGB values of the sub-image's
    shape, ("green",), ("palette", ARGB residuals of the colours).  `events` describe the picture as the stream carries it: (packed width) x height, where
    packed_width(width, transforms) is the width behind a palette of <= 16 colours.  meta / cache_bits: of the picture."""
    bw = BitWriter()
    if not headerless:
        bw.put(0x2F, 8); bw.put(width - 1, 14); bw.put(height - 1, 14); bw.put(alpha_used, 1); bw.put(0, 3)
    sub = sub_make or make
    xs = width
    for t in transforms:
        bw.put(1, 1)
        if t[0] in ("predictor", "cross"):
            bits, data = t[1], np.asarray(t[2])
            bw.put(0 if t[0] == "predictor" else 1, 2); bw.put(bits - 2, 3)
            assert data.shape == ((height + (1 << bits) - 1) >> bits, (xs + (1 << bits) - 1) >> bits), (data.shape, t[0], bits)
            encode_image(bw, data.shape[1], data.shape[0], literals(data), sub, level0=False)
        elif t[0] == "green":
            bw.put(2, 2)
        else:
            pal = np.asarray(t[1]).reshape(-1)
            bw.put(3, 2); bw.put(len(pal) - 1, 8)
            encode_image(bw, len(pal), 1, literals(pal), sub, level0=False)
            xs = packed_width(xs, [t])
    bw.put(0, 1)
    groups = encode_image(bw, xs, height, events, make, cache_bits=cache_bits, meta=meta, level0=True, sub_make=sub)
    if info is not None:
        info["groups"] = groups   # the picture's codes, for a test that has to know how many symbols each one holds
    return bw.bytes()


def packed_width(width, transforms):
    for t in transforms:
        if t[0] == "palette":
            n = len(np.asarray(t[1]).reshape(-1))
            bits = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            width = (width + (1 << bits) - 1) >> bits
    return width


def _chunk(tag, data):
    return tag + len(data).to_bytes(4, "little") + data + (b"\0" if len(data) & 1 else b"")


def riff(chunks):
    body = b"WEBP" + b"".join(chunks)
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def vp8l_file(stream):
    return riff([_chunk(b"VP8L", stream)])


def alph_file(width, height, lossy_file, filt, method, data, pre=0):
    """an extended-format file: VP8X with the alpha flag, ALPH (header byte, then `data`: the raw plane for method 0, a headerless VP8L stream for method 1),
    and the VP8 chunk of `lossy_file` (a simple-format lossy file of the same size)"""
    assert lossy_file[12:16] == b"VP8 "
    n = int.from_bytes(lossy_file[16:20], "little")
    vp8x = bytes([0x10, 0, 0, 0]) + (width - 1).to_bytes(3, "little") + (height - 1).to_bytes(3, "little")
    return riff([_chunk(b"VP8X", vp8x), _chunk(b"ALPH", bytes([method | (filt << 2) | (pre << 4)]) + data), _chunk(b"VP8 ", lossy_file[20:20 + n])])
