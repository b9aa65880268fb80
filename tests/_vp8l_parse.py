"""A small reader of the lossless WebP (VP8L) bitstream, written from the WebP Lossless Bitstream Specification and independent of this
repository's decoder (caesium-clt_amd/csrc/vp8l_dec.h): the tests use it to see WHICH tools a stream uses -- the colour-cache size, how many
literals / cache hits / backward references code the picture, every (length, distance, position) -- and to decode the pixels a second way.

    info = parse(blob)          # blob: a RIFF file with a VP8L chunk, or a bare VP8L payload with headerless=(width, height)
    info.cache_bits, info.literals, info.cache_hits, info.refs -> [(length, distance, position)], info.argb -> (h, w) uint32 array
    info.codes -> [(where, group, which, Code)] of every prefix code in the stream, in stream order: where "argb" (the picture), "meta" (the entropy image) or
                  "transform"; which 0 .. 4 (green, red, blue, alpha, distance).  A Code keeps its lengths and how often each symbol was read with it (count); a
                  normally coded one (not simple) also the code-length code that described it (cl_lengths), the use of ITS symbols (cl_count) and
                  whether the description states how many lengths it lists (cl_counted)
"""
import numpy as np

CODE_LENGTH_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
# the specification's (dx, dy) of the distance codes 1 .. 120
DISTANCE_MAP = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3), (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2),
                (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5),
                (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2),
                (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4),
                (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6),
                (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]
assert len(DISTANCE_MAP) == 120


class Bits:
    def __init__(self, data):
        self.data = bytes(data) + b"\0" * 16
        self.pos = 0
        self.nbits = 8 * len(data)

    def peek(self, n):
        b = self.pos >> 3
        return (int.from_bytes(self.data[b:b + 8], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def read(self, n):
        v = self.peek(n) if n else 0
        self.pos += n
        assert self.pos <= self.nbits, "read past the end of the stream"
        return v


class Code:
    """canonical prefix code from code lengths; the stream carries a code's bits from its most significant one"""

    def __init__(self, lengths):
        self.lengths, self.count, self.simple, self.cl_lengths, self.cl_count = list(lengths), [0] * len(lengths), False, None, None
        used = [(l, s) for s, l in enumerate(lengths) if l]
        assert used, "a code without symbols"
        self.single = used[0][1] if len(used) == 1 else None
        if self.single is not None:
            return
        self.maxlen = max(l for l, _ in used)
        self.table = [None] * (1 << self.maxlen)
        code, prev, left = 0, 0, 1
        for l, s in sorted(used):
            code <<= l - prev
            left = (left << (l - prev)) - 1
            assert left >= 0, "over-subscribed code"
            prev = l
            rev = int(format(code, "0%db" % l)[::-1], 2)
            for i in range(rev, 1 << self.maxlen, 1 << l):
                self.table[i] = (s, l)
            code += 1
        assert left == 0, "incomplete code"

    def read(self, br):
        if self.single is not None:
            self.count[self.single] += 1
            return self.single
        s, l = self.table[br.peek(self.maxlen)]
        br.pos += l
        self.count[s] += 1
        return s


def read_code(br, alphabet):
    lengths = [0] * alphabet
    if br.read(1):
        n = br.read(1) + 1
        s0 = br.read(8 if br.read(1) else 1)
        lengths[s0] = 1
        if n == 2:
            lengths[br.read(8)] = 1
        c = Code(lengths)
        c.simple = True
        return c
    ncl = 4 + br.read(4)
    cl = [0] * 19
    for i in range(ncl):
        cl[CODE_LENGTH_ORDER[i]] = br.read(3)
    cc = Code(cl)
    max_symbol, counted = alphabet, False
    if br.read(1):
        counted = True
        max_symbol = 2 + br.read(2 + 2 * br.read(3))
        assert max_symbol <= alphabet
    s, prev = 0, 8
    while s < alphabet and max_symbol:
        max_symbol -= 1
        v = cc.read(br)
        if v < 16:
            lengths[s] = v
            s += 1
            if v:
                prev = v
        else:
            rep = br.read({16: 2, 17: 3, 18: 7}[v]) + (11 if v == 18 else 3)
            assert s + rep <= alphabet
            if v == 16:
                lengths[s:s + rep] = [prev] * rep
            s += rep
    c = Code(lengths)
    c.cl_lengths, c.cl_count, c.cl_counted = cl, cc.count, counted   # cl_counted: the stream says how many lengths follow
    return c


def prefix_value(br, sym):
    if sym < 4:
        return sym + 1
    extra = (sym - 2) >> 1
    return ((2 + (sym & 1)) << extra) + br.read(extra) + 1


class Stats:
    pass


def read_pixels(br, w, h, level0, st=None, codes=None, where="transform"):
    """an entropy-coded ARGB image -> list of w * h values; st (level 0 only) receives the counts; codes: a list that receives (where, group, which, Code)"""
    cache_bits = br.read(4) if br.read(1) else 0
    assert cache_bits == 0 or 1 <= cache_bits <= 11
    prec, meta, mw, ngroups = 0, None, 0, 1
    if level0 and br.read(1):
        prec = br.read(3) + 2
        mw, mh = -(-w >> prec), -(-h >> prec)
        meta = [(v >> 8) & 0xFFFF for v in read_pixels(br, mw, mh, False, codes=codes, where="meta")]
        ngroups = max(meta) + 1
    csize = (1 << cache_bits) if cache_bits else 0
    groups = [[read_code(br, n) for n in (256 + 24 + csize, 256, 256, 256, 40)] for _ in range(ngroups)]
    if codes is not None:
        codes += [("argb" if level0 else where, gi, k, c) for gi, g in enumerate(groups) for k, c in enumerate(g)]
    cache = [0] * csize
    out = [0] * (w * h)
    n, pos, shift = w * h, 0, 32 - cache_bits
    lit = hits = 0
    refs = []
    g = groups[0]
    while pos < n:
        if meta is not None:
            y, x = divmod(pos, w)
            g = groups[meta[(y >> prec) * mw + (x >> prec)]]
        s = g[0].read(br)
        if s < 256:
            r = g[1].read(br)   # the order in the stream: green, red, blue, alpha
            b = g[2].read(br)
            v = (g[3].read(br) << 24) | (r << 16) | (s << 8) | b
            lit += 1
        elif s < 280:
            length = prefix_value(br, s - 256)
            dcode = prefix_value(br, g[4].read(br))
            if dcode > 120:
                dist = dcode - 120
            else:
                dx, dy = DISTANCE_MAP[dcode - 1]
                dist = max(1, dx + dy * w)
            assert dist <= pos and pos + length <= n, "a copy outside the picture"
            refs.append((length, dist, pos))
            for _ in range(length):
                v = out[pos - dist]
                out[pos] = v
                if csize:
                    cache[((0x1E35A7BD * v) & 0xFFFFFFFF) >> shift] = v
                pos += 1
            continue
        else:
            assert s - 280 < csize
            v = cache[s - 280]
            hits += 1
        out[pos] = v
        if csize:
            cache[((0x1E35A7BD * v) & 0xFFFFFFFF) >> shift] = v
        pos += 1
    if st is not None:
        st.cache_bits, st.literals, st.cache_hits, st.refs, st.meta_prefix = cache_bits, lit, hits, refs, meta is not None
    return out


def _add(a, b):
    return (((a & 0xFF00FF00) + (b & 0xFF00FF00)) & 0xFF00FF00) | (((a & 0x00FF00FF) + (b & 0x00FF00FF)) & 0x00FF00FF)


def _avg(a, b):
    return (((a ^ b) & 0xFEFEFEFE) >> 1) + (a & b)


def _ch(v):
    return (v >> 24, (v >> 16) & 255, (v >> 8) & 255, v & 255)


def _pack(c):
    return (c[0] << 24) | (c[1] << 16) | (c[2] << 8) | c[3]


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _predict(mode, L, T, TR, TL):
    if mode == 0:
        return 0xFF000000
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    if mode == 11:
        l, t, tl = _ch(L), _ch(T), _ch(TL)
        pl = sum(abs(t[i] - tl[i]) for i in range(4))   # |estimate - L| with estimate = L + T - TL
        pt = sum(abs(l[i] - tl[i]) for i in range(4))
        return L if pl < pt else T
    if mode == 12:
        l, t, tl = _ch(L), _ch(T), _ch(TL)
        return _pack([_clip(l[i] + t[i] - tl[i]) for i in range(4)])
    if mode == 13:
        a, tl = _ch(_avg(L, T)), _ch(TL)
        return _pack([_clip(a[i] + (a[i] - tl[i]) // 2 if a[i] >= tl[i] else a[i] - ((tl[i] - a[i]) // 2)) for i in range(4)])   # (a - tl) / 2 truncates towards zero
    return 0xFF000000


def _s8(v):
    return v - 256 if v >= 128 else v


def parse(blob, headerless=None):
    if headerless is None:
        assert blob[:4] == b"RIFF" and blob[8:16] == b"WEBPVP8L"
        size = int.from_bytes(blob[16:20], "little")
        br = Bits(blob[20:20 + size])
        assert br.read(8) == 0x2F
        W, H = br.read(14) + 1, br.read(14) + 1
        br.read(1)
        assert br.read(3) == 0
    else:
        br = Bits(blob)
        W, H = headerless
    transforms, xs, seen, codes = [], W, set(), []
    while br.read(1):
        t = br.read(2)
        assert t not in seen
        seen.add(t)
        if t in (0, 1):
            bits = br.read(3) + 2
            bw, bh = -(-xs >> bits), -(-H >> bits)
            transforms.append((t, bits, xs, read_pixels(br, bw, bh, False, codes=codes)))
        elif t == 2:
            transforms.append((t, 0, xs, None))
        else:
            ncol = br.read(8) + 1
            pal = read_pixels(br, ncol, 1, False, codes=codes)
            for i in range(1, ncol):
                pal[i] = _add(pal[i], pal[i - 1])
            bits = 0 if ncol > 16 else 1 if ncol > 4 else 2 if ncol > 2 else 3
            transforms.append((t, bits, xs, pal))
            xs = -(-xs >> bits)
    st = Stats()
    px = read_pixels(br, xs, H, True, st, codes=codes)
    st.codes = codes
    st.width, st.height, st.transforms, st.payload_bits = W, H, [t[0] for t in transforms], br.pos
    for t, bits, tw, data in reversed(transforms):
        if t == 2:
            a = np.array(px, dtype=np.uint32)
            g = (a >> 8) & 255
            px = ((a & 0xFF00FF00) | (((a & 0x00FF00FF) + ((g << 16) | g)) & 0x00FF00FF)).tolist()
        elif t == 0:
            bw = -(-tw >> bits)
            for y in range(H):
                row = y * tw
                for x in range(tw):
                    i = row + x
                    if y == 0:
                        pred = 0xFF000000 if x == 0 else px[i - 1]
                    elif x == 0:
                        pred = px[i - tw]
                    else:
                        mode = (data[(y >> bits) * bw + (x >> bits)] >> 8) & 15
                        if mode == 1:
                            pred = px[i - 1]
                        elif mode == 2:
                            pred = px[i - tw]
                        else:
                            pred = _predict(mode, px[i - 1], px[i - tw], px[i - tw + 1], px[i - tw - 1])   # (the last pixel's top-right is the row's own first)
                    px[i] = _add(px[i], pred)
        elif t == 1:
            bw = -(-tw >> bits)
            for y in range(H):
                for x in range(tw):
                    m = data[(y >> bits) * bw + (x >> bits)]
                    g2r, g2b, r2b = _s8(m & 255), _s8((m >> 8) & 255), _s8((m >> 16) & 255)
                    p = px[y * tw + x]
                    green = _s8((p >> 8) & 255)
                    r = (((p >> 16) & 255) + ((g2r * green) >> 5)) & 255
                    b = ((p & 255) + ((g2b * green) >> 5) + ((r2b * _s8(r)) >> 5)) & 255
                    px[y * tw + x] = (p & 0xFF00FF00) | (r << 16) | b
        else:
            pw, per, nb = -(-tw >> bits), 1 << bits, 8 >> bits
            out = [0] * (tw * H)
            for y in range(H):
                for x in range(tw):
                    packed = (px[y * pw + (x >> bits)] >> 8) & 255
                    idx = (packed >> (nb * (x & (per - 1)))) & ((1 << nb) - 1) if bits else packed
                    out[y * tw + x] = data[idx] if idx < len(data) else 0
            px = out
    st.argb = np.array(px, dtype=np.uint32).reshape(H, W)
    return st


def rgba_of(argb):
    """(h, w) ARGB words -> (h, w, 4) uint8 RGBA"""
    return np.dstack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255, argb >> 24]).astype(np.uint8)
