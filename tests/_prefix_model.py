"""The plain statement of the prefix codes this library builds from a histogram, written from the standards and from nothing else:
ITU-T T.81 Annex K.2 (Figures K.1 to K.4: code sizes by repeated merge with the `others` chain, the counts, the bit-count adjustment, the order
of the symbols), Annex C.2 (canonical JPEG codes) and RFC 1951 3.2.2 (canonical DEFLATE codes).  Python integers only; no numpy, no library, no
oracle.  tests/test_prefix_model.py proves it; the device units (tests/_devunit_cases.py) and the file-level checks (tests/test_code_tables_emul.py)
hold the three builders of the library to it: k_gen_tables, csp::code_lengths + csp::canonical, csw::code_lengths_wide.

The one thing K.2 leaves open is which of several equal frequencies is taken.  libjpeg's reading, which the library states as its rule, is "the
larger index": it is written here once, in k2_sizes.  What does not depend on that rule (completeness, the limit, optimality where the limit does
not bind) has its own functions at the end, so that a test can tell a wrong tie from a wrong code."""
import functools
import heapq


def k2_sizes(freq):
    """Figure K.1 (Code_size) over the symbols 0 .. len(freq) - 1.  V1: the least non-zero frequency, the largest index on a tie; V2: the same among
    the rest; the sum stays in V1's slot, V2's becomes 0; every symbol of both chains grows by one bit and V2's chain is hung behind V1's.
    -> code size per symbol (0: not coded; a single used symbol has size 0 too, as in the figure)"""
    freq = [int(f) for f in freq]
    n = len(freq)
    codesize, others = [0] * n, [-1] * n
    # "least frequency, the largest index on a tie" as one integer per live symbol: frequency above, n - 1 - index below; min() is then the figure's search
    sh = n.bit_length()
    live = [(freq[i] << sh) | (n - 1 - i) for i in range(n) if freq[i] > 0]
    while len(live) >= 2:
        k1 = min(live)
        live.remove(k1)
        k2 = min(live)
        live.remove(k2)
        v1, v2 = n - 1 - (k1 & ((1 << sh) - 1)), n - 1 - (k2 & ((1 << sh) - 1))
        freq[v1] += freq[v2]
        freq[v2] = 0
        live.append((freq[v1] << sh) | (n - 1 - v1))
        codesize[v1] += 1
        while others[v1] >= 0:
            v1 = others[v1]
            codesize[v1] += 1
        others[v1] = v2
        codesize[v2] += 1
        while others[v2] >= 0:
            v2 = others[v2]
            codesize[v2] += 1
    return codesize


def count_sizes(codesize):
    """Figure K.2 (Count_BITS): bits[i] = how many symbols have size i, i = 1 .. the largest size (bits[0] stays 0)"""
    bits = [0] * (max(codesize, default=0) + 1)
    for s in codesize:
        if s > 0: bits[s] += 1
    return bits


def k2_adjust(bits, limit):
    """Figure K.3 (Adjust_BITS), its loop from the top length down to limit + 1: while a length above the limit holds codes, two of them give way
    to one code a bit shorter, and the longest shorter code J becomes two of J + 1 bits.  (The figure's last step, the reserved code point, is
    jpeg_table's.)  -> the counts for 0 .. limit"""
    bits = list(bits) + [0] * (limit + 1 - len(bits))
    i = len(bits) - 1
    while i > limit:
        if bits[i] > 0:
            j = i - 1
            while True:
                j -= 1
                if bits[j] > 0: break
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        else:
            i -= 1
    return bits[:limit + 1]


def jpeg_codes(bits, huffval):
    """Annex C.2 (Figures C.1 to C.3): the size table from BITS, the codes counting up within a size and doubling between sizes, handed to the
    symbols in HUFFVAL's order.  -> code[256], size[256]"""
    huffsize = [l for l in range(1, 17) for _ in range(bits[l])]
    huffcode, c = [], 0
    for k, s in enumerate(huffsize):
        if k and s != huffsize[k - 1]: c <<= s - huffsize[k - 1]
        huffcode.append(c)
        c += 1
    code, size = [0] * 256, [0] * 256
    for k, v in enumerate(huffval):
        code[v], size[v] = huffcode[k], huffsize[k]
    return code, size


@functools.lru_cache(None)
def _jpeg_table(freq256):
    sizes = k2_sizes(list(freq256) + [1])                 # K.2: "FREQ(256) is set to 1": the reserved code point, so that no code is all ones
    depth = max(sizes)
    bits = k2_adjust(count_sizes(sizes), 16)
    i = 16
    while i > 0 and bits[i] == 0: i -= 1
    if i > 0: bits[i] -= 1                                # Figure K.3's end: the reserved code point leaves the longest length
    huffval = [s for _, s in sorted((sizes[s], s) for s in range(256) if sizes[s] > 0)]   # Figure K.4 (Sort_input)
    code, size = jpeg_codes(bits, huffval)
    return tuple(bits), tuple(huffval), tuple(code), tuple(size), depth


def jpeg_table(freq256):
    """the JPEG table of 256 symbol counts -> bits[17], vals, code[256], size[256], the unlimited depth (of the 257 entries, the reserved one included)"""
    assert len(freq256) == 256
    return _jpeg_table(tuple(int(f) for f in freq256))


@functools.lru_cache(None)
def _limited_lengths(freq, limit):
    freq = list(freq)
    for i in range(len(freq)):                            # zlib's rule: at least two codes, the lowest unused symbols at frequency 1
        if sum(1 for f in freq if f) >= 2: break
        if not freq[i]: freq[i] = 1
    sizes = k2_sizes(freq)
    bits = k2_adjust(count_sizes(sizes), limit)
    lengths = [l for l in range(1, limit + 1) for _ in range(bits[l])]
    out = [0] * len(freq)
    for (_, s), l in zip(sorted((sizes[s], s) for s in range(len(freq)) if sizes[s] > 0), lengths):
        out[s] = l
    return tuple(out), max(sizes)


def limited_lengths(freq, limit):
    """code lengths of at most `limit` bits for the counts `freq` (at least two symbols are coded) -> lengths, the unlimited depth.
    The symbols ordered by (unlimited size, index) take the adjusted lengths, the shortest first."""
    assert len(freq) >= 2
    return _limited_lengths(tuple(int(f) for f in freq), int(limit))


def canonical_codes(lengths):
    """RFC 1951 3.2.2: bl_count, next_code, then the symbols in order -> the codes, most significant bit first"""
    top = max(lengths, default=0)
    bl_count = [0] * (top + 1)
    for l in lengths:
        if l: bl_count[l] += 1
    next_code, c = [0] * (top + 2), 0
    for b in range(1, top + 1):
        c = (c + bl_count[b - 1]) << 1
        next_code[b] = c
    out = []
    for l in lengths:
        out.append(next_code[l] if l else 0)
        if l: next_code[l] += 1
    return out


def deflate_codes(lengths):
    """the same codes as the packer stores them: bit-reversed, so that an LSB-first writer sends a code from its most significant bit"""
    return [int(format(c, f"0{l}b")[::-1], 2) if l else 0 for c, l in zip(canonical_codes(lengths), lengths)]


# ---------------------------------------------------------------------------------------------------- what holds whatever the tie rule
def kraft(lengths, limit):
    """sum of 2^(limit - len) over the coded symbols: 2^limit for a complete code, more for one that cannot exist"""
    return sum(1 << (limit - l) for l in lengths if l)


def huffman_cost(freq):
    """the least sum of frequency x length over all prefix codes of the used symbols: the sum of the merged weights (0 for fewer than two symbols)"""
    h = [int(f) for f in freq if f]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a = heapq.heappop(h) + heapq.heappop(h)
        cost += a
        heapq.heappush(h, a)
    return cost


def check_lengths(freq, lengths, limit):
    """a length for every used symbol and for no other (but for the symbols forced in to make two), none above the limit, and a complete code"""
    used = [i for i, f in enumerate(freq) if f]
    coded = [i for i, l in enumerate(lengths) if l]
    assert len(coded) >= 2 and set(used) <= set(coded) and len(coded) == max(2, len(used)), (used, coded)
    assert max(lengths) <= limit
    assert kraft(lengths, limit) == 1 << limit, (kraft(lengths, limit), limit)
