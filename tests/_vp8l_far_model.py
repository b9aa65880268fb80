"""What k_vp8l_far.hip's link stage and k_vp8l_match_far compute (CSH_VP8L=far), restated from their definitions: a dictionary-based
previous-occurrence scan for prev[], and the finder's rule position by position.  Hashes are Python integers; the only numpy here compares two slices.  Nothing
is taken from either build of the kernels."""
import numpy as np

M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF      # VP8L_FAR_NONE
MAX_LEN = 4096         # VP8L_MAX_LEN
MIN_MATCH = 3          # VP8L_MIN_MATCH
WINDOW = (1 << 20) - 120
LINKS = 8              # VP8L_FAR_LINKS


def hash24(a, b, c):
    return (((((a * 0x9E3779B1) & M32) ^ ((b * 0x85EBCA6B) & M32) ^ ((c * 0xC2B2AE35) & M32)) * 0x27D4EB2F) & M32) >> 8


def linked(px, p):
    """the degenerate-bucket rule: the inside of a flat run, px[p - 1] == px[p] == px[p + 1] == px[p + 2], has no link and is no link's target; nor has a position
    without three pixels"""
    if p + 3 > len(px):
        return False
    return not (p >= 1 and px[p - 1] == px[p] == px[p + 1] == px[p + 2])


def links(px):
    """prev[p] = the largest q < p, both linked, whose three pixels hash like p's; NONE where there is none"""
    px = [int(v) for v in px]
    last, prev = {}, [NONE] * len(px)
    for p in range(len(px)):
        if linked(px, p):
            h = hash24(px[p], px[p + 1], px[p + 2])
            prev[p] = last.get(h, NONE)
            last[h] = p
    return prev


def min_len(dist):
    """a copy found through a link is at least this long"""
    return MIN_MATCH + (1 if dist >= 4096 else 0) + (1 if dist >= 65536 else 0)


def fixed_distances(width):
    """in the order ties are settled; a distance named twice counts once, a distance of 0 not at all"""
    out = []
    for d in (1, width, width + 1, width - 1, 2):
        if d and d not in out:
            out.append(d)
    return out


def common(a, p, q, cap):
    """how many of a[p ..] and a[q ..] agree from the start, at most cap"""
    ne = np.flatnonzero(a[p:p + cap] != a[q:q + cap])
    return int(ne[0]) if ne.size else cap


def candidates(px, width, prev):
    """per position (length, distance) as k_vp8l_match_far leaves them: the longest copy among the fixed distances (the first in their order on a tie), then the
    links nearest first, at most LINKS of them while they stay in the window -- one at a fixed distance is passed by and still counted -- of which only a strictly
    longer copy of at least min_len replaces the best; nothing once the cap is reached; (0, 0) below MIN_MATCH"""
    a = np.asarray(px, np.uint32)
    n = len(a)
    fixed = fixed_distances(width)
    runs = []
    for d in fixed:   # run[i] = a[i] == a[i - d] ? 1 + run[i + 1] : 0
        run = [0] * (n + 1)
        for i in range(n - 1, d - 1, -1):
            if a[i] == a[i - d]:
                run[i] = run[i + 1] + 1
        runs.append(run)
    out = []
    for p in range(n):
        cap = min(MAX_LEN, n - p)
        bl, bd = 0, 0
        for d, run in zip(fixed, runs):
            length = min(run[p], MAX_LEN)
            if length > bl:
                bl, bd = length, d
        q = p
        for _ in range(LINKS):
            if bl >= cap:
                break
            q = prev[q]
            if q == NONE or p - q > WINDOW:
                break
            d = p - q
            if d in fixed:
                continue
            length = common(a, p, q, cap)
            if length > bl and length >= min_len(d):
                bl, bd = length, d
        out.append((bl, bd) if bl >= MIN_MATCH else (0, 0))
    return out


def tokens(px, width, prev):
    """candidates() as the words the kernel stores: bits 0-15 the length, from bit 16 the distance"""
    return np.array([l | (d << 16) for l, d in candidates(px, width, prev)], np.uint64)
