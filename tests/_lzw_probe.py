"""Byte strings that drive the LZW encoders' dictionary look-up (k_tiff.hip k_tiff_lzw_encode, k_gif_lzw.hip k_gif_lzw_encode) into its second probe step, found
by search, and a replay of the look-up that proves they do.

The scheme both encoders state: a dictionary entry is keyed by key = prefix code << 8 | byte; its home slot is (key * 2654435761 mod 2^32) >> 19 of 8192 slots;
a look-up reads the 64 consecutive slots from the home (modulo 8192) in one step, takes the first slot that holds the key, else the first empty one (an absent
key is inserted there), else goes on to the next 64.  Codes start at 258 behind an empty table (TIFF, and GIF at code size 8).  A greedy LZW stream does not
depend on any of this -- which is why only a string built for it reaches the second step: with at most 4096 entries in 8192 slots, 64 occupied slots in a row
from one home do not happen by chance.

The strings: every pair of literal bytes (a, b) is a key below 2^16, eight of them to a slot on average.  The ~128 pairs homed in the 16 slots from H on, inserted
in the order of their homes, pile up in the slots behind H: from about the 74th on they lie 64 or more slots behind their homes, so inserting them is a
two-step miss, and finding them again is a two-step hit.  The parse inserts a pair when it meets it for the first time with a literal in hand, so the string
walks through the pairs, with a detour byte wherever the connecting pair would be an old one; then it names the late pairs once more."""
import functools

SLOTS, WINDOW, MUL = 8192, 64, 2654435761


def home(key):
    return ((key * MUL) & 0xFFFFFFFF) >> 19


def replay(data, limit):
    """the look-ups of a greedy parse of `data` from an empty table whose first free code is 258 and which takes entries while fewer than `limit` codes exist
    (4094: TIFF, 4096: GIF); -> [(found, steps, the windows read crossed slot 8191 / 0)]"""
    tab, nxt, cur, out = {}, 258, data[0], []
    for b in data[1:]:
        key = (cur << 8) | b
        h, steps, wrapped = home(key), 0, False
        while True:
            steps += 1
            assert steps <= SLOTS // WINDOW
            win = [(h + l) % SLOTS for l in range(WINDOW)]
            wrapped |= win[0] > win[-1]
            hit = [s for s in win if s in tab and tab[s][0] == key]
            if hit:
                cur = tab[hit[0]][1]
                out.append((True, steps, wrapped))
                break
            free = [s for s in win if s not in tab]
            if free:
                out.append((False, steps, wrapped))
                if nxt < limit: tab[free[0]] = (key, nxt); nxt += 1
                else: tab, nxt = {}, 258
                cur = b
                break
            h += WINDOW
    return out


@functools.lru_cache(None)
def probe_string(H):
    """a string whose parse piles the ~128 literal pairs homed in slots H .. H + 15 (modulo 8192) up behind H, then looks the last 40 of them up again"""
    homes = [(H + d) % SLOTS for d in range(16)]
    targets = sorted(((a, b) for a in range(256) for b in range(256) if home((a << 8) | b) in homes), key=lambda p: homes.index(home((p[0] << 8) | p[1])))
    assert len(targets) > 2 * WINDOW - 32   # (eight a slot on average)
    out, seen = [], set()

    def literal(x):
        """append x so that it becomes the literal in hand: the pair it closes must be a new one, through a detour byte if need be"""
        if out and (out[-1], x) in seen:
            d = next(d for d in range(256) if (out[-1], d) not in seen and (d, x) not in seen and (out[-1], d) not in targets and (d, x) not in targets and d != out[-1] and d != x)
            seen.add((out[-1], d)); out.append(d)
        if out: seen.add((out[-1], x))
        out.append(x)

    for a, b in targets:
        if (a, b) in seen: continue   # (a connecting pair happened to be this one)
        literal(a); literal(b)
    for a, b in targets[-40:]:        # a: a literal again; a b: found, two steps from its home; then a byte that ends the match
        literal(a)
        out.append(b)
        d = next(d for d in range(256) if (b, d) not in seen and d != a and d != b)   # (cur is a code here: code << 8 | d is a new key wherever it is homed)
        out.append(d)
        seen.add((b, d))              # (not inserted, only kept out of the detours)
    return bytes(out)


FIRST, WRAPPING = 1000, SLOTS - 32   # the second pile lies across slots 8191 / 0


def check(data, limit, wraps):
    """the case means what it says: a present key found in the second step, an absent key placed in the second step; and for the second string, across the wrap"""
    ev = replay(data, limit)
    assert any(found and steps == 2 for found, steps, _ in ev), "no look-up found its key in the second step"
    assert any(not found and steps == 2 for found, steps, _ in ev), "no look-up of an absent key went into the second step"
    if wraps:
        assert any(found and steps == 2 and w for found, steps, w in ev) and any(not found and steps == 2 and w for found, steps, w in ev), "no two-step look-up crossed slots 8191 / 0"
    return ev
