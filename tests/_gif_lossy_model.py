"""The lossy GIF route's model (CSH_GIF=lossy): _gif_model's output rule with the coder replaced, and nothing else.  D = 100 - quality; two
table colours are near when their squared RGB distance is at most D * D; with prefix code cur and next pixel b the coder walks cand(b) = [b] + near(b) and lets
the first candidate c with (cur, c) in the dictionary extend the match (the decoder shows c); with none it sends cur and adds (cur, b), the exact pixel.
Rectangles, disposals, the pixels PACK writes (which are transparent among them), tables, heads, chunking, fallbacks: _gif_model.optimise as it stands."""
import numpy as np

import _gif_model as M

ROW = 64


def distance(quality):
    """D: the quality is held to 1..100 (0 counts as 1, as in libcaesium)"""
    return 100 - min(100, max(1, int(quality)))


def _rgb(word):
    return int(word) & 255, (int(word) >> 8) & 255, (int(word) >> 16) & 255


def dist2(a, b):
    return sum((x - y) ** 2 for x, y in zip(_rgb(a), _rgb(b)))


def near_lists(table, n, D):
    """-> cand: 256 lists.  cand[b] = [b] + the canonical indices c != b below n (no lower index holds c's colour) whose colour is near b's, by (distance^2,
    index), the first 63 of them -- for a canonical b below n; every other b stands alone.  No transparent index plays a part: the list belongs to the table"""
    canonical = [i < n and all(int(table[j]) != int(table[i]) for j in range(i)) for i in range(256)]
    cand = []
    for b in range(256):
        near = []
        if canonical[b] and D > 0:
            near = sorted((dist2(table[c], table[b]), c) for c in range(n) if c != b and canonical[c] and dist2(table[c], table[b]) <= D * D)[:ROW - 1]
        cand.append([b] + [c for _, c in near])
    return cand


def near_arrays(cand):
    """the lists as the device's tap gives them: rows [256][64] padded with 0, counts [256]"""
    rows, count = np.zeros((256, ROW), dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    for b, lst in enumerate(cand):
        rows[b, :len(lst)] = lst
        count[b] = len(lst)
    return rows, count


def encode_chunks(px, mcs, chunk, cand, transparent, n, tally=None):
    """_gif_model.encode_chunks with the candidate walk in front of the dictionary look-up; cand of single entries (D = 0) is that coder bit for bit.
    tally: a dict that counts "clears" (clear codes behind a code sent with a full table) and "shown" (the indices the decoder will show, in order)"""
    clear = 1 << mcs
    acc = nb = 0
    out = bytearray()
    shown = []
    nclears = 0

    def put(code, width):
        nonlocal acc, nb
        acc |= code << nb; nb += width
        while nb >= 8:
            out.append(acc & 255); acc >>= 8; nb -= 8

    put(clear, mcs + 1)
    nchunks = (len(px) + chunk - 1) // chunk
    for c in range(nchunks):
        part = [int(v) for v in px[c * chunk:(c + 1) * chunk]]
        table, nxt, width = {}, clear + 2, mcs + 1
        cur = part[0]
        shown.append(cur)
        for b in part[1:] + [None]:
            if b is not None:
                walk = [b] if (b == transparent or b >= n) else [v for v in cand[b] if v == b or v != transparent]
                hit = next((v for v in walk if (cur, v) in table), None)
                if hit is not None:
                    cur = table[(cur, hit)]
                    shown.append(hit)
                    continue
            put(cur, width)
            if nxt < 4096:
                if b is not None:
                    table[(cur, b)] = nxt
                nxt += 1
                if nxt > (1 << width) and width < 12:
                    width += 1
            else:
                put(clear, width)
                nclears += 1
                table, nxt, width = {}, clear + 2, mcs + 1
            cur = b
            if b is not None:
                shown.append(b)
        put(clear + 1 if c == nchunks - 1 else clear, width)
    if nb:
        out.append(acc & 255)
    if tally is not None:
        tally["clears"] = tally.get("clears", 0) + nclears
        tally.setdefault("shown", []).append(shown)
    return bytes(out)


def optimise(blob, chunk, quality, keep_metadata=False, tally=None):
    """_gif_model.optimise with its coder replaced: -> (the file, None) or (None, the fallback raised)"""
    g = M.parse(blob)
    D = distance(quality)
    frames = iter(g["frames"])
    lists = {}

    def coder(px, mcs, chunk_px):
        f = next(frames)   # optimise codes the frames in order, once each
        table, n = M.colour_table(g, f)
        key = f["lct"] or g["gct"]
        if key not in lists:
            lists[key] = near_lists(table, n, D)
        return encode_chunks(px, mcs, chunk_px, lists[key], f["transparent"], n, tally)

    saved = M.encode_chunks
    M.encode_chunks = coder
    try:
        return M.optimise(blob, chunk, keep_metadata)
    finally:
        M.encode_chunks = saved


def frame_lists(blob, frame, quality):
    """the candidate lists of the table that frame `frame` uses"""
    g = M.parse(blob)
    table, n = M.colour_table(g, g["frames"][frame])
    return near_lists(table, n, distance(quality))
