"""The size table of CSH_VP8L=far: every picture of the far battery (tests/test_webp_lossless_far_emul.py), a page of glyphs over a column
gradient and the larger pictures of the refs battery, coded by the emulation build in every mode, against libwebp (Pillow lossless=True, quality=75, method=4).

    python tools/vp8l_far_sizes.py > profiles/r10_vp8l_far_sizes.txt

The last column names the token set the picture kept: `far` where the file differs from the groups mode's (the second set replaces the first only where its
stream is strictly smaller, so a file that kept the first set IS the groups file), with the pixels its copies take from beyond the reach of CSH_VP8L=refs' own
finder (16 384 positions).  The device writes the same bytes (tests/test_zzz_webp_lossless_far_gpu.py), so the sizes are the product's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
from PIL import Image, ImageDraw

import _vp8l_parse as V
import test_webp_lossless_emul as E
import test_webp_lossless_far_emul as F
import test_webp_lossless_refs_emul as R
from _util import emul_api

MORE = ["w0.webp", "texture0", "texture0_640x480", "gradient", "rgba", "grey_alpha", "far_repeat"]   # of the refs battery
SLOW_READ = ["edge_out", "edge_one", "far_repeat"]   # 1.5 M and 1 M pixels of noise: the pure-Python reader is not asked for their copies
MODES = ("plain", "refs", "palette", "groups", "far")


def glyph_page(w=320, h=240):
    """12 rows of 8 glyph cells (Pillow's built-in font) over a gradient that changes with the column only: a cell's text depends on its column and on its row
    modulo 4, so every cell comes back 4 rows of cells = 76 picture rows = 24 320 positions lower, beyond the reach of CSH_VP8L=refs' finder"""
    x = np.arange(w)[None, :] + np.zeros((h, 1), int)
    im = Image.fromarray(np.dstack([200 + x * 40 // w, 210 + x * 30 // w, 190 + x * 60 // w]).astype(np.uint8))
    d = ImageDraw.Draw(im)
    names = "ABCDEFGHIJKLMNOPQRSTUVWXYZ012345"
    for row in range(12):
        for col in range(8):
            k = (row % 4) * 8 + col
            d.text((8 + 38 * col, 6 + 19 * row), names[k] + names[k].lower() + names[31 - k], fill=(20, 20, 30))
    return np.asarray(im)


def main():
    api = emul_api()
    rows = [(n, s) for (n, _), s in zip(F.pictures(), F.sources())] + [("glyph_page", F.source_of(glyph_page()))] + [(n, s) for n, s in R.battery() if n in MORE]
    sizes = {}
    for mode in MODES:
        with F.vp8l_mode(mode):
            sizes[mode] = api.cs_batch_compress([s for _, s in rows], E.params(webp_lossless=True))
    print("%-18s %9s %9s %9s %9s %9s %9s  %-10s %-11s %s" % ("picture", "plain", "refs", "palette", "groups", "far", "libwebp", "far/groups", "far/libwebp", "token set kept"))
    for k, (name, src) in enumerate(rows):
        out = [sizes[m][k] for m in MODES]
        gr, fa = out[3], out[4]
        lw = R.libwebp_size(src)
        kept = "first (the groups file)" if fa == gr else "far"
        if fa != gr and name not in SLOW_READ:
            kept += ", %d pixels copied from beyond 16384" % sum(l for l, d, _ in V.parse(fa).refs if d > 16384)
        print("%-18s %9d %9d %9d %9d %9d %9d  %-10.4f %-11.3f %s" % ((name,) + tuple(len(o) for o in out) + (lw, len(fa) / len(gr), len(fa) / lw, kept)))


if __name__ == "__main__":
    main()
