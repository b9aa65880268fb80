"""The size table of CSH_VP8L=groups: every picture of the groups battery (tests/test_webp_lossless_groups_emul.py) and a few larger ones from
the refs battery, coded by the emulation build in every mode, against libwebp (Pillow lossless=True, quality=75, method=4).

    python tools/vp8l_groups_sizes.py > profiles/r09_vp8l_groups_sizes.txt

The device writes the same bytes (tests/test_zzz_webp_lossless_groups_gpu.py), so the sizes are the product's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _vp8l_parse as V
import test_webp_lossless_emul as E
import test_webp_lossless_groups_emul as G
import test_webp_lossless_refs_emul as R
from _util import emul_api

MORE = ["w0.webp", "texture0", "texture0_640x480", "gradient", "rgba", "grey_alpha"]   # of the refs battery


def main():
    api = emul_api()
    rows = [(n, s) for (n, _), s in zip(G.pictures(), G.sources())] + [(n, s) for n, s in R.battery() if n in MORE]
    sizes = {}
    for mode in ("plain", "refs", "palette", "groups"):
        with G.vp8l_mode(mode):
            sizes[mode] = api.cs_batch_compress([s for _, s in rows], E.params(webp_lossless=True))
    print("%-20s %9s %9s %9s %9s %9s  %-15s %-14s %s" % ("picture", "plain", "refs", "palette", "groups", "libwebp", "groups/palette", "groups/libwebp", "groups in the stream"))
    for k, (name, src) in enumerate(rows):
        pl, rf, pa, gr = (sizes[m][k] for m in ("plain", "refs", "palette", "groups"))
        st = V.parse(gr)
        lw = R.libwebp_size(src)
        print("%-20s %9d %9d %9d %9d %9d  %-15.4f %-14.3f %s" % (name, len(pl), len(rf), len(pa), len(gr), lw, len(gr) / len(pa), len(gr) / lw, "yes" if st.meta_prefix else "-"))


if __name__ == "__main__":
    main()
