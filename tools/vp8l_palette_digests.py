"""Record what CSH_VP8L=palette writes for the palette battery (tests/test_webp_lossless_palette_emul.py pictures()), on the emulation build:

    python tools/vp8l_palette_digests.py [--out tests/golden/vp8l_palette_digests.json]

One sha256 per picture.  tests/test_webp_lossless_groups_emul.py holds the palette coder to them, as tests/golden/vp8l_refs_digests.json holds unset / plain /
refs: run this at the commit whose palette bytes are to be kept, BEFORE the change that must not move them."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_webp_lossless_palette_emul as P
from _util import emul_api


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vp8l_palette_digests.json"))
    a = ap.parse_args()
    outs = P.outputs(emul_api(), "palette")
    digests = {"palette": {name: hashlib.sha256(o).hexdigest() for (name, _, _), o in zip(P.pictures(), outs)}}
    with open(a.out, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(digests["palette"]), a.out))


if __name__ == "__main__":
    main()
