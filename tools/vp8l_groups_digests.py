"""Record what CSH_VP8L=groups writes for the refs, palette and groups batteries (tests/test_webp_lossless_refs_emul.py battery(),
tests/test_webp_lossless_palette_emul.py pictures(), tests/test_webp_lossless_groups_emul.py pictures()), on the emulation build:

    python tools/vp8l_groups_digests.py [--out tests/golden/vp8l_groups_digests.json]

One sha256 per picture, under the battery's name.  tests/test_webp_lossless_far_emul.py holds the groups coder to them, as tests/golden/vp8l_refs_digests.json
holds unset / plain / refs and tests/golden/vp8l_palette_digests.json holds palette: run this at the commit whose groups bytes are to be kept, BEFORE the change
that must not move them."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_webp_lossless_groups_emul as G
import test_webp_lossless_palette_emul as P
import test_webp_lossless_refs_emul as R
from _util import emul_api


def digests_of(api):
    """{battery: {picture: sha256 of its groups file}}"""
    sha = lambda o: hashlib.sha256(o).hexdigest()
    return {"refs": {n: sha(o) for (n, _), o in zip(R.battery(), R.outputs(api, "groups"))},
            "palette": {n: sha(o) for (n, _, _), o in zip(P.pictures(), P.outputs(api, "groups"))},
            "groups": {n: sha(o) for (n, _), o in zip(G.pictures(), G.outputs(api, "groups"))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vp8l_groups_digests.json"))
    a = ap.parse_args()
    digests = digests_of(emul_api())
    with open(a.out, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s digests -> %s" % (" + ".join(str(len(v)) for v in digests.values()), a.out))


if __name__ == "__main__":
    main()
