#!/usr/bin/env python3
"""TIFF inputs through cs_batch_compress with CSH_TIFF set, timed on one device: what profiles/tiff_device_time.txt holds.
64 uncompressed 1024 x 1024 RGB files written by Pillow (16 distinct pictures, each four times), host buffers in -> host buffers out, after a warm-up call of two
files.  Settings: CSH_TIFF=lzw, packbits, and lzw with CSH_TIFF_STRIP 8192 / 65536 / 262144.  Per setting: seconds per call (three calls), output / input bytes, the
per-kernel split of a second cst_batch_run over the same files.  For context -- not as a bound: the device's strips and coder are not libtiff's -- the size of
Pillow / libtiff's own LZW files of the same pictures, with and without Predictor 2.
    python tools/tiff_time.py [--files 64] [--size 1024] [--out profiles/tiff_device_time.txt]"""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _util import package, product_api   # noqa: E402


def pictures(n, size):
    """photograph-like content: smooth shading, edges, a little sensor noise"""
    out = []
    y, x = np.mgrid[0:size, 0:size].astype(np.float32) / size
    for k in range(n):
        rng = np.random.default_rng(100 + k)
        img = np.stack([0.5 + 0.5 * np.sin(6.0 * (x * rng.uniform(0.5, 2) + y * rng.uniform(0.5, 2)) + c + k) for c in range(3)], axis=2)
        for _ in range(12):
            cx, cy, r = rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.03, 0.2)
            img[(x - cx) ** 2 + (y - cy) ** 2 < r * r] = rng.uniform(0, 1, 3)
        img = img * 255 + rng.normal(0, 2.0, img.shape)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def save(arr, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "TIFF", **kw)
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiff_device_time.txt"))
    a = ap.parse_args()
    import PIL
    from PIL import Image
    api = product_api()
    P = package().default_parameters()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    t0 = time.time()
    distinct = pictures(max(1, a.files // 4), a.size)
    blobs = [save(distinct[i % len(distinct)], compression="raw") for i in range(a.files)]
    nin = sum(map(len, blobs))
    say("TIFF inputs through cs_batch_compress with CSH_TIFF set on one MI355X (DESIGN.md 8.4).  Host buffers in -> host buffers out (container walk, upload, kernels,")
    say("download), after one warm-up call of two files.  %d files (%d distinct, Pillow %s, uncompressed RGB), %d x %d; made in %.1f s; input bytes %d"
        % (a.files, len(distinct), PIL.__version__, a.size, a.size, time.time() - t0, nin))
    for pred in (1, 2):
        size = sum(len(save(d, compression="tiff_lzw", tiffinfo={317: pred})) for d in distinct) * (a.files // len(distinct))
        say("for context, libtiff's own LZW files of the same pictures (Pillow, Predictor %d): %d bytes, %.3f of the input" % (pred, size, size / nin))
    os.environ["CSH_TIFF"] = "lzw"
    api.cs_batch_compress(blobs[:2], P)
    for name, strip in (("lzw", None), ("packbits", None), ("lzw", "8192"), ("lzw", "65536"), ("lzw", "262144")):
        os.environ["CSH_TIFF"] = name
        os.environ.pop("CSH_TIFF_STRIP", None)
        if strip:
            os.environ["CSH_TIFF_STRIP"] = strip
        secs, outs = [], None
        for _ in range(3):
            t1 = time.time()
            outs = api.cs_batch_compress(blobs, P)
            secs.append(time.time() - t1)
        failed = sum(isinstance(o, Exception) for o in outs)
        nout = sum(len(o) for o in outs if not isinstance(o, Exception))
        same = np.array_equal(np.array(Image.open(io.BytesIO(outs[0]))), distinct[0]) if not failed else False
        say("CSH_TIFF=%s%s: seconds per call %s | failed %d | output bytes %d | out / in %.3f | file 0 decodes to the input's pixels (Pillow): %s"
            % (name, " CSH_TIFF_STRIP=" + strip if strip else "", " ".join("%.3f" % s for s in secs), failed, nout, nout / nin, same))
        b = api.tiff_batch(blobs, P, name)
        try:
            b.run()
            t = b.run()
        finally:
            b.close()
        say("  cst_batch_run (second run): total %.2f ms; files %d pages %d segments %d passed %d failed %d strip_bytes %d; predictor won on %d pages, lost on %d"
            % (t.total_ms, t.n_files, t.n_pages, t.n_segments, t.n_passed, t.n_failed, t.strip_bytes, t.n_pred_won, t.n_pred_lost))
        for i, kname in enumerate(api.tiff_kernel_names()):
            if t.kernel_ms[i] > 0:
                say("    %-22s %8.3f ms" % (kname, t.kernel_ms[i]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
