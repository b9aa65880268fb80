"""Time csl_encode_pixels (pixels in device memory -> lossless WebP files) in its coders, in one process: CSH_VP8L=plain (literals only), CSH_VP8L=refs
(backward references and a colour cache), CSH_VP8L=palette (refs, and the colour-indexing transform for pictures of at most 256 colours), CSH_VP8L=groups
(palette, and an entropy image of up to eight groups of prefix codes), CSH_VP8L=far (groups, and a second token set from a match finder over the whole window).
96 pictures of 1920 x 1080 by default: photographic (three textures) and graphic content, repeated.

    python tools/vp8l_refs_time.py [--count 96] [--width 1920] [--height 1080] [--repeats 3] [--once] [--modes plain,refs] [--dithered 0] [--library PATH]

--once: one call per mode after the warm-up (what a kernel trace wants); --modes: the coders to run, the first is what the others are compared with;
--dithered K: K more pictures, texture 5 dithered to 16 colours (Floyd-Steinberg), behind the mix; --library: another build of libcaesium_hip.so (the parent commit's, to compare a mode across commits: `--modes groups,far` in one process gives far
against groups).  Prints one line per call and a summary."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from _util import package
from gen_synth import synth_rgb


class Pixels(C.Structure):
    _fields_ = [("device_pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32)]


def pictures(w, h):
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    flat = np.full((h, w, 3), 250, np.uint8)
    flat[h // 4:h // 2, w // 8:w // 2] = (30, 90, 200)
    flat[h // 3:3 * h // 4, w // 3:7 * w // 8] = (200, 40, 60)
    grad = np.dstack([(x * 255 // (w - 1)) + 0 * y, (y * 255 // (h - 1)) + 0 * x, (x + y) * 255 // (w + h - 2)]).astype(np.uint8)
    return [synth_rgb(1, w, h, texture=20.0), synth_rgb(2, w, h, texture=5.0), synth_rgb(3, w, h, texture=0.0), flat, grad, synth_rgb(4, w, h, texture=10.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=96)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--modes", default="plain,refs")
    ap.add_argument("--dithered", type=int, default=0)
    ap.add_argument("--library", default=None)
    a = ap.parse_args()
    pkg = package()
    api = pkg.CaesiumHip(a.library) if a.library else pkg.load()
    assert api.device_count() >= 1, "no HIP device"
    from caesium_clt_amd.binding import CByteArray, CCSResult
    base = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pictures(a.width, a.height)]
    torch.cuda.synchronize()
    n = a.count + a.dithered
    px = (Pixels * n)()
    if a.dithered:
        from PIL import Image
        d16 = Image.fromarray(synth_rgb(2, a.width, a.height, texture=5.0)).quantize(16, dither=Image.Dither.FLOYDSTEINBERG).convert("RGB")
        dith = torch.from_numpy(np.ascontiguousarray(np.asarray(d16))).cuda()
        torch.cuda.synchronize()
    for i in range(n):
        px[i].device_pixels, px[i].width, px[i].height, px[i].channels = (base[i % len(base)] if i < a.count else dith).data_ptr(), a.width, a.height, 3
    api.L.csl_encode_pixels.argtypes = [C.POINTER(Pixels), C.c_size_t, C.c_int, C.POINTER(CByteArray), C.POINTER(CCSResult)]
    api.L.csl_encode_pixels.restype = C.c_int

    def call(mode):
        os.environ["CSH_VP8L"] = mode
        outs, res = (CByteArray * n)(), (CCSResult * n)()
        t0 = time.perf_counter()
        failed = api.L.csl_encode_pixels(px, n, 0, outs, res)
        dt = time.perf_counter() - t0
        assert failed == 0, [(res[i].code, res[i].error_message) for i in range(n) if not res[i].success][:3]
        sizes = [outs[i].length for i in range(n)]
        for i in range(n):
            api.L.cs_free_bytes(C.byref(outs[i])); api.L.cs_free_result(C.byref(res[i]))
        return dt, sizes
    modes = a.modes.split(",")
    for mode in modes:
        call(mode)   # warm-up: the memory pools, the code objects
    times = {m: [] for m in modes}
    sizes = {}
    for r in range(1 if a.once else a.repeats):
        for mode in modes:
            dt, sizes[mode] = call(mode)
            times[mode].append(dt)
            print("call %d %-7s %8.1f ms  %d bytes" % (r, mode, dt * 1e3, sum(sizes[mode])), flush=True)
    mp = n * a.width * a.height / 1e6
    for mode in modes:
        best = min(times[mode])
        print("%-7s best of %d: %8.1f ms, spread %.1f ms, for %d x %dx%d (%.0f MP/s), %d bytes" % (mode, len(times[mode]), best * 1e3, (max(times[mode]) - best) * 1e3, n, a.width,
                                                                                                    a.height, mp / best, sum(sizes[mode])))
    kinds = list(range(min(len(base), a.count))) + ([a.count] if a.dithered else [])
    for mode in modes[1:]:
        print("%s / %s: time %.2f, bytes %.3f" % (mode, modes[0], min(times[mode]) / min(times[modes[0]]), sum(sizes[mode]) / sum(sizes[modes[0]])))
        print("per picture kind (bytes %s -> %s):" % (modes[0], mode), ", ".join("%d -> %d" % (sizes[modes[0]][i], sizes[mode][i]) for i in kinds))


if __name__ == "__main__":
    main()
