"""Phase X (the pixel transcode) of a resident batch of 1080p 4:2:0 camera files recompressed to 4:2:2 and to 4:1:1, alternated in one process.

Both go IDCT -> plane -> resample -> FDCT: 4:2:2 through k_resample_plane's per-sample path, 4:1:1 through k_resample_any's vector path.
The 2048 inputs stay resident on the host; batch objects alternate 422, 411, 422, 411 .. (one on the device at a time: two do not fit),
each timed on its second run, so that clocks and caches treat both alike.  Phase X is the library's
phase 1 without the trellis quantiser's slots (as bench.py reports it); the resample + FDCT slot is listed on its own.

    python tools/layout_bench.py [--files 2048] [--rounds 5] [--uniq 64]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from _util import package
from bench import make_inputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--uniq", type=int, default=64)
    a = ap.parse_args()
    pkg = package()
    api = pkg.load()
    names = api.kernel_names()
    uniq = make_inputs(0, a.uniq)
    blobs = [uniq[i % a.uniq] for i in range(a.files)]
    quant = [names.index(n) for n in ("trellis_stats", "k_trellis_ac", "k_trellis_dc")]
    slot = names.index("k_resample+k_plane_fdct")
    res = {ss: [] for ss in (422, 411)}
    for r in range(a.rounds):
        for ss in res:   # two batch objects of 2048 1080p files do not fit the device together: one at a time, the inputs stay resident on the host
            b = api.batch(blobs, pkg.default_parameters(jpeg_quality=80, jpeg_chroma_subsampling=ss))
            b.run()      # warm-up: the first run of a batch object uploads and sizes its pools
            t = b.run()
            b.close()
            api.release_cached_memory()
            x = t.phase_ms[1] - sum(t.kernel_ms[i] for i in quant)
            res[ss].append({"X_ms": round(x, 3), "resample_fdct_ms": round(t.kernel_ms[slot], 3), "total_ms": round(t.total_ms, 3)})
            print(f"round {r} ss={ss} phase X {x:.3f} ms (resample+fdct {t.kernel_ms[slot]:.3f} ms) total {t.total_ms:.2f} ms", flush=True)
    summary = {str(ss): {"X_ms_min": min(v["X_ms"] for v in runs), "X_ms_mean": round(sum(v["X_ms"] for v in runs) / len(runs), 3),
                         "resample_fdct_ms_mean": round(sum(v["resample_fdct_ms"] for v in runs) / len(runs), 3)} for ss, runs in res.items()}
    print(json.dumps({"files": a.files, "rounds": a.rounds, "summary": summary, "runs": {str(k): v for k, v in res.items()}}))


if __name__ == "__main__":
    main()
