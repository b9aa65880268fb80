"""bench.py's host side: the inputs it makes are the SURVEY 8d recipe's files bit for bit (gen_synth.synth_rgb_fast == synth_rgb), what
--dump-outputs writes, and the arguments a run refuses."""
import os
import subprocess
import sys
import zlib

import numpy as np

from _util import ROOT
from gen_synth import synth_jpeg, synth_rgb, synth_rgb_fast


def test_fast_pictures_are_the_recipes():
    for i, (w, h) in [(0, (1920, 1080)), (999, (1920, 1080)), (1000, (1920, 1080)), (3, (320, 240)), (4, (161, 97)), (5, (1, 1))]:
        assert np.array_equal(synth_rgb_fast(i, w, h), synth_rgb(i, w, h)), (i, w, h)


def test_bench_inputs_are_synth_jpeg():
    import bench
    assert bench._one_input(7) == synth_jpeg(7)


def test_dump_outputs_writes_lengths_crcs_and_a_fixed_sample(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    outs = [bytes(rng.integers(0, 256, int(n), dtype=np.uint8)) for n in rng.integers(1, 3 << 20, 40)]
    outs[5] = RuntimeError("a failed file")
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    lengths, crc = np.load(tmp_path / "a" / "lengths.npy"), np.load(tmp_path / "a" / "crc32.npy")
    assert lengths.dtype == np.float64 and crc.dtype == np.float64 and len(lengths) == len(crc) == len(outs)
    for i, o in enumerate(outs):
        assert (lengths[i], crc[i]) == ((-1, -1) if i == 5 else (len(o), zlib.crc32(o)))
    names = sorted(p.name for p in (tmp_path / "a").glob("file_*.npy"))
    assert len(names) == bench.DUMP_FILES and names == sorted(p.name for p in (tmp_path / "b").glob("file_*.npy"))
    for name in names:
        i = int(name[5:10])
        a = np.load(tmp_path / "a" / name)
        assert a.dtype == np.float32 and np.array_equal(a, np.load(tmp_path / "b" / name))
        assert bytes(a.astype(np.uint8)) == (b"" if i == 5 else outs[i][:bench.DUMP_FILE_BYTES])
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64 << 20


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 2 and b"--steps must be at least 1" in r.stderr
