"""A plain `bench.py` run on the device: it times the steps it is given, checks nothing itself, and what --dump-outputs writes is what the
last timed step made -- the oracle's files for the same inputs."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from _util import ROOT, oracle_lossy

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_its_last_step(tmp_path):
    import bench
    d = tmp_path / "out"
    batch, unique = 48, 6
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(batch), "--unique", str(unique),
                        "--dump-outputs", str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "MP/s" and line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["parity_spot_check"] is None and line["parity_files_checked"] == 0 and line["cpu_baseline"] is None
    lengths, crc = np.load(d / "lengths.npy"), np.load(d / "crc32.npy")
    assert len(lengths) == len(crc) == batch
    expected = {k: oracle_lossy(bench._one_input(k)) for k in range(unique)}
    for i in range(batch):
        assert (lengths[i], crc[i]) == (len(expected[i % unique]), zlib.crc32(expected[i % unique])), i
    files = sorted(d.glob("file_*.npy"))
    assert len(files) == bench.DUMP_FILES
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float32 and bytes(a.astype(np.uint8)) == expected[int(f.name[5:10]) % unique][:bench.DUMP_FILE_BYTES]
