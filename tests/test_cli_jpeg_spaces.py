"""A folder from a print workflow through the caesiumclt shell: one CMYK file among YCbCr ones comes back compressed with the rest (emulation build;
the `gpu` case runs the product binary)."""
import json
import os

import pytest

import _jpeg_spaces as S
from _util import emul_api, oracle_lossy
from gen_synth import synth_jpeg
from test_cli import EMUL_CLI, PRODUCT_CLI, run_cli


def tree_with_cmyk(binary, tmp_path):
    root = tmp_path / "print"
    (root / "plates").mkdir(parents=True)
    files = {"cover.jpg": synth_jpeg(61, 120, 80, texture=20), "plates/sheet_cmyk.jpg": S.pillow_cmyk(62, 97, 61), "plates/proof.jpg": synth_jpeg(63, 64, 96, subsampling=0, texture=12)}
    for rel, data in files.items():
        (root / rel).write_bytes(data)
    out = tmp_path / "out"
    r = run_cli(binary, "-q", 80, "-o", out, "-R", "-S", "--json", root)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    assert sorted(os.path.relpath(f["original_path"], root) for f in j["files"]) == sorted(files)
    assert [f["status"] for f in j["files"]] == ["success"] * 3, [f.get("message") for f in j["files"]]
    for f in j["files"]:
        rel = os.path.relpath(f["original_path"], root)
        data = open(f["output_path"], "rb").read()
        assert f["compressed_size"] == len(data)
        if "cmyk" in rel:
            fr = S.frame(data)
            assert bytes(c[0] for c in fr["comps"]) == b"CMYK" and fr["adobe"] == 0 and not fr["jfif"] and len(data) < len(files[rel])
        else:
            assert data == oracle_lossy(files[rel], 80)


def test_cmyk_among_ycbcr_emulated(tmp_path):
    emul_api()
    tree_with_cmyk(EMUL_CLI, tmp_path)


@pytest.mark.gpu
def test_cmyk_among_ycbcr_on_device(tmp_path):
    assert os.path.exists(PRODUCT_CLI), "caesium-clt_amd/bin/caesiumclt is not built"
    tree_with_cmyk(PRODUCT_CLI, tmp_path)
