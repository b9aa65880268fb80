"""The inflate catalogue (tests/_inflate_cases.py) through the emulation build of k_png_huff / k_png_lz77 at -o2: stage by stage and file
bytes against the oracle, the decoded rows against the numpy model where the picture is irreducible, the output file against Pillow,
the invalid streams refused.  test_inflate_gpu.py runs the same checks on the device."""
import io

import numpy as np
import pytest

import _deflate as D
import _inflate_cases as IC
from _util import emul_api, package
from oracle import oracle as O
from test_png_emul import check_batch

PIL = pytest.importorskip("PIL.Image")
CS_ERR_BAD_PNG = 30100


@pytest.fixture(scope="module")
def api():
    return emul_api()


def check_catalogue(api, valid, invalid, level=2):
    pkg = package()
    params = pkg.default_parameters(png_optimize=True, png_optimization_level=level)
    # rows, scores, every trial's stream and size, the winner and the file == the oracle's
    check_batch(api, [(c.name, c.png) for c in valid], level)
    b = api.png_batch([c.png for c in valid], params)
    try:
        b.run()
        outs = b.fetch()
        for i, c in enumerate(valid):
            if c.irreducible:   # no reduction: the device's rows are the inflate + unfilter of the stream as they are
                assert O.png_decode(c.png).reduce() == 0, c.name
                assert np.array_equal(b.rows(i), D.unfilter(c.raw, c.width, c.height, c.ctype, c.depth)), c.name
    finally:
        b.close()
    for c, out in zip(valid, outs):
        got, src = PIL.open(io.BytesIO(out)), PIL.open(io.BytesIO(c.png))
        if src.mode == "I;16" and got.mode == "I;16":
            assert np.array_equal(np.asarray(got), D.pillow_view(D.unfilter(c.raw, c.width, c.height, c.ctype, c.depth), c.width, c.height, c.ctype, c.depth)), c.name
        else:
            assert np.array_equal(np.asarray(got.convert("RGBA")), np.asarray(src.convert("RGBA"))), c.name
    # the whole catalogue in one call, and every file on its own: the same bytes
    together = api.cs_batch_compress([c.png for c in valid], params)
    assert together == outs
    for c, out in zip(valid, outs):
        assert api.compress_in_memory(c.png, params) == out, c.name
    bad = api.cs_batch_compress([c.png for c in invalid] + [valid[0].png], params)
    for c, out in zip(invalid, bad):
        assert isinstance(out, Exception) and out.code == CS_ERR_BAD_PNG, (c.name, out)
    assert bad[-1] == outs[0]


def test_emul_inflate_catalogue(api):
    check_catalogue(api, IC.cached_valid(), IC.cached_invalid())
