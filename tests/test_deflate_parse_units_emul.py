"""lz_chunk and deep_chunk (png_lz.h, png_parse.h) on the emulation build, called directly on the battery of tests/test_deflate_parse_model.py -- streams no
filtered PNG produces -- and held, stage by stage, to tests/_deflate_parse_model.py: the greedy tokens, the candidates, the last pass's choices and counts, the
tokens at 1, 5 and 15 passes; each between two paddings and over two scratch fills that must not show.  Then two whole files through the emulated product, read
back token by token.  tests/test_zzz_deflate_parse_units_gpu.py has the same bodies on the MI355X, where deep_chunk's candidate search is four real waves."""
import pytest

import _deflate_parse_units as U
import _devunit_cases as DU
from _util import emul_api
from test_deflate_parse_model import NAMES


@pytest.mark.parametrize("name", NAMES)
def test_chunk_functions_follow_the_model(name):
    U.check_entry(DU.emul_lib(), name)


def test_chunk_functions_do_not_depend_on_the_order_of_the_lanes():
    """the emulation runs a launch's lanes in either order (gpu_rt.h csh_emul_reverse)"""
    lib = DU.emul_lib()
    lib.dll.csdu_set_reverse(1)
    try:
        for name in ("words_513", "ten_copies", "period_7"):
            U.check_entry(lib, name)
    finally:
        lib.dll.csdu_set_reverse(0)


def test_entries_refuse_what_the_functions_do_not_take():
    U.check_refusals(DU.emul_lib())


@pytest.mark.parametrize("name", [n for n, _ in U.whole_files()])
def test_whole_file_ships_the_models_tokens(name):
    U.check_whole_file(emul_api(), name)
