"""lz_chunk and deep_chunk (png_lz.h, png_parse.h) on the MI355X, called directly: the device-only shape of deep_chunk -- four waves that share three LDS tables
across workgroup barriers, deep_last_lanes on borrowed S.hist words, candidates written by four waves and read back by the first behind one fence, the 16-wide
register window of the path and its look-ups in the scratch area -- on the battery of tests/test_deflate_parse_model.py, held stage by stage to
tests/_deflate_parse_model.py.  The bodies are those of tests/test_deflate_parse_units_emul.py.  A missing library or no device FAILS: nothing here skips."""
import pytest

import _deflate_parse_units as U
import _devunit_cases as DU
from _util import product_api
from test_deflate_parse_model import NAMES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", NAMES)
def test_chunk_functions_follow_the_model(name):
    U.check_entry(DU.device_lib(), name)


def test_entries_refuse_what_the_functions_do_not_take():
    U.check_refusals(DU.device_lib())


@pytest.mark.parametrize("name", [n for n, _ in U.whole_files()])
def test_whole_file_ships_the_models_tokens(name):
    U.check_whole_file(product_api(), name)
