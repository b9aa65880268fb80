"""The link stage and the finder of CSH_VP8L=far on the MI355X: the cases of tests/test_vp8l_far_units_emul.py through the device build of
tests/devunit/du_vp8l_far.cpp, against the same model values, exactly.  A missing library or no device FAILS: nothing here skips."""
import pytest

import test_vp8l_far_units_emul as U
from _devunit_cases import device_lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", U.CASES)
def test_far_unit(name):
    U.run_case(device_lib(), name)


def test_far_unit_refuses_what_the_coder_would():
    U.run_refusals(device_lib())
