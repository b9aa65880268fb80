"""The device units (tests/devunit/, tests/_devunit_cases.py) on the MI355X: the product-build branch of every CSH_EMUL conditional in the kernels' helpers --
the inline-asm v_dot2 transform, the DPP ladders, the readlane windows of the bit readers, the v_perm selectors, v_alignbyte, the ballot exit of the deringing --
function by function against the battery tests/test_device_units_emul.py proves on the emulation build.  A wrong primitive is named here, in front of the
whole-file parity tests that would only show a file differing from the oracle's.  A missing library or no device FAILS: nothing here skips."""
import pytest

import _devunit_cases as DU

pytestmark = pytest.mark.gpu


def test_the_unit_library_is_the_device_build_and_sees_a_device():
    assert not DU.device_lib().emul


@pytest.mark.parametrize("unit", list(DU.UNITS))
def test_unit(unit):
    DU.UNITS[unit](DU.device_lib())
