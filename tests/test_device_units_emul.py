"""The device units (tests/devunit/, tests/_devunit_cases.py) on the emulation build of the unit library: every function's CSH_EMUL branch against the battery's
expected values.  It is the proof, where no GPU is, that the battery and its expected values are right; tests/test_device_units_gpu.py puts the device
branches through the same battery."""
import pytest

import _devunit_cases as DU


@pytest.mark.parametrize("unit", list(DU.UNITS))
def test_unit(unit):
    DU.UNITS[unit](DU.emul_lib())


def test_units_do_not_depend_on_the_order_of_the_lanes():
    """the emulation runs a launch's lanes in either order (gpu_rt.h csh_emul_reverse); a block function or a wave helper must not notice"""
    lib = DU.emul_lib()
    lib.dll.csdu_set_reverse(1)
    try:
        for unit in ("dering-1-256", "fdct-2-64", "lscan-256", "LeReader-256", "wave_incl_scan-256", "gen_tables-5", "code_lengths-19-7", "code_lengths_wide-536"):
            DU.UNITS[unit](lib)
    finally:
        lib.dll.csdu_set_reverse(0)
