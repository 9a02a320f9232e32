"""CPU: the step launch with the C3 group's static slot layout on a step whose time sits on a reader level
(k_step_grid<..., LayoutC3L1>) keeps the registers and the occupancy of the two-level launch: no scratch memory and <= 96
VGPRs (five waves per SIMD).  Its burst gathers slot A at two levels and the other slots at one (csrc/odr_field.hip.h
env_burst); this reads the code object's metadata so that an edit that makes it spill fails here."""
import os

import pytest

from code_objects import OBJCOPY, READELF, kernel_resources

SPEC = 'k_step_gridILi2ELi0ELb1ELb0ELi1ENS_10LayoutC3L1E'


@pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJCOPY)), reason='needs the ROCm LLVM tools')
def test_onlevel_layout_step_kernel_does_not_spill():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = [(r['private_segment_fixed_size'], r['vgpr_count']) for r in kernel_resources(_abi.LIB_PATH, SPEC)]
    assert found, 'k_step_grid<..., LayoutC3L1> is not in the library'
    for scratch, vgpr in found:
        assert scratch == 0 and vgpr <= 96, (scratch, vgpr)
