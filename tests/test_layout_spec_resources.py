"""CPU: the step launch with the C3 group's static slot layout (k_step_grid<..., LayoutC3>) keeps the registers and the
occupancy of the run-time layout's launch: no scratch memory and <= 96 VGPRs (five waves per SIMD).  A static layout lets the
scheduler mix the burst sampler's gathers (csrc/odr_field.hip.h env_burst), which spilled; this reads the code object's
metadata so that an edit that brings the spill back fails here."""
import os

import pytest

from code_objects import READELF, kernel_resources

SPEC = 'k_step_gridILi2ELi0ELb1ELb0ELi1ENS_8LayoutC3E'


@pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
def test_static_layout_step_kernel_has_no_scratch_and_at_most_96_vgprs():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = [(r['private_segment_fixed_size'], r['vgpr_count']) for r in kernel_resources(_abi.LIB_PATH, SPEC)]
    assert found, 'k_step_grid<..., LayoutC3> is not in the library'
    for scratch, vgpr in found:
        assert scratch == 0 and vgpr <= 96, (scratch, vgpr)
