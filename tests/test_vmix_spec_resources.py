"""CPU: the mixing launch with C3's static configuration (k_vmix_col<NQ, TL, VMixC3>, both level counts of C3's field, both
time-level cases) keeps the occupancy of the run-time configuration's launch: no scratch memory and <= 80 VGPRs (six waves per
SIMD, ODR_VMIX_WAVES).  Without the fences between the column's quads (csrc/odr_kernels.hip.h vmix_col_fill) the 8-level column
with two time levels spilled; this reads the code object's metadata so that an edit that brings the spill back fails here."""
import os

import pytest

from code_objects import READELF, kernel_resources

SPEC = ['k_vmix_colILi%dELb%dENS_6VMixC3E' % (nq, tl) for nq in (2, 3) for tl in (0, 1)]


@pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
def test_static_mixing_kernels_do_not_spill():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = {}
    for spec in SPEC:
        for r in kernel_resources(_abi.LIB_PATH, spec):
            found[spec] = (r['private_segment_fixed_size'], r['vgpr_count'])
    assert sorted(found) == sorted(SPEC), found
    for spec, (scratch, vgpr) in found.items():
        assert scratch == 0 and vgpr <= 80, (spec, scratch, vgpr)
