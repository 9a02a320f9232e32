"""CPU: k_ftle_displacement and k_ftle_cell (csrc/odr_ftle.hip.h) -- one element resp. one cell per lane, no LDS tile: no scratch
memory and no static LDS in either.  DESIGN.md section 8h has the register counts of the build it was written with; the test prints
the present ones.  Reads the metadata of the library's gfx950 code object."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')


@pytest.mark.parametrize('kernel', ['k_ftle_displacement', 'k_ftle_cell'])
def test_ftle_kernels_have_no_scratch(kernel):
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, kernel)
    print(found)
    assert len(found) == 1, '%s is not in the library exactly once: %s' % (kernel, found)
    r = found[0]
    assert r['private_segment_fixed_size'] == 0, r
    assert r['group_segment_fixed_size'] == 0, r
    assert r['vgpr_count'] <= 128, r      # 256 lanes per workgroup: at least 4 waves per SIMD
