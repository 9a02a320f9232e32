"""CPU: k_density (csrc/odr_density.hip.h) bins one entry per lane with the edge arrays in LDS or in memory: no scratch memory in any
of its four instantiations (counts / weighted, edges in LDS / in memory), and no static LDS (the edges take dynamic LDS, sized by
the launch).  DESIGN.md section 8g has the register counts of the build it was written with; the test prints the present ones.
Reads the metadata of the library's gfx950 code object."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')


def test_density_kernels_have_no_scratch():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, 'k_density')
    print(found)
    assert len(found) == 4, 'k_density is not in the library in four instantiations: %s' % found
    for r in found:
        assert r['private_segment_fixed_size'] == 0, r
        assert r['group_segment_fixed_size'] == 0, r
        assert r['vgpr_count'] <= 64, r      # 256 lanes per workgroup, 8 waves per SIMD
