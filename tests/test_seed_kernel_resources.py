"""CPU: the kernels of csrc/odr_seed.hip.h keep the inverse projection, the crossing rule and the geodesic solves in registers:
no scratch memory.  k_pip_points has exactly one tile of 256 ring vertices (x and y, float64) in LDS, k_seed_edges that tile and
its four wave counts, k_seed_scan its double-buffered 256 partial sums; k_seed_compact, k_npts_line and k_npts_points none.  DESIGN.md
section 8j has the register counts of the build it was written with; the test prints the present ones.  Reads the metadata of the
library's gfx950 code object."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')

LDS = {'k_pip_points': 2 * 256 * 8, 'k_seed_edges': 2 * 256 * 8 + 4 * 4, 'k_seed_scan': 2 * 256 * 4, 'k_seed_compact': 0,
       'k_npts_line': 0, 'k_npts_points': 0}


@pytest.mark.parametrize('kernel', sorted(LDS))
def test_no_scratch_and_the_designed_lds(kernel):
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, kernel)
    print(found)
    assert len(found) == 1, '%s is not in the library exactly once: %s' % (kernel, found)
    assert found[0]['private_segment_fixed_size'] == 0, found
    assert found[0]['group_segment_fixed_size'] == LDS[kernel], found
    assert found[0]['vgpr_count'] <= 256, found      # 256 lanes per workgroup: one workgroup per SIMD quad must fit
