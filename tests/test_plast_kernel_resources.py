"""CPU: the three kernels of csrc/odr_plast.hip.h stream -- one element per thread, the coefficients in the launch arguments: no
scratch memory, no LDS, and few enough vector registers for full occupancy (DESIGN.md section 7j has the counts of the build it was
written with; the test prints the present ones).  Reads the metadata of the library's gfx950 code object, so that an edit that
makes the unrolled Horner chain index its coefficients at run time (scratch) fails here."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
FULL_OCCUPANCY_VGPRS = 64      # 512 vector registers per lane and SIMD, 8 waves


@pytest.mark.parametrize('kernel', ['k_stokes_from_wind', 'k_plast_depth', 'k_plast_check'])
def test_plast_kernels_have_no_scratch_no_lds_and_full_occupancy(kernel):
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, kernel)
    print(kernel, found)
    assert len(found) == 1, found
    r = found[0]
    assert r['private_segment_fixed_size'] == 0 and r['group_segment_fixed_size'] == 0, r
    assert r['vgpr_count'] <= FULL_OCCUPANCY_VGPRS, r
