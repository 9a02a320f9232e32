"""CPU: k_blk_convolve and k_blk_convolve_zy (csrc/odr_convolve.hip.h), the convolution pass of the level preparation -- no scratch
memory in either (the accumulators and the strip of loaded values are indexed by unrolled loops only, the weights are read from the
kernel arguments), the staged region of the 2-D kernel within a workgroup's LDS, none in the 3-D kernel.  DESIGN.md section 4.4a has
the register counts of the build it was written with; the test prints the present ones.  Reads the metadata of the library's gfx950
code object."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')

LDS_PER_WORKGROUP = 64 * 1024      # what one workgroup may declare statically
REGION_BYTES = 4 * 46 * 46         # (CONV_T + CONV_MAX - 1)^2 floats


@pytest.mark.parametrize('kernel,lds', [('14k_blk_convolveE', REGION_BYTES), ('17k_blk_convolve_zyE', 0)])
def test_convolution_kernels_have_no_scratch(kernel, lds):
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, kernel)
    print(found)
    assert len(found) == 1, '%s is not in the library exactly once: %s' % (kernel, found)
    r = found[0]
    assert r['private_segment_fixed_size'] == 0, r
    assert r['group_segment_fixed_size'] == lds and lds <= LDS_PER_WORKGROUP, r
    assert r['vgpr_count'] <= 64, r      # 256 lanes per workgroup: eight waves per SIMD
