"""CPU: the kernels of csrc/odr_schism.hip.h keep the stack-free k-d tree walk, the best three of a search (three distances, three
indices and three levels in named scalars), the weights of up to three searches and the values of up to eight variables in
registers: no scratch memory and no LDS.  DESIGN.md section 8p has the register counts of the build it was written with; the test
prints the present ones.  Reads the metadata of the library's gfx950 code object."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')

LDS = {'k_schism_nearest3': 0, 'k_schism_sample': 0}


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
