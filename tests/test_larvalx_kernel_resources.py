"""CPU: the kernels of csrc/odr_larvalx.hip.h are streaming kernels, one element per lane: no scratch memory and no LDS -- the
float64 sin, cos and arcsin of the solar elevation included (their argument reduction must not index a private table).  Reads the
metadata of the library's gfx950 code object."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    return _abi.LIB_PATH


@pytest.mark.parametrize('kernel', ['k_larvalx_hatch', 'k_larvalx_behave', 'k_solar_elevation'])
def test_larvalx_kernels_have_no_scratch_and_no_lds(lib, kernel):
    found = kernel_resources(lib, kernel)
    print(kernel, found)
    assert len(found) == 1, '%s is not in the library exactly once: %s' % (kernel, found)
    assert found[0]['private_segment_fixed_size'] == 0, found
    assert found[0]['group_segment_fixed_size'] == 0, found
