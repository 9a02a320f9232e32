"""CPU: the kernels of csrc/odr_radio.hip.h use no scratch memory -- the row of the rate table is read from LDS with a fully unrolled
loop over the compile-time maximum of seven species, the probabilities stay in registers -- and the speciation launch stages exactly
its table and histogram in LDS.  Reads the metadata of the library's gfx950 code object, so that an edit that indexes a private
array dynamically fails here.  Of the kernels that gained the species-aware sea-floor action, k_vbuoy and k_vmix_wind stay without
scratch and the statically configured C3 launches are untouched (test_layout_spec_resources.py); the run-time configurations of
k_vmix_col / k_vmix_win spilled 16 - 36 bytes in some instantiations before the action was added and still do."""
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


@pytest.mark.parametrize('kernel,lds', [('k_radio_speciation', 4 * 49 * 8 + 50 * 4), ('k_radio_terminal_velocity', 0),
                                        ('k_radio_resuspend', 50 * 4)])
def test_radio_kernels_have_no_scratch(lib, kernel, lds):
    found = kernel_resources(lib, kernel)
    print(kernel, found)
    assert len(found) == 1, '%s is not in the library exactly once: %s' % (kernel, found)
    assert found[0]['private_segment_fixed_size'] == 0, found
    assert found[0]['group_segment_fixed_size'] == lds, found


@pytest.mark.parametrize('kernel', ['k_vbuoy', 'k_vmix_wind', 'VMixC3'])
def test_kernels_with_the_species_action_have_no_scratch(lib, kernel):
    found = kernel_resources(lib, kernel)
    print(kernel, found)
    assert found, kernel
    for r in found:
        assert r['private_segment_fixed_size'] == 0, (kernel, r)
