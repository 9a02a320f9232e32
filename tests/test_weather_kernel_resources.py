"""CPU: the kernels of the NOAA oil weathering (csrc/odr_weather.hip) use no scratch memory -- the element's record is 14 float64
registers, the row of mass_components is read and written in place, the eight partial sums of NumPy's pairwise order are scalars --
and their LDS is what the source declares: the component constants and the step's reduction in k_weather (4 * 32 + 8 float64),
one 8-vector per lane in the folds.  DESIGN.md section 7i has the register counts of the build it was written with; the test
prints the present ones.  Reads the metadata of the library's gfx950 code object."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
FOLD_LDS = 256 * 8 * 8
# label -> (what its mangled name contains, static LDS in bytes); k_weather_fold has one instantiation per fold, flags and sums
KERNELS = {'k_weather': ('9k_weatherx', (4 * 32 + 8) * 8), 'k_weather_reduce': ('k_weather_reduce', FOLD_LDS),
           'k_weather_budget': ('k_weather_budget', FOLD_LDS), 'k_weather_fold': ('k_weather_fold', FOLD_LDS)}


@pytest.mark.parametrize('kernel', sorted(KERNELS))
def test_weather_kernels_have_no_scratch(kernel):
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    mangled, lds = KERNELS[kernel]
    found = kernel_resources(_abi.LIB_PATH, mangled)
    print(kernel, found)
    assert len(found) == (2 if kernel == 'k_weather_fold' else 1), found
    for r in found:
        assert r['private_segment_fixed_size'] == 0, r
        assert r['group_segment_fixed_size'] == lds, r
        assert r['vgpr_count'] <= 128, r      # 256 lanes per workgroup: at least 4 waves per SIMD
