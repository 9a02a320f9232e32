"""CPU: the kernels of csrc/odr_conc.hip.h in the library's gfx950 code object: each once per instantiation -- k_conc_bin in six (masks
/ weighted masks / species, edges in LDS / in memory), k_conc_extent and k_conc_grid in one, k_conc_box in two (rows, columns) -- with no
scratch memory and no static LDS (edges, layer bounds and the per-wave extremes take dynamic LDS, sized by the launch).  DESIGN.md
section 8m has the register counts of the build it was written with; the test prints the present ones."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')


@pytest.mark.parametrize('kernel,instantiations', [('k_conc_bin', 6), ('k_conc_extent', 1), ('k_conc_grid', 1), ('k_conc_box', 2)])
def test_conc_kernels_have_no_scratch_and_no_static_lds(kernel, instantiations):
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, kernel)
    print(found)
    assert len(found) == instantiations, '%s is in the library in %d instantiations, not %d' % (kernel, len(found), instantiations)
    for r in found:
        assert r['private_segment_fixed_size'] == 0, r
        assert r['group_segment_fixed_size'] == 0, r


def test_the_bin_kernel_stays_within_128_registers():
    """256 lanes per workgroup; the projections of odr_field.hip.h are inlined into it: at most 128 registers (4 waves per SIMD)."""
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    for r in kernel_resources(_abi.LIB_PATH, 'k_conc_bin'):
        assert r['vgpr_count'] <= 128, r
