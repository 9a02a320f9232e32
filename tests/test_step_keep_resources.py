"""CPU: the keep ballots the static-layout step launches form for the dense mixing launch (StepDesc.keep, csrc/odr_kernels.hip.h:
one compare, two ballots and two lane-0 stores at the sea-floor clause) cost the step kernel nothing it is held to -- no scratch
memory, and no more VGPRs than the launch had before it formed them (96 for both static layouts: five waves per SIMD) -- and the
three list kernels, which now read wave counts either producer wrote, still use no scratch memory.  Read from the code object's
metadata."""
import os

import pytest

from code_objects import OBJCOPY, READELF, kernel_resources

# k_step_grid<RK4, lat / lon, 3-D, no noise, FAST stage arithmetic, LY>: every instantiation with a static layout
STATIC_STEP = ('k_step_gridILi2ELi0ELb1ELb0ELi1ENS_8LayoutC3E', 'k_step_gridILi2ELi0ELb1ELb0ELi1ENS_10LayoutC3L1E')
VGPR_BEFORE = 96     # vgpr_count of either kernel in the library of the commit before the ballots
LIST_KERNELS = ('11k_vmix_keepE', '16k_vmix_keep_scanE', '16k_vmix_keep_fillE')

needs_tools = pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJCOPY)), reason='needs the ROCm LLVM tools')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    return _abi.LIB_PATH


@needs_tools
def test_no_other_step_kernel_has_a_static_layout(lib):
    """the bound below covers every instantiation that carries the code"""
    from code_objects import _named_blocks
    static = sorted(k for k, _ in _named_blocks(lib) if 'k_step_grid' in k and 'LayoutC3' in k)
    assert len(static) == len(STATIC_STEP) and all(any(s in k for k in static) for s in STATIC_STEP), static


@needs_tools
@pytest.mark.parametrize('name', STATIC_STEP)
def test_static_layout_step_kernels_keep_their_registers(lib, name):
    found = kernel_resources(lib, name)
    assert len(found) == 1, (name, len(found))
    assert found[0]['private_segment_fixed_size'] == 0 and found[0]['vgpr_count'] <= VGPR_BEFORE, found[0]


@needs_tools
@pytest.mark.parametrize('name', LIST_KERNELS)
def test_list_kernels_use_no_scratch(lib, name):
    found = kernel_resources(lib, name)
    assert len(found) == 1, (name, len(found))
    assert found[0]['private_segment_fixed_size'] == 0, found[0]
