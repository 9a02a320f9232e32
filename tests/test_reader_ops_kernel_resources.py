"""CPU: k_combined_sample (csrc/odr_combine.hip.h) in the library's gfx950 code object: once, no scratch memory, no LDS, at most 256
VGPRs.  Figures of the build this was written with: 239 VGPRs, scratch 0, LDS 0, bounded to two waves per SIMD.  It holds them
because the reader front door -- the projections of every kind, which alone take more than a wave's share of registers -- runs
once per leaf in the pass before it (k_combined_front, 291 VGPRs, held to no scratch and no LDS) and hands the positions on; with
the front door inlined per leaf and variable the kernel took 403 VGPRs, or 608 bytes of scratch under the bound."""
import os

import pytest

from code_objects import READELF, kernel_resources

pytestmark = pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')


def _found(kernel):
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, kernel)
    print(kernel, found)
    return found


def test_the_sample_kernel_is_there_once_without_scratch_and_lds():
    for kernel in ('k_combined_sample', 'k_combined_front'):
        found = _found(kernel)
        assert len(found) == 1, '%s is in the library %d times' % (kernel, len(found))
        assert found[0]['private_segment_fixed_size'] == 0 and found[0]['group_segment_fixed_size'] == 0, found


def test_the_sample_kernel_stays_within_256_registers():
    assert _found('k_combined_sample')[0]['vgpr_count'] <= 256
