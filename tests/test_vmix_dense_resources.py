"""CPU: every instantiation of the dense mixing kernel (k_vmix_dense, csrc/odr_kernels.hip.h: the one-element-per-thread routine
over the launch-wide list of elements to mix) exists and keeps the launch's occupancy -- no scratch memory and <= 80 VGPRs (six
waves per SIMD, ODR_VMIX_WAVES), read from the code object's metadata; its dynamic LDS (vmix_dense_lds_bytes: column and
tables) stays within a sixth of a CU's 160 KB; and the three kernels that build the list use no scratch memory."""
import os
import re

import pytest

from code_objects import READELF, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS_H = os.path.join(ROOT, 'opendrift_amd', 'csrc', 'odr_kernels.hip.h')
# the static configurations odr_vmix launches: VMixC3 and VMixC3Rec at 2 and 3 quads, VMixC3W and VMixC3RecW at 3 quads,
# each on a time level and between two
N_INSTANTIATIONS = 12
LIST_KERNELS = ('11k_vmix_keepE', '16k_vmix_keep_scanE', '16k_vmix_keep_fillE')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    return _abi.LIB_PATH


@pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
def test_dense_mixing_kernels_do_not_spill(lib):
    found = kernel_resources(lib, 'k_vmix_denseILi')
    assert len(found) == N_INSTANTIATIONS, len(found)
    for r in found:
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_count'] <= 80, r
        assert r['group_segment_fixed_size'] == 0, r          # all of its LDS is the dynamic part below


@pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
@pytest.mark.parametrize('name', LIST_KERNELS)
def test_list_kernels_use_no_scratch(lib, name):
    found = kernel_resources(lib, name)
    assert len(found) == 1, (name, len(found))
    assert found[0]['private_segment_fixed_size'] == 0, found[0]


def test_dynamic_lds_keeps_six_workgroups_per_cu():
    src = open(KERNELS_H).read()
    block = int(re.search(r'#define ODR_BLOCK (\d+)', src).group(1))
    # the expression of vmix_dense_lds_bytes, restated: float64 column [4 nq][BLOCK] and tables [4][4 nq]
    body = re.search(r'constexpr size_t vmix_dense_lds_bytes\(int nq\) \{\s*return ([^;]+);', src).group(1)
    assert body == 'sizeof(double) * ((size_t)(4 * nq) * BLOCK + 4 * (size_t)(4 * nq))', body

    def lds(nq):
        return 8 * (4 * nq * block + 4 * 4 * nq)
    assert lds(3) == 24960 and lds(3) <= 163840 // 6 == 27306
    assert lds(2) <= 163840 // 6
