"""CPU: every instantiation of the tiled K-column mixing kernel (k_vmix_col, csrc/odr_kernels.hip.h) -- the loop over a tile's
passes around the particle routine -- keeps the launch's occupancy: no scratch memory and <= 80 VGPRs (six waves per SIMD,
ODR_VMIX_WAVES), read from the code object's metadata; and the dynamic LDS of the 12-level launch (vmix_col_lds_bytes: column,
tables, the tile's 16-bit offset list and its counts) stays within a sixth of a CU's 160 KB, so six workgroups stay resident."""
import os
import re

import pytest

from code_objects import READELF, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS_H = os.path.join(ROOT, 'opendrift_amd', 'csrc', 'odr_kernels.hip.h')
N_INSTANTIATIONS = 28      # six static configurations x on a level / between two, eight run-time quad counts x the same


@pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
def test_tiled_mixing_kernels_do_not_spill():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, 'k_vmix_colILi')
    assert len(found) == N_INSTANTIATIONS, len(found)
    for r in found:
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_count'] <= 80, r


def test_dynamic_lds_keeps_six_workgroups_per_cu():
    src = open(KERNELS_H).read()
    block = int(re.search(r'#define ODR_BLOCK (\d+)', src).group(1))
    rounds = int(re.search(r'constexpr int VMIX_TILE_ROUNDS = (\d+);', src).group(1))
    # the expression of vmix_col_lds_bytes, restated: float64 column [4 nq][BLOCK] and tables [4][4 nq], uint16 list, uint32 counts
    assert 'sizeof(double) * ((size_t)(4 * nq) * BLOCK + 4 * (size_t)(4 * nq)) + sizeof(unsigned short) * VMIX_TILE +' in src
    assert 'sizeof(unsigned) * VMIX_TILE_ROUNDS * (BLOCK / 64);' in src

    def lds(nq):
        return 8 * (4 * nq * block + 4 * 4 * nq) + 2 * rounds * block + 4 * rounds * (block // 64)
    assert lds(3) == 27072 and lds(3) <= 163840 // 6 == 27306
    assert lds(2) <= 163840 // 6
    assert lds(16) <= 163840           # the longest instantiated column still fits a CU
