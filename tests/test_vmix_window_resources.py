"""CPU: the two-quad instantiations of the static 12-level mixing launch (k_vmix_col<3, TL, VMixC3W / VMixC3RecW>: K planes and
node records, on a reader level and between two) carry the whole-column routine as their in-launch fall-back and still keep the
launch's occupancy: no scratch memory and <= 80 VGPRs (six waves per SIMD, ODR_VMIX_WAVES).  Read from the code object's
metadata, as tests/test_vmix_spec_resources.py does."""
import os

import pytest

from code_objects import READELF, kernel_resources

WINDOWED = ['k_vmix_colILi3ELb%dENS_%sE' % (tl, vm) for vm in ('7VMixC3W', '10VMixC3RecW') for tl in (0, 1)]


@pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
def test_two_quad_mixing_kernels_do_not_spill():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = {}
    for name in WINDOWED:
        for r in kernel_resources(_abi.LIB_PATH, name):
            found[name] = (r['private_segment_fixed_size'], r['vgpr_count'])
    assert sorted(found) == sorted(WINDOWED), found
    for name, (scratch, vgpr) in found.items():
        assert scratch == 0 and vgpr <= 80, (name, scratch, vgpr)
