"""CPU: k_ship_drift (csrc/odr_ship.hip.h) keeps the 100-point spectrum loop in registers: no scratch memory and no LDS (DESIGN.md
section 7f has the register count of the build it was written with; the test prints the present one).  Reads the metadata of the
library's gfx950 code object, so that an edit that makes the loop spill, or stages something in LDS, fails here."""
import os

import pytest

from code_objects import READELF, kernel_resources

KERNEL = 'k_ship_driftILb0E'      # k_ship_drift<false>: the launch of a run (<true> also reports the intermediates, for the tests)


@pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
def test_ship_kernel_has_no_scratch_and_no_lds():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = kernel_resources(_abi.LIB_PATH, KERNEL)
    assert len(found) == 1, 'k_ship_drift<false> is not in the library exactly once: %s' % found
    both = kernel_resources(_abi.LIB_PATH, 'k_ship_drift')
    print(both)
    assert len(both) == 2
    for r in both:
        assert r['private_segment_fixed_size'] == 0 and r['group_segment_fixed_size'] == 0, r
