"""CPU: the mixing launch with C3's static configuration (k_vmix_col<NQ, TL, VMixC3>, both level counts of C3's field, both
time-level cases) keeps the occupancy of the run-time configuration's launch: no scratch memory and <= 80 VGPRs (six waves per
SIMD, ODR_VMIX_WAVES).  Without the fences between the column's quads (csrc/odr_kernels.hip.h vmix_col_fill) the 8-level column
with two time levels spilled; this reads the code object's metadata so that an edit that brings the spill back fails here."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

READELF = '/opt/rocm/llvm/bin/llvm-readelf'
SPEC = ['k_vmix_colILi%dELb%dENS_6VMixC3E' % (nq, tl) for nq in (2, 3) for tl in (0, 1)]


def _code_objects(lib):
    """The gfx950 code objects of the library's .hip_fatbin: the ELF images inside the offload bundles."""
    out = []
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, 'fat.bin')
        subprocess.check_call(['/opt/rocm/llvm/bin/llvm-objcopy', '--dump-section', '.hip_fatbin=' + fat, lib, os.path.join(d, 'x')])
        data = open(fat, 'rb').read()
    pos = data.find(b'\x7fELF')
    while pos >= 0:
        if data[pos + 4] == 2 and data[pos + 18] == 224:   # 64-bit, e_machine EM_AMDGPU
            shoff, = struct.unpack_from('<Q', data, pos + 40)
            shentsize, shnum = struct.unpack_from('<HH', data, pos + 58)
            out.append(data[pos:pos + shoff + shentsize * shnum])
        pos = data.find(b'\x7fELF', pos + 4)
    return out


@pytest.mark.skipif(not os.path.exists(READELF), reason='needs the ROCm LLVM tools')
def test_static_mixing_kernels_do_not_spill():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for k, co in enumerate(_code_objects(_abi.LIB_PATH)):
            path = os.path.join(d, 'co%d.o' % k)
            open(path, 'wb').write(co)
            notes = subprocess.run([READELF, '--notes', path], capture_output=True, text=True).stdout
            for block in re.split(r'\n\s+- \.', notes):
                m = re.search(r'(?:^|\n)\s*\.?name:\s+(\S+)', block)
                if not m or m.group(1).endswith('.kd'):
                    continue
                for spec in SPEC:
                    if spec in m.group(1):
                        scratch = int(re.search(r'private_segment_fixed_size:\s+(\d+)', block).group(1))
                        vgpr = int(re.search(r'vgpr_count:\s+(\d+)', block).group(1))
                        found[spec] = (scratch, vgpr)
    assert sorted(found) == sorted(SPEC), found
    for spec, (scratch, vgpr) in found.items():
        assert scratch == 0 and vgpr <= 80, (spec, scratch, vgpr)
