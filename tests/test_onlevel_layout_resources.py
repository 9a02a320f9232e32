"""CPU: the step launch with the C3 group's static slot layout on a step whose time sits on a reader level
(k_step_grid<..., LayoutC3L1>) keeps the registers and the occupancy of the two-level launch: no scratch memory and <= 96
VGPRs (five waves per SIMD).  Its burst gathers slot A at two levels and the other slots at one (csrc/odr_field.hip.h
env_burst); this reads the code object's metadata so that an edit that makes it spill fails here."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

READELF = '/opt/rocm/llvm/bin/llvm-readelf'
OBJCOPY = '/opt/rocm/llvm/bin/llvm-objcopy'
SPEC = 'k_step_gridILi2ELi0ELb1ELb0ELi1ENS_10LayoutC3L1E'


def _code_objects(lib):
    """The gfx950 code objects of the library's .hip_fatbin: the ELF images inside the offload bundles."""
    out = []
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, 'fat.bin')
        subprocess.check_call([OBJCOPY, '--dump-section', '.hip_fatbin=' + fat, lib, os.path.join(d, 'x')])
        data = open(fat, 'rb').read()
    pos = data.find(b'\x7fELF')
    while pos >= 0:
        if data[pos + 4] == 2 and data[pos + 18] == 224:   # 64-bit, e_machine EM_AMDGPU
            shoff, = struct.unpack_from('<Q', data, pos + 40)
            shentsize, shnum = struct.unpack_from('<HH', data, pos + 58)
            out.append(data[pos:pos + shoff + shentsize * shnum])
        pos = data.find(b'\x7fELF', pos + 4)
    return out


@pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJCOPY)), reason='needs the ROCm LLVM tools')
def test_onlevel_layout_step_kernel_does_not_spill():
    import __graft_entry__ as g
    g.build()
    from opendrift_amd import _abi
    found = []
    with tempfile.TemporaryDirectory() as d:
        for k, co in enumerate(_code_objects(_abi.LIB_PATH)):
            path = os.path.join(d, 'co%d.o' % k)
            open(path, 'wb').write(co)
            notes = subprocess.run([READELF, '--notes', path], capture_output=True, text=True).stdout
            for block in re.split(r'\n\s+- \.', notes):
                m = re.search(r'(?:^|\n)\s*\.?name:\s+(\S+)', block)
                if m and SPEC in m.group(1) and not m.group(1).endswith('.kd'):
                    scratch = int(re.search(r'private_segment_fixed_size:\s+(\d+)', block).group(1))
                    vgpr = int(re.search(r'vgpr_count:\s+(\d+)', block).group(1))
                    found.append((scratch, vgpr))
    assert found, 'k_step_grid<..., LayoutC3L1> is not in the library'
    for scratch, vgpr in found:
        assert scratch == 0 and vgpr <= 96, (scratch, vgpr)
