"""TEST INFRASTRUCTURE: the gfx950 code objects inside a HIP shared library and what their metadata says about each kernel
(scratch, LDS, registers), read with the ROCm LLVM tools.  The *_resources.py tests hold kernels to their budgets with it."""
import os
import re
import struct
import subprocess
import tempfile

READELF = '/opt/rocm/llvm/bin/llvm-readelf'
OBJCOPY = '/opt/rocm/llvm/bin/llvm-objcopy'
RESOURCES = ('private_segment_fixed_size', 'group_segment_fixed_size', 'vgpr_count', 'sgpr_count')
_blocks = {}


def code_objects(lib):
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


def _named_blocks(lib):
    """(name, metadata block) of every named entry in the notes of the library's code objects; read once per build of it."""
    key = (os.path.abspath(lib), os.path.getmtime(lib))
    if key not in _blocks:
        found = []
        with tempfile.TemporaryDirectory() as d:
            for k, co in enumerate(code_objects(lib)):
                path = os.path.join(d, 'co%d.o' % k)
                open(path, 'wb').write(co)
                notes = subprocess.run([READELF, '--notes', path], capture_output=True, text=True).stdout
                for block in re.split(r'\n\s+- \.', notes):
                    m = re.search(r'(?:^|\n)\s*\.?name:\s+(\S+)', block)
                    if m and not m.group(1).endswith('.kd'):
                        found.append((m.group(1), block))
        _blocks[key] = found
    return _blocks[key]


def kernel_resources(lib, name):
    """RESOURCES of every kernel of the library whose mangled name contains `name`."""
    return [{k: int(re.search(r'%s:\s+(\d+)' % k, block).group(1)) for k in RESOURCES}
            for kernel, block in _named_blocks(lib) if name in kernel]
