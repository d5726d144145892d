"""The disassembly of precompiled kernels: the gfx950 code objects are cut out of the library's offload bundles (one bundle per
translation unit) and given to llvm-objdump."""
import os
import re
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(marker, pattern, tmp_path):
    """(name, text) of every kernel whose symbol matches the regex `pattern`, in the library's first gfx950 code object that
    holds the byte string `marker`; text is the kernel's disassembly up to its s_endpgm"""
    blob = open(SO, "rb").read()
    found = None
    at = blob.find(MAGIC)
    while at >= 0 and found is None:
        n = struct.unpack_from("<Q", blob, at + 24)[0]
        off = at + 32
        for _ in range(n):
            o, size, ts = struct.unpack_from("<QQQ", blob, off)
            triple = blob[off + 24: off + 24 + ts]
            off += 24 + ts
            elf = blob[at + o: at + o + size]
            if size and b"gfx950" in triple and marker in elf:
                found = elf
        at = blob.find(MAGIC, at + 24)
    assert found is not None, f"no gfx950 code object with {marker.decode()} in the library"
    (tmp_path / "k.co").write_bytes(found)
    out = subprocess.run([OBJDUMP, "-d", str(tmp_path / "k.co")], check=True, capture_output=True, text=True).stdout
    return [(m.group("name"), m.group("text")) for m in re.finditer(r"<(?P<name>%s)>:\n(?P<text>.*?)s_endpgm" % pattern, out, re.S)]
