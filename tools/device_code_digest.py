"""Digest of the device code of every file in build.SOURCES, kernel by kernel: the check that a host-side change left the
kernels alone.  Needs hipcc, no GPU.

    python tools/device_code_digest.py [--all | file.hip ...] > profiles/rNN_device_code_digest_<what>.txt

Each file is compiled device-only with the library's own flags (build.FLAGS + build.FILE_FLAGS), the gfx950 code object is taken
out of the offload bundle, and per kernel symbol, sorted by name, one line is formed:

    <file> <kernel> text=<sha256 of the symbol's bytes in .text> kd=<sha256 of its 64-byte kernel descriptor>
        vgpr=<n> sgpr=<n> scratch=<bytes> lds=<bytes>          (the last four from the code object's metadata note)

(hashes cut to 64 bits.)  The lines are printed for the files named on the command line (--all: every file); for EVERY file of
build.SOURCES one more line, `<file> kernels=<n> sha256=<of its kernel lines>`, stands for them, so that an output kept under
profiles/ stays a few hundred lines: the kernels of the files a change touches, one line each for the rest.

The descriptor is hashed with its kernel_code_entry_byte_offset (bytes 16 .. 23) zeroed: that field is the distance from the
descriptor to the code, a matter of layout (one unchanged file compiled in two directories gave the same bytes for every
kernel and descriptors that differed in this field alone), while every other field -- register blocks, scratch, LDS, enabled
inputs -- describes the kernel.

Contents are hashed, not files: a host-only edit changes the bundle and ELF hashes (paths, host symbol tables) but no byte of
a kernel.  Per kernel, not per section: the order in which the host code first names the template instantiations may move
kernels inside .text without changing any of them.  Two outputs that are equal line for line mean the same kernel set with the
same code, descriptors, registers, scratch and LDS.  The tool only hashes; it looks for no instruction.
"""
import hashlib
import importlib.util
import os
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
NT_AMDGPU_METADATA = 32


def _build_module():
    spec = importlib.util.spec_from_file_location("_pn2_build", os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def code_object(blob, arch="gfx950"):
    """the ELF of `arch` inside a clang offload bundle (or the blob itself when it already is an ELF)"""
    if blob[:4] == b"\x7fELF":
        return blob
    if blob[:len(BUNDLE_MAGIC)] != BUNDLE_MAGIC:
        raise ValueError("neither an ELF nor a clang offload bundle")
    at = len(BUNDLE_MAGIC)
    (count,) = struct.unpack_from("<Q", blob, at)
    at += 8
    for _ in range(count):
        off, size, idlen = struct.unpack_from("<QQQ", blob, at)
        at += 24
        ident = blob[at:at + idlen].decode()
        at += idlen
        if ident.startswith("hip") and ident.endswith(arch):
            return blob[off:off + size]
    raise ValueError("no %s code object in the bundle" % arch)


def _sections(elf):
    if elf[4] != 2 or elf[5] != 1:
        raise ValueError("ELF64 little-endian expected")
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    raw = []
    for i in range(shnum):
        name, typ, _flags, addr, off, size, link, _info, _align, entsize = struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
        raw.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link, entsize=entsize))
    strtab = raw[shstrndx]
    for s in raw:
        end = elf.index(b"\0", strtab["off"] + s["name"])
        s["name"] = elf[strtab["off"] + s["name"]:end].decode()
    return raw


def _metadata(elf, sections):
    """kernel name -> its entry of amdhsa.kernels (the NT_AMDGPU_METADATA note, msgpack)"""
    import msgpack
    for s in sections:
        if s["type"] != 7:  # SHT_NOTE
            continue
        at, end = s["off"], s["off"] + s["size"]
        while at < end:
            namesz, descsz, typ = struct.unpack_from("<III", elf, at)
            at += 12
            name = elf[at:at + namesz].rstrip(b"\0")
            at += (namesz + 3) & ~3
            desc = elf[at:at + descsz]
            at += (descsz + 3) & ~3
            if name == b"AMDGPU" and typ == NT_AMDGPU_METADATA:
                meta = msgpack.unpackb(desc, raw=False)
                return {k[".name"]: k for k in meta.get("amdhsa.kernels", [])}
    return {}  # a file without kernels


def kernels(elf):
    """[(kernel, sha256 of its .text bytes, sha256 of its descriptor, vgpr, sgpr, scratch bytes, lds bytes)] sorted by name"""
    sections = _sections(elf)
    meta = _metadata(elf, sections)
    if not meta:
        return []
    symtab = next(s for s in sections if s["type"] == 2)
    names = sections[symtab["link"]]
    syms = {}
    for i in range(symtab["size"] // symtab["entsize"]):
        name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, symtab["off"] + i * symtab["entsize"])
        end = elf.index(b"\0", names["off"] + name)
        syms[elf[names["off"] + name:end].decode()] = (shndx, value, size)

    def contents(sym):
        shndx, value, size = syms[sym]
        sec = sections[shndx]
        start = sec["off"] + value - sec["addr"]
        return elf[start:start + size]

    out = []
    for name in sorted(meta):
        m = meta[name]
        code, kd = contents(name), contents(m[".symbol"])
        if not code or len(kd) != 64:
            raise ValueError("kernel %s: empty code or a descriptor that is not 64 bytes" % name)
        kd = kd[:16] + bytes(8) + kd[24:]  # kernel_code_entry_byte_offset: where the code lies from here, not what the kernel is
        out.append((name, hashlib.sha256(code).hexdigest()[:16], hashlib.sha256(kd).hexdigest()[:16], m[".vgpr_count"], m[".sgpr_count"],
                    m[".private_segment_fixed_size"], m[".group_segment_fixed_size"]))
    return out


def digest_file(build, src, tmpdir):
    obj = os.path.join(tmpdir, src + ".device")
    cmd = [build._hipcc()] + build.FLAGS + build.FILE_FLAGS.get(src, []) + ["--offload-device-only", "-c",
                                                                            os.path.join(build.CSRC, src), "-o", obj]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    with open(obj, "rb") as f:
        return kernels(code_object(f.read()))


def main(argv):
    build = _build_module()
    listed = build.SOURCES if "--all" in argv else [a for a in argv if a != "--all"]
    with tempfile.TemporaryDirectory() as tmpdir, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        results = list(pool.map(lambda src: digest_file(build, src, tmpdir), build.SOURCES))
    for src, rows in zip(build.SOURCES, results):
        lines = ["%s %s text=%s kd=%s vgpr=%d sgpr=%d scratch=%d lds=%d" % ((src,) + row) for row in rows]
        if src in listed:
            print("\n".join(lines))
        print("%s kernels=%d sha256=%s" % (src, len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()))


if __name__ == "__main__":
    main(sys.argv[1:])
