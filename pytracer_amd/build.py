"""Build recipe for libptrace.so and its add-ons libptrace_rays.so, libptrace_surface.so, libptrace_scatter.so,
libptrace_radiance.so and libptrace_gather.so (HIP, gfx950 only).

``hipcc --offload-arch=gfx950 -O3 -ffp-contract=off``: the parity kernels must not fuse a*b+c (the
reference is Python: every operation rounds), and nothing enables fast-math.  The library is built
in-tree (``pytracer_amd/libptrace.so``) so it travels to the GPU box with the repository snapshot.

``libptrace_rays.so`` (csrc/ptrace_rays.hip, include/ptrace_rays.h: ray batches) is a second translation unit and a second
shared object ON PURPOSE: ``code_hash()`` of libptrace.so is what ties every ``profiles/pmc_*.json`` to the kernels it
measured, and a kernel added to ptrace.hip would change it.  Same flags, its own ``-cuid``; built after libptrace.so.

``libptrace_surface.so`` (csrc/ptrace_surface.hip, include/ptrace_surface.h: materials and point-light shading of hit
records) is the third, for the same reason once more: the exported symbols of libptrace_rays.so are its interface 1.0's.

``libptrace_scatter.so`` (csrc/ptrace_scatter.hip, include/ptrace_scatter.h: BRDF.scatter_ray and the Russian roulette for hit
records) is the fourth: the exported symbols of libptrace_surface.so are pinned to its eleven as well.

``libptrace_radiance.so`` (csrc/ptrace_radiance.hip, include/ptrace_radiance.h: the whole ``PathTracer`` recursion for ray
batches) is the fifth: the exported symbols of libptrace_scatter.so are pinned to its seven.

``libptrace_gather.so`` (csrc/ptrace_gather.hip, include/ptrace_gather.h: the mean radiance over the hemisphere of batches of
surface points) is the sixth: the exported symbols of libptrace_radiance.so are pinned to its eight.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libptrace.so")
SOURCES = ["ptrace.hip"]
RAYS_LIB = os.path.join(HERE, "libptrace_rays.so")
RAYS_SOURCES = ["ptrace_rays.hip"]
SURFACE_LIB = os.path.join(HERE, "libptrace_surface.so")
SURFACE_SOURCES = ["ptrace_surface.hip"]
SCATTER_LIB = os.path.join(HERE, "libptrace_scatter.so")
SCATTER_SOURCES = ["ptrace_scatter.hip"]
RADIANCE_LIB = os.path.join(HERE, "libptrace_radiance.so")
RADIANCE_SOURCES = ["ptrace_radiance.hip"]
GATHER_LIB = os.path.join(HERE, "libptrace_gather.so")
GATHER_SOURCES = ["ptrace_gather.hip"]
# every file the one translation unit includes: all of csrc/ (tests/test_host.py checks this list against the #include lines)
DEPS = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))) + [os.path.join("..", "..", "include", "ptrace.h"),
                                                                            os.path.join("..", "..", "include", "ptrace_debug.h"),
                                                                            os.path.join("..", "..", "include", "ptrace_rays.h"),
                                                                            os.path.join("..", "..", "include", "ptrace_surface.h"),
                                                                            os.path.join("..", "..", "include", "ptrace_scatter.h"),
                                                                            os.path.join("..", "..", "include", "ptrace_radiance.h"),
                                                                            os.path.join("..", "..", "include", "ptrace_gather.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC",
         "-shared", "-Wall", "-Wno-unused-function", "-Wno-pass-failed",
         # a fixed compilation-unit id: by default clang derives it from the command line (paths included), which would make
         # code_hash() depend on WHERE the library was built
         "-cuid=libptrace"]
RAYS_FLAGS = FLAGS[:-1] + ["-cuid=libptrace_rays"]
SURFACE_FLAGS = FLAGS[:-1] + ["-cuid=libptrace_surface"]
SCATTER_FLAGS = FLAGS[:-1] + ["-cuid=libptrace_scatter"]
RADIANCE_FLAGS = FLAGS[:-1] + ["-cuid=libptrace_radiance"]
GATHER_FLAGS = FLAGS[:-1] + ["-cuid=libptrace_gather"]
# every library the recipe makes, in build order: what build() and needs_build() walk
TARGETS = ((FLAGS, LIB, SOURCES), (RAYS_FLAGS, RAYS_LIB, RAYS_SOURCES), (SURFACE_FLAGS, SURFACE_LIB, SURFACE_SOURCES),
           (SCATTER_FLAGS, SCATTER_LIB, SCATTER_SOURCES), (RADIANCE_FLAGS, RADIANCE_LIB, RADIANCE_SOURCES),
           (GATHER_FLAGS, GATHER_LIB, GATHER_SOURCES))


def code_hash(lib: str = LIB) -> str:
    """sha256 of the DEVICE code in ``lib``: the bytes of its ``.hip_fatbin`` ELF section (the gfx950 code object bundle
    hipcc embedded).  Two builds with this hash equal run the same kernels; bench.py compares it with the hash recorded
    in every ``profiles/pmc_*.json`` it prices a roofline from and refuses to price on a mismatch.
    Pure Python (ELF64 little-endian section table): needs no ROCm tool, works wherever the library file is."""
    import hashlib
    import struct

    with open(lib, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        raise ValueError(f"{lib}: not a little-endian ELF64 file")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)

    def section(i):
        name, _type, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize)
        return name, off, size

    _, stroff, strsize = section(shstrndx)
    names = data[stroff:stroff + strsize]
    for i in range(shnum):
        name, off, size = section(i)
        if names[name:names.index(b"\0", name)] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()
    raise ValueError(f"{lib}: no .hip_fatbin section (not a HIP library?)")


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm): cannot build libptrace.so")


def needs_build() -> bool:
    libs = [lib for _, lib, _ in TARGETS]
    if not all(os.path.exists(lib) for lib in libs):
        return True
    t = min(os.path.getmtime(lib) for lib in libs)  # (one list of files for all six: they share the headers)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    for flags, lib, sources in TARGETS:
        cmd = [_hipcc()] + flags + ["-o", lib] + [os.path.join(CSRC, s) for s in sources]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
