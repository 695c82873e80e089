"""Build recipe for libptrace.so and its add-on libraries (HIP, gfx950 only).

``hipcc --offload-arch=gfx950 -O3 -ffp-contract=off``: the parity kernels must not fuse a*b+c (the
reference is Python: every operation rounds), and nothing enables fast-math.  The libraries are built
in-tree (``pytracer_amd/lib*.so``) so they travel to the GPU box with the repository snapshot.

Every add-on is a translation unit and a shared object of its own ON PURPOSE: ``code_hash()`` of libptrace.so is what ties
every ``profiles/pmc_*.json`` to the kernels it measured, and a kernel added to ptrace.hip would change it; the exported
symbols of every add-on already released are pinned to its interface in the same way.  Same flags, its own ``-cuid``; built
after libptrace.so, in the order of ``ADDONS`` (csrc/ptrace_NAME.hip, include/ptrace_NAME.h -> libptrace_NAME.so):

* rays: closest-hit and any-hit queries for a caller's own rays
* surface: materials and point-light shading of hit records
* scatter: BRDF.scatter_ray and the Russian roulette for hit records
* radiance: the whole ``PathTracer`` recursion for ray batches
* gather: the mean radiance over the hemisphere of batches of surface points
* bake: surface points from (shape, u, v), and light maps over a shape's (u, v) grid
* sh: order-2 spherical-harmonic radiance probes at free points, and their evaluation
* lit: hit records shaded from a lattice of those probes (corners, blend, evaluation and the material in one kernel)
* denoise: an edge-avoiding a-trous filter for the noisy frames and maps of the steps above, guided by their hit records
* temporal: last frame's demodulated radiance reprojected onto this frame's hit records and blended with the new samples
* variance: luminance moments for that accumulation, the per-pixel variance they give, and an a-trous filter guided by it
* adaptive: sample counts from that variance, their prefix sum, and a gather whose sample count is a per-record plane
* weighted: that accumulation with every frame weighted by the samples it took, colour and luminance moments in one launch
* motion: the weighted accumulation with a motion per shape, so that the history of a shape that moved is fetched where it was
* gradient: probes re-gathered in the previous world, the share of its history each pixel keeps, and the motion accumulation with it
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
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC",
         "-shared", "-Wall", "-Wno-unused-function", "-Wno-pass-failed",
         # a fixed compilation-unit id: by default clang derives it from the command line (paths included), which would make
         # code_hash() depend on WHERE the library was built
         "-cuid=libptrace"]
# the add-ons, in build order: name -> (sources, library, cuid)
ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}")
          for name in ("rays", "surface", "scatter", "radiance", "gather")}
# libptrace.so and the add-ons of interfaces 1.0 - 1.4, in build order
TARGETS = ((FLAGS, LIB, SOURCES),) + tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in ADDONS.values())
(_, (RAYS_FLAGS, RAYS_LIB, RAYS_SOURCES), (SURFACE_FLAGS, SURFACE_LIB, SURFACE_SOURCES), (SCATTER_FLAGS, SCATTER_LIB, SCATTER_SOURCES),
 (RADIANCE_FLAGS, RADIANCE_LIB, RADIANCE_SOURCES), (GATHER_FLAGS, GATHER_LIB, GATHER_SOURCES)) = TARGETS  # (the rows by name)
# The add-ons since interface 1.5, rows of the same kind.  ADDONS and TARGETS above keep the values they had at interface 1.4
# (tests/test_gather_host.py pins them: six rows, the gather's last), so what came later is listed here and ALL_TARGETS is what
# build() and needs_build() walk.
LATER_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("bake",)}
LATER_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in LATER_ADDONS.values())
((BAKE_FLAGS, BAKE_LIB, BAKE_SOURCES),) = LATER_TARGETS
ALL_TARGETS = TARGETS + LATER_TARGETS
# The add-ons since interface 1.6.  ALL_TARGETS keeps the value it had at interface 1.5 (tests/test_bake_host.py pins it: seven
# rows, the bake's last), so what came later is listed here and EVERY_TARGET is what build() and needs_build() walk.
NEWER_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("sh",)}
NEWER_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in NEWER_ADDONS.values())
((SH_FLAGS, SH_LIB, SH_SOURCES),) = NEWER_TARGETS
EVERY_TARGET = ALL_TARGETS + NEWER_TARGETS
# The add-ons since interface 1.7.  EVERY_TARGET keeps the value it had at interface 1.6 (tests/test_sh_host.py pins it: eight
# rows, the probes' last), so what came later is listed here and BUILD_TARGETS is what build() and needs_build() walk.
NEWEST_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("lit",)}
NEWEST_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in NEWEST_ADDONS.values())
((LIT_FLAGS, LIT_LIB, LIT_SOURCES),) = NEWEST_TARGETS
BUILD_TARGETS = EVERY_TARGET + NEWEST_TARGETS
# The add-ons since interface 1.8.  BUILD_TARGETS keeps the value it had at interface 1.7 (tests/test_lit_host.py pins it: nine
# rows, the lit library's last), so what came later is listed here and WALK_TARGETS is what build() and needs_build() walk.
DENOISE_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("denoise",)}
DENOISE_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in DENOISE_ADDONS.values())
((DENOISE_FLAGS, DENOISE_LIB, DENOISE_SOURCES),) = DENOISE_TARGETS
WALK_TARGETS = BUILD_TARGETS + DENOISE_TARGETS
# The add-ons since interface 1.9.  WALK_TARGETS keeps the value it had at interface 1.8 (tests/test_denoise_host.py pins it: ten
# rows, the denoise library's last), so what came later is listed here and FRAME_TARGETS is what build() and needs_build() walk.
TEMPORAL_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("temporal",)}
TEMPORAL_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in TEMPORAL_ADDONS.values())
((TEMPORAL_FLAGS, TEMPORAL_LIB, TEMPORAL_SOURCES),) = TEMPORAL_TARGETS
FRAME_TARGETS = WALK_TARGETS + TEMPORAL_TARGETS
# The add-ons since interface 1.10.  FRAME_TARGETS keeps the value it had at interface 1.9 (tests/test_temporal_host.py pins it:
# eleven rows, the temporal library's last), so what came later is listed here and GUIDED_TARGETS is what build() and needs_build() walk.
VARIANCE_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("variance",)}
VARIANCE_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in VARIANCE_ADDONS.values())
((VARIANCE_FLAGS, VARIANCE_LIB, VARIANCE_SOURCES),) = VARIANCE_TARGETS
GUIDED_TARGETS = FRAME_TARGETS + VARIANCE_TARGETS
# The add-ons since interface 1.11.  GUIDED_TARGETS keeps the value it had at interface 1.10 (tests/test_variance_host.py pins it:
# twelve rows, the variance library's last), so what came later is listed here and SAMPLED_TARGETS is what build() and needs_build() walk.
ADAPTIVE_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("adaptive",)}
ADAPTIVE_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in ADAPTIVE_ADDONS.values())
((ADAPTIVE_FLAGS, ADAPTIVE_LIB, ADAPTIVE_SOURCES),) = ADAPTIVE_TARGETS
SAMPLED_TARGETS = GUIDED_TARGETS + ADAPTIVE_TARGETS
# The add-ons since interface 1.12.  SAMPLED_TARGETS keeps the value it had at interface 1.11 (tests/test_adaptive_host.py pins it:
# thirteen rows, the adaptive library's last), so what came later is listed here and HISTORY_TARGETS is what build() and needs_build() walk.
WEIGHTED_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("weighted",)}
WEIGHTED_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in WEIGHTED_ADDONS.values())
((WEIGHTED_FLAGS, WEIGHTED_LIB, WEIGHTED_SOURCES),) = WEIGHTED_TARGETS
HISTORY_TARGETS = SAMPLED_TARGETS + WEIGHTED_TARGETS
# The add-ons since interface 1.13.  HISTORY_TARGETS keeps the value it had at interface 1.12 (tests/test_weighted_host.py pins it:
# fourteen rows, the weighted library's last), so what came later is listed here and MOVING_TARGETS is what build() and needs_build() walk.
MOTION_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("motion",)}
MOTION_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in MOTION_ADDONS.values())
((MOTION_FLAGS, MOTION_LIB, MOTION_SOURCES),) = MOTION_TARGETS
MOVING_TARGETS = HISTORY_TARGETS + MOTION_TARGETS
# The add-ons since interface 1.14.  MOVING_TARGETS keeps the value it had at interface 1.13 (tests/test_motion_host.py pins it:
# fifteen rows, the motion library's last), so what came later is listed here and LIGHT_TARGETS is what build() and needs_build() walk.
GRADIENT_ADDONS = {name: ([f"ptrace_{name}.hip"], os.path.join(HERE, f"libptrace_{name}.so"), f"libptrace_{name}") for name in ("gradient",)}
GRADIENT_TARGETS = tuple((FLAGS[:-1] + [f"-cuid={cuid}"], lib, sources) for sources, lib, cuid in GRADIENT_ADDONS.values())
((GRADIENT_FLAGS, GRADIENT_LIB, GRADIENT_SOURCES),) = GRADIENT_TARGETS
LIGHT_TARGETS = MOVING_TARGETS + GRADIENT_TARGETS
# every file the translation units include: all of csrc/ (tests/test_host.py checks this list against the #include lines)
DEPS = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))) + [
    os.path.join("..", "..", "include", h) for h in ["ptrace.h", "ptrace_debug.h"] + [f"ptrace_{name}.h" for name in list(ADDONS) + list(LATER_ADDONS) + list(NEWER_ADDONS) + list(NEWEST_ADDONS) + list(DENOISE_ADDONS) + list(TEMPORAL_ADDONS) + list(VARIANCE_ADDONS) + list(ADAPTIVE_ADDONS) + list(WEIGHTED_ADDONS) + list(MOTION_ADDONS) + list(GRADIENT_ADDONS)]]


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
    libs = [lib for _, lib, _ in LIGHT_TARGETS]
    if not all(os.path.exists(lib) for lib in libs):
        return True
    t = min(os.path.getmtime(lib) for lib in libs)  # (one list of files for all sixteen: they share the headers)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    for flags, lib, sources in LIGHT_TARGETS:
        cmd = [_hipcc()] + flags + ["-o", lib] + [os.path.join(CSRC, s) for s in sources]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
