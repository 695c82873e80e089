"""The loader of every add-on library (libptrace_rays.so, libptrace_surface.so, ...), written once.

An add-on has no link dependency on libptrace.so and loads nothing itself: it is handed the scene's argument block
(``_rays_lib.scene_args``; all libraries come from one build of the tree, and each refuses a block of another size).  What
differs between them is data: the file, the symbols with their C types, and the interface version -- each ``_NAME_lib``
module states its own and binds ``lib`` / ``lib_path`` / ``last_error`` / ``check`` to an :class:`Addon`.  Nothing is
loaded before the first ``lib()``.  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib


def c_int(x, what) -> int:
    """``x`` for a C ``int`` field of a params structure."""
    x = int(x)
    if not -2 ** 31 <= x < 2 ** 31:
        raise ValueError(f"{what}={x} does not fit a C int")
    return x


def background3(background) -> C.Array:
    """The ``background`` field of a params structure, from a ``Color`` or three numbers."""
    bg = (background.r, background.g, background.b) if hasattr(background, "r") else tuple(background)
    if len(bg) != 3:
        raise ValueError("background must be a Color or three numbers")
    return (C.c_double * 3)(*[float(x) for x in bg])


class Addon:
    """``file``: the library beside this module; ``env``: the variable that names an alternative build of the same C-ABI
    library (mutation runs; as PTRACE_LIB for libptrace.so), read once, here; ``interface``: what the version error calls the
    ABI; ``version`` / ``last_error``: the symbols of those two entry points; ``major`` / ``minor``: the interface this package
    needs (the major exactly, the minor at least); ``signatures``: ``(symbol, restype, argtypes)`` per exported function."""

    def __init__(self, file, env, interface, version, last_error, major, minor, signatures):
        self.path = os.environ.get(env) or os.path.join(os.path.dirname(os.path.abspath(__file__)), file)
        self.interface, self.version, self.error_symbol = interface, version, last_error
        self.major, self.minor, self.signatures = major, minor, signatures
        self._loaded = None

    def lib_path(self) -> str:
        return self.path

    def lib(self):
        """The loaded library; raises if it has not been built (``python -m pytracer_amd.build``)."""
        if self._loaded is None:
            if not os.path.exists(self.path):
                raise ImportError(f"{self.path} is missing: the HIP extension has not been built. "
                                  "Run `python -m pytracer_amd.build` (needs hipcc); there is no CPU fallback.")
            _lib.lib()  # first: ONE HIP runtime per process, the one libptrace.so bound to (shared with torch unless standalone())
            L = C.CDLL(self.path)
            for symbol, restype, argtypes in self.signatures:
                fn = getattr(L, symbol)
                fn.restype, fn.argtypes = restype, list(argtypes)
            ver = int(getattr(L, self.version)())
            if ver >> 16 != self.major or (ver & 0xFFFF) < self.minor:
                needs = f"{self.major}.{self.minor} or later" if self.minor else f"{self.major}.x"
                raise ImportError(f"{self.path} implements {self.interface} {ver >> 16}.{ver & 0xFFFF}; this package needs {needs}: "
                                  "rebuild with `python -m pytracer_amd.build --force`")
            self._loaded = L
        return self._loaded

    def last_error(self) -> str:
        buf = C.create_string_buffer(512)
        getattr(self.lib(), self.error_symbol)(buf, 512)
        return buf.value.decode("utf-8", "replace")

    def check(self, rc: int) -> None:
        if rc != 0:
            raise _lib.PtraceError(rc, self.last_error())
