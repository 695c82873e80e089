"""Device memory and streams through the C-ABI (``pt_device_alloc`` / ``pt_stream_create``, ABI 1.5): what the resident frame of
the ``render`` command and the frames of a :class:`pytracer_amd.pipeline.FramePipeline` live in when the caller brings no GPU
framework of its own.  The reference keeps its frame in a Python list (hdrimages.py:70); here it stays in HBM between the
render kernel and the post-processing kernels, and this is the buffer that takes.  Nothing here imports torch."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib


class Stream:
    """A non-blocking HIP stream on ``device`` (``pt_stream_create``); ``handle`` is what ``pt_render_device`` takes."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _lib.check(_lib.lib().pt_stream_create(int(device), C.byref(h)))
        self.device, self.handle = int(device), h.value

    @property
    def cuda_stream(self) -> int:  # (the attribute torch's streams carry the same handle under)
        return self.handle

    def synchronize(self) -> None:
        if self.handle is not None:
            _lib.check(_lib.lib().pt_stream_sync(self.device, C.c_void_p(self.handle)))

    def close(self) -> None:
        if self.handle is not None:
            h, self.handle = self.handle, None
            _lib.check(_lib.lib().pt_stream_destroy(self.device, C.c_void_p(h)))

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class DeviceBuffer:
    """``shape`` values of ``dtype`` in the HBM of ``device``: ``data_ptr()`` for the C-ABI, ``numpy()`` to copy it to the host."""

    is_device_buffer = True

    def __init__(self, shape: Tuple[int, ...], dtype=np.float64, device: int = 0):
        self.shape = tuple(int(x) for x in shape)
        self.dtype = np.dtype(dtype)
        self.device = int(device)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        _lib.check(_lib.lib().pt_device_alloc(self.device, self.nbytes, C.byref(p)))
        self._ptr: Optional[int] = p.value
        self.last_stream = None  # the stream the buffer was last rendered on (see rendered_on)

    def data_ptr(self) -> int:
        if self._ptr is None and self.nbytes:
            raise RuntimeError("DeviceBuffer used after free()")
        return self._ptr or 0

    def rendered_on(self, stream) -> "DeviceBuffer":
        """Note the stream (a :class:`Stream`, a raw ``hipStream_t`` value, or ``None`` for a synchronous call with nothing in
        flight) a render into this buffer was enqueued on: ``numpy()`` then orders its download behind it by default."""
        self.last_stream = stream
        return self

    def numpy(self, stream: Optional[Stream] = None) -> np.ndarray:
        """Copy to the host, ordered behind ``stream`` -- by default the stream the buffer was last rendered on
        (``rendered_on``), so that a frame still in flight on a caller's stream is complete when this returns."""
        if stream is None:
            stream = self.last_stream
        handle = getattr(stream, "handle", stream)  # (a closed Stream has handle None: nothing of it is in flight)
        out = np.empty(self.shape, dtype=self.dtype)
        _lib.check(_lib.lib().pt_device_download(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.data_ptr()), self.nbytes,
                                                 C.c_void_p(handle) if handle else None))
        return out

    def free(self) -> None:
        if self._ptr is not None:
            p, self._ptr = self._ptr, None
            _lib.check(_lib.lib().pt_device_free(self.device, C.c_void_p(p)))

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001
            pass


class DeviceSpan:
    """``nbytes`` bytes at ``offset`` inside a device buffer (anything with ``data_ptr()``), or at a raw device address: what a
    ``device=True`` call takes where it wants a buffer that knows its size -- the ray block inside a scatter batch handed to
    ``DeviceScene.trace_rays``.  Owns nothing; the buffer must outlive it."""

    def __init__(self, base, nbytes: int, offset: int = 0):
        self._base, self.offset, self.nbytes = base, int(offset), int(nbytes)

    def data_ptr(self) -> int:
        base = self._base.data_ptr() if callable(getattr(self._base, "data_ptr", None)) else int(self._base)
        return base + self.offset
