"""DeviceScene: a scene resident in the HBM of one MI355X, rendered through the C-ABI."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib, abi


class _PinnedBuf:
    """One page-locked host buffer (``pt_host_alloc``) exposed through the array interface; the numpy arrays
    viewing it keep it alive, and it goes back to the pool when the last one is collected."""

    def __init__(self, ptr: int, nbytes: int):
        self.ptr, self.nbytes = ptr, nbytes
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def __del__(self):
        try:
            _release_pinned(self.ptr, self.nbytes)
        except Exception:
            pass


_free_pinned = {}  # nbytes -> [ptr, ...]; at most _POOL_KEEP idle buffers per size stay allocated
_POOL_KEEP = 2


def _release_pinned(ptr: int, nbytes: int) -> None:
    idle = _free_pinned.setdefault(nbytes, [])
    if len(idle) < _POOL_KEEP:
        idle.append(ptr)
    else:
        _lib.lib().pt_host_free(C.c_void_p(ptr))


def free_pinned_pool() -> None:
    """Release every idle page-locked buffer of the pool (also registered to run at interpreter exit)."""
    for idle in _free_pinned.values():
        while idle:
            try:
                _lib.lib().pt_host_free(C.c_void_p(idle.pop()))
            except Exception:
                pass


import atexit  # noqa: E402

atexit.register(free_pinned_pool)


def pinned_empty(shape, dtype) -> np.ndarray:
    """``np.empty(shape, dtype)`` in page-locked host memory: the destination ``pt_render`` copies into at link
    speed (a pageable array costs about half again as much per frame)."""
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    if nbytes == 0:
        return np.empty(shape, dtype=dtype)
    idle = _free_pinned.get(nbytes)
    if idle:
        ptr = idle.pop()
    else:
        p = C.c_void_p()
        _lib.check(_lib.lib().pt_host_alloc(nbytes, C.byref(p)))
        ptr = int(p.value)
    return np.asarray(_PinnedBuf(ptr, nbytes)).view(dtype).reshape(shape)


class DeviceScene:
    """Owns a ``pt_scene`` handle (``pt_scene_upload`` / ``pt_scene_free``)."""

    def __init__(self, scene: abi.FlatScene, device: int = 0):
        self._h = C.c_void_p()
        self.flat = scene
        self.device = device
        d = scene.desc()
        _lib.check(_lib.lib().pt_scene_upload(C.byref(d), int(device), C.byref(self._h)))

    def clone(self) -> "DeviceScene":
        """A further handle on the same scene (``pt_scene_clone``): shares the uploaded tables, has its own per-camera
        constants, queues and workspace -- so that frames rendered through different handles may be in flight at once,
        each on its own stream (``pytracer_amd.pipeline.FramePipeline``)."""
        other = DeviceScene.__new__(DeviceScene)
        other._h = C.c_void_p()
        other.flat = self.flat
        other.device = self.device
        _lib.check(_lib.lib().pt_scene_clone(self._h, C.byref(other._h)))
        return other

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().pt_scene_free(self._h)
            self._h = C.c_void_p()
            self._kargs = None  # (its device copy went with the handle)
            slots, self._slots = getattr(self, "_slots", None), None
            if slots is not None:
                slots.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def output_shape(params: abi.Params) -> Tuple[int, int, int]:
        return int(_lib.lib().pt_rows_for_rank(C.byref(params))), int(params.width), 3

    def render(self, cam: abi.Camera, params: abi.Params, pinned: bool = False) -> np.ndarray:
        """Kernel + device->host copy; returns ``[rows_for_rank, W, 3]`` (fp64 or fp32) as an ordinary numpy array, or
        with ``pinned=True`` in page-locked memory from a small pool (for callers that consume the frame at once: the
        array's memory goes back to the pool when it is collected; ``free_pinned_pool()`` releases the idle buffers)."""
        dt = np.float64 if params.out_format == abi.OUT_F64 else np.float32
        out = pinned_empty(self.output_shape(params), dt) if pinned else np.empty(self.output_shape(params), dtype=dt)
        _lib.check(_lib.lib().pt_render(self._h, C.byref(cam), C.byref(params),
                                        out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def render_into(self, cam: abi.Camera, params: abi.Params, dev_ptr: int, nbytes: int,
                    stream: Optional[int] = None) -> None:
        """Render into caller-owned device memory (e.g. a torch tensor's ``data_ptr()``) on ``stream``
        (a ``hipStream_t`` value; ``None`` = the library's stream, synchronous)."""
        _lib.check(_lib.lib().pt_render_device(self._h, C.byref(cam), C.byref(params), C.c_void_p(dev_ptr),
                                               nbytes, C.c_void_p(stream) if stream else None))

    def render_hits(self, cam: abi.Camera, params: abi.Params, channels=abi.HIT_ALL, pinned: bool = False):
        """The hit-record frame of ``params`` (``pt_render_hits``: kernel + device->host copy) -> :class:`pytracer_amd.hits.HitFrame`,
        numpy views over ONE host buffer (page-locked with ``pinned=True``, as :meth:`render`)."""
        from .hits import HitFrame

        channels = abi.hit_channels(channels)
        nbytes = int(_lib.lib().pt_hits_bytes(C.byref(params), channels))
        buf = pinned_empty((nbytes,), np.uint8) if pinned else np.empty((nbytes,), dtype=np.uint8)
        _lib.check(_lib.lib().pt_render_hits(self._h, C.byref(cam), C.byref(params), channels, buf.ctypes.data_as(C.c_void_p), nbytes))
        return HitFrame(buf, params, channels)

    def render_hits_into(self, cam: abi.Camera, params: abi.Params, channels, dev_ptr, nbytes: Optional[int] = None,
                         stream=None) -> None:
        """The same frame into caller-owned device memory of ``pt_hits_bytes`` bytes on ``stream`` (``pt_render_hits_device``;
        ``None`` = the library's stream, synchronous).  ``dev_ptr``: a device address, or a
        :class:`pytracer_amd.devmem.DeviceBuffer` -- which then remembers ``stream``, so that its ``numpy()`` waits for this
        frame; ``stream``: a ``hipStream_t`` value or a :class:`pytracer_amd.devmem.Stream`.
        ``HitFrame(buffer.numpy(), params, channels)`` views a download."""
        handle = getattr(stream, "handle", stream)
        if getattr(dev_ptr, "is_device_buffer", False):
            nbytes = dev_ptr.nbytes if nbytes is None else nbytes
            dev_ptr.rendered_on(stream)
            dev_ptr = dev_ptr.data_ptr()
        _lib.check(_lib.lib().pt_render_hits_device(self._h, C.byref(cam), C.byref(params), abi.hit_channels(channels),
                                                    C.c_void_p(dev_ptr), int(nbytes), C.c_void_p(handle) if handle else None))

    # -- ray batches (include/ptrace_rays.h, libptrace_rays.so): the caller's own rays through the scene ---------------------
    def kernel_args(self):
        """The scene's argument block (``pt_scene_kernel_args``, ABI 1.7) as ``pt_rays_trace*`` take it: fetched once per handle."""
        from . import _rays_lib

        if getattr(self, "_kargs", None) is None:
            self._kargs = _rays_lib.scene_args(self._h)
        return self._kargs

    def _trace(self, rays, channels: int, anyhit: bool, device, stream, out):
        from . import _rays_lib, rays as rb

        L = _rays_lib.lib()
        block = self.kernel_args()
        handle = getattr(stream, "handle", stream)
        if device:
            # (a DeviceBuffer, or anything else that names device memory the same way: a torch tensor has data_ptr() and nbytes)
            if not callable(getattr(rays, "data_ptr", None)) or int(rays.nbytes) % 64:
                raise TypeError("device=True takes the rays as a DeviceBuffer (or a device tensor) holding [8, n] float64")
            n = int(rays.nbytes) // 64
            need = rb.rays_bytes(n, channels, anyhit)
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((need,), np.uint8, self.device)
            _rays_lib.check(L.pt_rays_trace_device(self.device, block, len(block), C.c_void_p(rays.data_ptr()), n, channels, int(anyhit),
                                                   C.c_void_p(out.data_ptr()), int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out, n
        if stream is not None or out is not None:
            raise ValueError("stream= and out= go with device=True (host batches are staged and synchronous)")
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        if rays.ndim != 2 or rays.shape[0] != 8:
            raise ValueError(f"rays must be the [8, n] block of pytracer_amd.rays.ray_planes, not {rays.shape}")
        n = rays.shape[1]
        buf = np.empty(rb.rays_bytes(n, channels, anyhit), dtype=np.uint8)
        _rays_lib.check(L.pt_rays_trace(self.device, block, len(block), rays.ctypes.data_as(C.c_void_p), n, channels, int(anyhit),
                                        buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return buf, n

    def trace_rays(self, rays, channels=None, device: bool = False, stream=None, out=None):
        """``World.ray_intersection`` (world.py:51-69) for a batch: ``rays`` is the ``[8, n]`` block of
        :func:`pytracer_amd.rays.ray_planes` -> :class:`pytracer_amd.rays.RayHits` with the selected ``channels`` (default: t,
        point, normal, uv).  ``device=True``: ``rays`` is a :class:`pytracer_amd.devmem.DeviceBuffer` holding that block, the
        batch is enqueued on ``stream`` (a ``Stream`` or ``hipStream_t``; ``None``: synchronous) and the result stays in HBM:
        -> the output ``DeviceBuffer`` (``out``, or a new one), which remembers the stream -- ``RayHits(buf.numpy(), n, channels)``
        views a download."""
        from . import rays as rb

        bits = rb.RAY_CHANNELS if channels is None else rb.ray_channels(channels)
        buf, n = self._trace(rays, bits, False, device, stream, out)
        return buf if device else rb.RayHits(buf, n, bits)

    def occluded(self, rays, device: bool = False, stream=None, out=None):
        """``[n]`` int32, 1 where some shape has a root in the ray's (tmin, tmax) -- ``Shape.quick_ray_intersection`` over the
        world, what ``World.is_point_visible`` negates (world.py:76-78) -- else 0.  ``device=True``: as :meth:`trace_rays`, the
        result a ``DeviceBuffer`` whose first ``4 n`` bytes are that plane."""
        buf, n = self._trace(rays, 0, True, device, stream, out)
        return buf if device else buf[: n * 4].view(np.int32)

    def points_visible(self, points, observer) -> np.ndarray:
        """``[n]`` bool: ``World.is_point_visible(points[i], observer)`` (world.py:71-80)."""
        from . import rays as rb

        return self.occluded(rb.visibility_rays(points, observer)) == 0

    # -- surface queries (include/ptrace_surface.h, libptrace_surface.so): the records' materials, and their light --------
    def slot_table(self):
        """The scene's ``World.shapes`` index -> record table in HBM (``pt_rays_slots_device``), made once per handle like
        :meth:`kernel_args` and freed with it -> :class:`pytracer_amd.devmem.DeviceBuffer`."""
        from . import _surface_lib
        from .devmem import DeviceBuffer

        if getattr(self, "_slots", None) is None:
            L, block = _surface_lib.lib(), self.kernel_args()
            need = int(L.pt_rays_slots_bytes(block, len(block)))
            table = DeviceBuffer((max(need, 8),), np.uint8, self.device)
            _surface_lib.check(L.pt_rays_slots_device(self.device, block, len(block), C.c_void_p(table.data_ptr()), table.nbytes, None))
            self._slots = table
        return self._slots

    @staticmethod
    def _plane_ptr(x, what: str):
        """A device address from a ``DeviceBuffer`` / device tensor (``data_ptr()``) or a raw address (a plane inside one)."""
        if x is None:
            return None
        if callable(getattr(x, "data_ptr", None)):
            return C.c_void_p(int(x.data_ptr()))
        if isinstance(x, (int, np.integer)):
            return C.c_void_p(int(x))
        raise TypeError(f"device=True takes {what} as a DeviceBuffer, a device tensor or a raw device address, not {type(x).__name__}")

    @staticmethod
    def _device_count(first, n) -> int:
        if n is not None:
            return int(n)
        if not hasattr(first, "nbytes"):
            raise ValueError("n= is needed when the planes are raw device addresses")
        return int(first.nbytes) // 4

    def surface(self, shape_index, uv=None, channels="all", device: bool = False, stream=None, out=None, n=None):
        """The material of every hit record: ``brdf.pigment.get_color(uv)`` and ``emitted_radiance.get_color(uv)``
        (materials.py:50-100; ``channels``: ``"brdf_color"``, ``"emitted"``, ``"all"``, ``"none"`` or ``PT_SURF_*`` bits) and the
        BRDF's kind.  ``shape_index``: ``World.shapes`` indices (negative: no hit), any shape; ``uv``: ``[..., 2]`` (not needed
        without a colour) -> :class:`pytracer_amd.rays.SurfaceColors`.  ``device=True``: ``shape_index`` (``n`` int32) and
        ``uv`` (two planes of ``n`` doubles) are in HBM -- ``DeviceBuffer`` s, device tensors, or raw addresses of planes inside
        a ray-batch or hit-frame buffer, then with ``n=`` -- the batch is enqueued on ``stream`` and the result stays there:
        -> the output ``DeviceBuffer`` (``out``, or a new one), as :meth:`trace_rays`."""
        from . import _surface_lib, rays as rb

        L, block, bits = _surface_lib.lib(), self.kernel_args(), rb.surface_channels(channels)
        if device:
            handle = getattr(stream, "handle", stream)
            n = self._device_count(shape_index, n)
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((max(rb.surface_bytes(n, bits), 8),), np.uint8, self.device)
            _surface_lib.check(L.pt_rays_surface_device(self.device, block, len(block), C.c_void_p(self.slot_table().data_ptr()),
                                                        self._plane_ptr(shape_index, "shape_index"), self._plane_ptr(uv, "uv"), n, bits,
                                                        self._plane_ptr(out, "out"), int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None:
            raise ValueError("stream=, out= and n= go with device=True (host batches are staged and synchronous)")
        shape = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        n = shape.shape[0]
        uvp = rb.planar(uv, 2) if bits else None
        if uvp is not None and uvp.shape[1] != n:
            raise ValueError(f"{n} shape indices but {uvp.shape[1]} (u, v) pairs")
        buf = np.empty(rb.surface_bytes(n, bits), dtype=np.uint8)
        _surface_lib.check(L.pt_rays_surface(self.device, block, len(block), shape.ctypes.data_as(C.c_void_p),
                                             uvp.ctypes.data_as(C.c_void_p) if uvp is not None else None, n, bits,
                                             buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return rb.SurfaceColors(buf, n, bits)

    def shade_lights(self, shape_index, point, normal, uv, dirs, ambient=(0.1, 0.1, 0.1), background=(0.0, 0.0, 0.0),
                     device: bool = False, stream=None, out=None, n=None):
        """``PointLightRenderer.__call__`` (render.py:157-193) for every hit record: ``background`` where nothing was hit, else
        ``ambient`` + emitted + one term per point light of the scene that ``World.is_point_visible`` sees from the hit point.
        ``point``, ``normal``, ``dirs``: ``[..., 3]``, ``uv``: ``[..., 2]``, ``dirs`` the directions of the rays that were traced
        -> ``[n, 3]`` float64 (a view of the three planes the library wrote).  ``device=True``: planes in HBM as for
        :meth:`surface`; -> the output ``DeviceBuffer`` of ``[3, n]`` float64."""
        from . import _surface_lib, rays as rb

        L, block = _surface_lib.lib(), self.kernel_args()
        amb, bg = _surface_lib.rgb(ambient), _surface_lib.rgb(background)
        if device:
            handle = getattr(stream, "handle", stream)
            n = self._device_count(shape_index, n)
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((3, max(n, 1)), np.float64, self.device)
            ptr = self._plane_ptr
            _surface_lib.check(L.pt_rays_shade_lights_device(self.device, block, len(block), C.c_void_p(self.slot_table().data_ptr()),
                                                             ptr(shape_index, "shape_index"), ptr(point, "point"), ptr(normal, "normal"),
                                                             ptr(uv, "uv"), ptr(dirs, "dirs"), n, amb, bg, ptr(out, "out"), int(out.nbytes),
                                                             C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None:
            raise ValueError("stream=, out= and n= go with device=True (host batches are staged and synchronous)")
        shape = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        n = shape.shape[0]
        planes = [rb.planar(point, 3), rb.planar(normal, 3), rb.planar(uv, 2), rb.planar(dirs, 3)]
        if any(p.shape[1] != n for p in planes):
            raise ValueError(f"{n} shape indices but {[p.shape[1] for p in planes]} points, normals, (u, v) pairs and directions")
        buf = np.empty((3, n), dtype=np.float64)
        _surface_lib.check(L.pt_rays_shade_lights(self.device, block, len(block), shape.ctypes.data_as(C.c_void_p),
                                                  *[p.ctypes.data_as(C.c_void_p) for p in planes], n, amb, bg,
                                                  buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return buf.T

    # -- the bounce (include/ptrace_scatter.h, libptrace_scatter.so): roulette and BRDF.scatter_ray, a generator per record ---
    def scatter(self, shape_index, point, normal, uv, dirs, pcg, roulette: bool = False, channels="all", device: bool = False,
                stream=None, out=None, n=None):
        """The bounce of ``PathTracer.__call__`` (render.py:107-134, one child) for every hit record: the Russian roulette
        (``roulette``: whether ``ray.depth >= russian_roulette_limit`` holds for this batch) and ``brdf.scatter_ray``
        (materials.py:132-196), drawing from the record's own generator.  ``point``, ``normal``, ``dirs``: ``[..., 3]``,
        ``uv``: ``[..., 2]``, ``dirs`` the directions of the rays that were traced; ``pcg``: ``uint64[2, n]`` -- state and
        increment per record (:func:`pytracer_amd.rays.pcg_streams`, or ``ScatteredRays.pcg`` of the bounce before);
        ``channels``: ``"weight"``, ``"emitted"``, ``"all"``, ``"none"`` or ``PT_SCAT_*`` bits
        -> :class:`pytracer_amd.rays.ScatteredRays`, whose ``rays`` block :meth:`trace_rays` takes as it stands.
        ``device=True``: the planes are in HBM as for :meth:`shade_lights` (``pcg``: a buffer of ``[2, n]`` uint64, or a pair
        of plane addresses); the batch is enqueued on ``stream`` -> the output ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _scatter_lib, rays as rb

        L, block, bits = _scatter_lib.lib(), self.kernel_args(), rb.scatter_channels(channels)
        if device:
            handle = getattr(stream, "handle", stream)
            n = self._device_count(shape_index, n)
            if isinstance(pcg, (tuple, list)):
                state, inc = pcg
            else:
                base = int(self._plane_ptr(pcg, "pcg").value or 0)
                state, inc = base, base + 8 * n
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((max(rb.scatter_bytes(n, bits), 8),), np.uint8, self.device)
            ptr = self._plane_ptr
            _scatter_lib.check(L.pt_rays_scatter_device(self.device, block, len(block), C.c_void_p(self.slot_table().data_ptr()),
                                                        ptr(shape_index, "shape_index"), ptr(point, "point"), ptr(normal, "normal"),
                                                        ptr(uv, "uv"), ptr(dirs, "dirs"), ptr(state, "pcg state"), ptr(inc, "pcg inc"), n,
                                                        int(bool(roulette)), bits, ptr(out, "out"), int(out.nbytes),
                                                        C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None:
            raise ValueError("stream=, out= and n= go with device=True (host batches are staged and synchronous)")
        shape = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        n = shape.shape[0]
        planes = [rb.planar(point, 3), rb.planar(normal, 3), rb.planar(uv, 2), rb.planar(dirs, 3)]
        if any(p.shape[1] != n for p in planes):
            raise ValueError(f"{n} shape indices but {[p.shape[1] for p in planes]} points, normals, (u, v) pairs and directions")
        gen = np.ascontiguousarray(pcg, dtype=np.uint64)
        if gen.shape != (2, n):
            raise ValueError(f"pcg must be uint64[2, {n}] (state and increment per record: pytracer_amd.rays.pcg_streams), not {gen.shape}")
        buf = np.empty(rb.scatter_bytes(n, bits), dtype=np.uint8)
        _scatter_lib.check(L.pt_rays_scatter(self.device, block, len(block), shape.ctypes.data_as(C.c_void_p),
                                             *[p.ctypes.data_as(C.c_void_p) for p in planes], gen[0].ctypes.data_as(C.c_void_p),
                                             gen[1].ctypes.data_as(C.c_void_p), n, int(bool(roulette)), bits,
                                             buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return rb.ScatteredRays(buf, n, bits)

    # -- the whole recursion (include/ptrace_radiance.h, libptrace_radiance.so): PathTracer.__call__ per ray, a generator per ray ---
    def radiance_workspace_bytes(self, n: int, num_of_rays: int = 1, max_depth: int = 10, depth: int = 0) -> int:
        """Bytes of the node-stack workspace ``radiance(device=True)`` needs for ``n`` rays (``pt_rays_radiance_workspace_bytes``:
        sized by the lanes a launch keeps resident, not by ``n``)."""
        from . import _radiance_lib

        need = int(_radiance_lib.lib().pt_rays_radiance_workspace_bytes(self.device, int(n), int(num_of_rays), int(max_depth), int(depth)))
        if need == 0:
            raise ValueError(f"no workspace size for these arguments: {_radiance_lib.last_error()}")
        return need

    def radiance(self, rays, pcg, num_of_rays: int = 1, max_depth: int = 10, russian_roulette_limit: int = 3,
                 background=(0.0, 0.0, 0.0), depth: int = 0, channels="all", device: bool = False, stream=None, out=None,
                 workspace=None, n=None):
        """``PathTracer(world, background, pcg_i, num_of_rays, max_depth, russian_roulette_limit)(ray_i)`` (render.py:99-139) for
        every ray of the ``[8, n]`` block of :func:`pytracer_amd.rays.ray_planes`, with ``Ray.depth = depth`` and ``pcg``
        (``uint64[2, n]``: state and increment per ray, :func:`pytracer_amd.rays.pcg_streams`) its generator: each ray is walked
        depth-first on the device, in the reference's order of draws.  ``channels``: ``"pcg"``, ``"count"``, ``"all"``, ``"none"``
        or ``PT_RAD_*`` bits -> :class:`pytracer_amd.rays.RayRadiance`.  ``device=True``: ``rays`` is a ``DeviceBuffer`` or device
        tensor holding that block (or a raw address, then with ``n=``), ``pcg`` a buffer of ``[2, n]`` uint64 or a pair of plane
        addresses; the batch is enqueued on ``stream`` with the node stacks in ``workspace`` (:meth:`radiance_workspace_bytes`
        bytes of device memory; ``None``: a new buffer) -> the output ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _radiance_lib, rays as rb

        L, block, bits = _radiance_lib.lib(), self.kernel_args(), rb.radiance_channels(channels)
        par = _radiance_lib.params(num_of_rays, max_depth, russian_roulette_limit, depth, background)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if n is None:
                if not hasattr(rays, "nbytes"):
                    raise ValueError("n= is needed when the rays are a raw device address")
                n = int(rays.nbytes) // 64
            n = int(n)
            if isinstance(pcg, (tuple, list)):
                state, inc = pcg
            else:
                base = int(self._plane_ptr(pcg, "pcg").value or 0)
                state, inc = base, base + 8 * n
            if out is None:
                out = DeviceBuffer((max(rb.radiance_bytes(n, bits), 8),), np.uint8, self.device)
            if workspace is None and n > 0:
                # (0: arguments the library refuses -- the call below then says which, with its own error code)
                need = int(L.pt_rays_radiance_workspace_bytes(self.device, n, par.num_of_rays, par.max_depth, par.depth0))
                if need:
                    workspace = DeviceBuffer((need,), np.uint8, self.device)
                    out._radiance_workspace = workspace  # in flight on `stream` as long as the output is: freed with it
            ptr = self._plane_ptr
            _radiance_lib.check(L.pt_rays_radiance_device(self.device, block, len(block), None, ptr(rays, "rays"), ptr(state, "pcg state"),
                                                          ptr(inc, "pcg inc"), n, C.byref(par), bits, ptr(workspace, "workspace"),
                                                          int(workspace.nbytes) if workspace is not None else 0, ptr(out, "out"),
                                                          int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            if hasattr(workspace, "rendered_on"):
                workspace.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None or workspace is not None:
            raise ValueError("stream=, out=, workspace= and n= go with device=True (host batches are staged and synchronous)")
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        if rays.ndim != 2 or rays.shape[0] != 8:
            raise ValueError(f"rays must be the [8, n] block of pytracer_amd.rays.ray_planes, not {rays.shape}")
        n = rays.shape[1]
        gen = np.ascontiguousarray(pcg, dtype=np.uint64)
        if gen.shape != (2, n):
            raise ValueError(f"pcg must be uint64[2, {n}] (state and increment per ray: pytracer_amd.rays.pcg_streams), not {gen.shape}")
        buf = np.empty(rb.radiance_bytes(n, bits), dtype=np.uint8)
        _radiance_lib.check(L.pt_rays_radiance(self.device, block, len(block), rays.ctypes.data_as(C.c_void_p),
                                               gen[0].ctypes.data_as(C.c_void_p), gen[1].ctypes.data_as(C.c_void_p), n, C.byref(par), bits,
                                               buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return rb.RayRadiance(buf, n, bits)

    # -- the gather (include/ptrace_gather.h, libptrace_gather.so): mean hemisphere radiance per surface point, summed in sample order ---
    def gather_workspace_bytes(self, n: int, samples: int, num_of_rays: int = 1, max_depth: int = 10, depth: int = 0) -> int:
        """Bytes of the workspace ``gather(device=True)`` needs for ``n`` records of ``samples`` samples
        (``pt_rays_gather_workspace_bytes``: the node stacks, sized by the lanes a launch keeps resident, and four 8-byte planes of
        ``n * samples`` values for the samples' radiance and counts)."""
        from . import _gather_lib

        need = int(_gather_lib.lib().pt_rays_gather_workspace_bytes(self.device, int(n), int(samples), int(num_of_rays), int(max_depth),
                                                                    int(depth)))
        if need == 0:
            raise ValueError(f"no workspace size for these arguments: {_gather_lib.last_error()}")
        return need

    def gather(self, points, normals, samples: int, init_state: int = 42, seqs=None, active=None, num_of_rays: int = 1,
               max_depth: int = 10, russian_roulette_limit: int = 3, background=(0.0, 0.0, 0.0), depth: int = 0, channels="all",
               init_seq: int = 54, device: bool = False, stream=None, out=None, workspace=None, n=None):
        """Per record ``i`` of the planar ``[3, n]`` ``points`` and ``normals``: the mean over ``k < samples`` of
        ``PathTracer(world, background, g, num_of_rays, max_depth, russian_roulette_limit)(DiffuseBRDF.scatter_ray(g, ., p_i, n_i,
        depth))`` with ``g = PCG(init_state, seqs[i] + k)``, every sample on a lane of its own and the sum taken on the device
        strictly in ``k`` order (include/ptrace_gather.h).  ``seqs``: ``uint64[n]``, or ``None``: ``init_seq + i * samples``.
        ``active``: ``int32[n]`` (a ``shape_index`` plane as it is), negative = the record is skipped (radiance 0, count 0), or
        ``None``.  ``channels``: ``"count"``, ``"all"``, ``"none"`` or ``PT_GATHER_*`` bits -> :class:`pytracer_amd.rays.GatheredRadiance`.
        ``device=True``: ``points`` / ``normals`` (and ``seqs`` / ``active``) are ``DeviceBuffer`` s, device tensors or raw addresses
        (then with ``n=``); the batch is enqueued on ``stream`` with ``workspace`` (:meth:`gather_workspace_bytes` bytes of device
        memory; ``None``: a new buffer) -> the output ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _gather_lib, rays as rb

        L, block, bits = _gather_lib.lib(), self.kernel_args(), rb.gather_channels(channels)
        par = _gather_lib.params(samples, num_of_rays, max_depth, russian_roulette_limit, depth, init_state, init_seq, background)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if n is None:
                if not hasattr(points, "nbytes"):
                    raise ValueError("n= is needed when the points are a raw device address")
                n = int(points.nbytes) // 24
            n = int(n)
            if out is None:
                out = DeviceBuffer((max(rb.gather_bytes(n, bits), 8),), np.uint8, self.device)
            if workspace is None and n > 0:
                # (0: arguments the library refuses -- the call below then says which, with its own error code)
                need = int(L.pt_rays_gather_workspace_bytes(self.device, n, par.samples, par.num_of_rays, par.max_depth, par.depth0))
                if need:
                    workspace = DeviceBuffer((need,), np.uint8, self.device)
                    out._gather_workspace = workspace  # in flight on `stream` as long as the output is: freed with it
            ptr = self._plane_ptr
            _gather_lib.check(L.pt_rays_gather_device(self.device, block, len(block), ptr(points, "points"), ptr(normals, "normals"),
                                                      ptr(active, "active"), ptr(seqs, "seqs"), n, C.byref(par), bits,
                                                      ptr(workspace, "workspace"), int(workspace.nbytes) if workspace is not None else 0,
                                                      ptr(out, "out"), int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            if hasattr(workspace, "rendered_on"):
                workspace.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None or workspace is not None:
            raise ValueError("stream=, out=, workspace= and n= go with device=True (host batches are staged and synchronous)")
        points = np.ascontiguousarray(points, dtype=np.float64)
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        if points.ndim != 2 or points.shape[0] != 3 or normals.shape != points.shape:
            raise ValueError(f"points and normals must both be planar [3, n] (pytracer_amd.rays.planar), not {points.shape} and {normals.shape}")
        n = points.shape[1]
        if seqs is not None:
            seqs = rb.stream_numbers(seqs)
            if seqs.shape != (n,):
                raise ValueError(f"seqs must hold one stream number per record ({n}), not {seqs.shape}")
        if active is not None:
            active = np.ascontiguousarray(np.asarray(active).reshape(-1), dtype=np.int32)
            if active.shape != (n,):
                raise ValueError(f"active must hold one int32 per record ({n}), not {active.shape}")
        buf = np.empty(rb.gather_bytes(n, bits), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _gather_lib.check(L.pt_rays_gather(self.device, block, len(block), p(points), p(normals), p(active), p(seqs), n, C.byref(par), bits,
                                           p(buf), buf.nbytes))
        return rb.GatheredRadiance(buf, n, bits)

    # -- the bake (include/ptrace_bake.h, libptrace_bake.so): surface points from (shape, u, v), light maps over a (u, v) grid ---
    def surface_points(self, shape, uv, side=None, device: bool = False, stream=None, out=None, n=None):
        """The world point and the unit normal at ``(u, v)`` of a shape -- the inverse of the shapes' own ``(u, v)`` maps
        (shapes.py:36-42, 183-185), then ``Transformation.__mul__``, the normal normalised (include/ptrace_bake.h).  ``shape``:
        ``World.shapes`` indices (outside the scene: the record is zeros), ``uv``: ``[..., 2]``, ``side``: int32 per record
        (negative: the side the local normal points away from) or ``None`` (+1) -> ``[6, n]`` float64, point xyz then normal xyz:
        its halves are the ``points`` and ``normals`` of :meth:`gather`.  ``device=True``: ``shape`` (``n`` int32), ``uv`` (two
        planes of ``n`` doubles) and ``side`` are in HBM as for :meth:`surface`; the batch is enqueued on ``stream`` -> the output
        ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _bake_lib, rays as rb

        L, block = _bake_lib.lib(), self.kernel_args()
        if device:
            handle = getattr(stream, "handle", stream)
            n = self._device_count(shape, n)
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((6, max(n, 1)), np.float64, self.device)
            ptr = self._plane_ptr
            _bake_lib.check(L.pt_rays_surface_points_device(self.device, block, len(block), ptr(shape, "shape"), ptr(uv, "uv"),
                                                            ptr(side, "side"), n, ptr(out, "out"), int(out.nbytes),
                                                            C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None:
            raise ValueError("stream=, out= and n= go with device=True (host batches are staged and synchronous)")
        shape = np.ascontiguousarray(shape, dtype=np.int32).reshape(-1)
        n = shape.shape[0]
        uvp = rb.planar(uv, 2)
        if uvp.shape[1] != n:
            raise ValueError(f"{n} shape indices but {uvp.shape[1]} (u, v) pairs")
        if side is not None:
            side = np.ascontiguousarray(np.asarray(side).reshape(-1), dtype=np.int32)
            if side.shape != (n,):
                raise ValueError(f"side must hold one int32 per record ({n}), not {side.shape}")
        buf = np.empty((6, n), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _bake_lib.check(L.pt_rays_surface_points(self.device, block, len(block), p(shape), p(uvp), p(side), n, p(buf), buf.nbytes))
        return buf

    def bake_workspace_bytes(self, width: int, height: int, samples: int, num_of_rays: int = 1, max_depth: int = 10, depth: int = 1,
                             window=None) -> int:
        """Bytes of the workspace ``bake(device=True)`` needs for ``window`` (``(col0, row0, w, h)``; ``None``: the whole map) of a
        ``width x height`` map at ``samples`` samples (``pt_rays_bake_workspace_bytes``: the node stacks, sized by the lanes a launch
        keeps resident, and four 8-byte planes of ``w * h * samples`` values)."""
        from . import _bake_lib

        par = _bake_lib.params(0, 1, width, height, window, True, samples, num_of_rays, max_depth, 0, depth, 0, 0, (0.0, 0.0, 0.0))
        need = int(_bake_lib.lib().pt_rays_bake_workspace_bytes(self.device, C.byref(par)))
        if need == 0:
            raise ValueError(f"no workspace size for these arguments: {_bake_lib.last_error()}")
        return need

    def bake(self, shape: int, width: int, height: int, samples: int, side: int = 1, jitter: bool = True, window=None,
             init_state: int = 42, init_seq: int = 54, num_of_rays: int = 1, max_depth: int = 10, russian_roulette_limit: int = 3,
             background=(0.0, 0.0, 0.0), depth: int = 1, channels="all", device: bool = False, stream=None, out=None, workspace=None):
        """The light map of ``World.shapes[shape]``: per texel of ``window`` (``(col0, row0, w, h)``; ``None``: all) of its
        ``width x height`` grid over ``(u, v)`` the mean over ``k < samples`` of ``PathTracer(world, background, g, num_of_rays,
        max_depth, russian_roulette_limit)(DiffuseBRDF.scatter_ray(g, ., p, n, depth))`` with ``g = PCG(init_state, init_seq + t *
        samples + k)``, ``t`` the texel's index in the WHOLE map, and ``(p, n)`` the surface point at the texel's centre or
        (``jitter``) at a point of the texel drawn from ``g`` first; summed on the device strictly in ``k`` order
        (include/ptrace_bake.h).  ``channels``: ``"count"``, ``"all"``, ``"none"`` or ``PT_BAKE_*`` bits
        -> :class:`pytracer_amd.rays.BakedMap`.  ``device=True``: the bake is enqueued on ``stream`` with ``workspace``
        (:meth:`bake_workspace_bytes` bytes of device memory; ``None``: a new buffer) and stays in HBM -> the output
        ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _bake_lib, rays as rb

        L, block, bits = _bake_lib.lib(), self.kernel_args(), rb.bake_channels(channels)
        par = _bake_lib.params(shape, side, width, height, window, jitter, samples, num_of_rays, max_depth, russian_roulette_limit, depth,
                               init_state, init_seq, background)
        texels = max(par.w, 0) * max(par.h, 0)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((max(rb.bake_bytes(texels, bits), 8),), np.uint8, self.device)
            if workspace is None:
                # (0: arguments the library refuses -- the call below then says which, with its own error code)
                need = int(L.pt_rays_bake_workspace_bytes(self.device, C.byref(par)))
                if need:
                    workspace = DeviceBuffer((need,), np.uint8, self.device)
                    out._bake_workspace = workspace  # in flight on `stream` as long as the output is: freed with it
            ptr = self._plane_ptr
            _bake_lib.check(L.pt_rays_bake_device(self.device, block, len(block), C.byref(par), bits, ptr(workspace, "workspace"),
                                                  int(workspace.nbytes) if workspace is not None else 0, ptr(out, "out"), int(out.nbytes),
                                                  C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            if hasattr(workspace, "rendered_on"):
                workspace.rendered_on(stream)
            return out
        if stream is not None or out is not None or workspace is not None:
            raise ValueError("stream=, out= and workspace= go with device=True (host bakes are staged and synchronous)")
        buf = np.empty(max(rb.bake_bytes(texels, bits), 8), dtype=np.uint8)
        _bake_lib.check(L.pt_rays_bake(self.device, block, len(block), C.byref(par), bits, buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return rb.BakedMap(buf, par.w, par.h, bits)

    # -- the probes (include/ptrace_sh.h, libptrace_sh.so): order-2 SH coefficients of the radiance arriving at free points ---
    def sh_workspace_bytes(self, n: int, samples: int, num_of_rays: int = 1, max_depth: int = 10, depth: int = 1) -> int:
        """Bytes of the workspace ``sh_project(device=True)`` needs for ``n`` probes of ``samples`` samples
        (``pt_rays_sh_workspace_bytes``: the node stacks, sized by the lanes a launch keeps resident, and seven 8-byte planes of
        ``n * samples`` values for the samples' radiance, counts and directions)."""
        from . import _sh_lib

        par = _sh_lib.params(samples, num_of_rays, max_depth, 0, depth)
        need = int(_sh_lib.lib().pt_rays_sh_workspace_bytes(self.device, int(n), C.byref(par)))
        if need == 0:
            raise ValueError(f"no workspace size for these arguments: {_sh_lib.last_error()}")
        return need

    def sh_project(self, points, samples: int, init_state: int = 42, init_seq: int = 54, seqs=None, active=None, num_of_rays: int = 1,
                   max_depth: int = 10, russian_roulette_limit: int = 3, background=(0.0, 0.0, 0.0), depth: int = 1, channels="all",
                   device: bool = False, stream=None, out=None, workspace=None, n=None):
        """Per probe ``i`` of the planar ``[3, n]`` ``points``: the 27 order-2 spherical-harmonic coefficients of the radiance
        arriving there, ``c[j][ch] = (sum over k < samples, in k order, of Y_j(d_k) * L_k[ch]) * (4 pi / samples)`` with ``d_k``
        uniform on the sphere from ``g = PCG(init_state, seqs[i] + k)`` and ``L_k = PathTracer(world, background, g, num_of_rays,
        max_depth, russian_roulette_limit)(Ray(x_i, d_k, depth=depth))`` (include/ptrace_sh.h).  ``seqs``: ``uint64[n]``, or
        ``None``: ``init_seq + i * samples``.  ``active``: ``int32[n]``, negative = the probe is skipped (zeros, count 0), or
        ``None``.  ``channels``: ``"count"``, ``"all"``, ``"none"`` or ``PT_SH_*`` bits -> :class:`pytracer_amd.rays.ProbeSet`.
        ``device=True``: ``points`` (and ``seqs`` / ``active``) are ``DeviceBuffer`` s, device tensors or raw addresses (then with
        ``n=``); the batch is enqueued on ``stream`` with ``workspace`` (:meth:`sh_workspace_bytes` bytes of device memory;
        ``None``: a new buffer) -> the output ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _sh_lib, rays as rb

        L, block, bits = _sh_lib.lib(), self.kernel_args(), rb.sh_channels(channels)
        par = _sh_lib.params(samples, num_of_rays, max_depth, russian_roulette_limit, depth, init_state, init_seq, background)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if n is None:
                if not hasattr(points, "nbytes"):
                    raise ValueError("n= is needed when the points are a raw device address")
                n = int(points.nbytes) // 24
            n = int(n)
            if out is None:
                out = DeviceBuffer((max(rb.sh_bytes(n, bits), 8),), np.uint8, self.device)
            if workspace is None and n > 0:
                # (0: arguments the library refuses -- the call below then says which, with its own error code)
                need = int(L.pt_rays_sh_workspace_bytes(self.device, n, C.byref(par)))
                if need:
                    workspace = DeviceBuffer((need,), np.uint8, self.device)
                    out._sh_workspace = workspace  # in flight on `stream` as long as the output is: freed with it
            ptr = self._plane_ptr
            _sh_lib.check(L.pt_rays_sh_project_device(self.device, block, len(block), ptr(points, "points"), ptr(active, "active"),
                                                      ptr(seqs, "seqs"), n, C.byref(par), bits, ptr(workspace, "workspace"),
                                                      int(workspace.nbytes) if workspace is not None else 0, ptr(out, "out"),
                                                      int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            if hasattr(workspace, "rendered_on"):
                workspace.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None or workspace is not None:
            raise ValueError("stream=, out=, workspace= and n= go with device=True (host batches are staged and synchronous)")
        points = np.ascontiguousarray(points, dtype=np.float64)
        if points.ndim != 2 or points.shape[0] != 3:
            raise ValueError(f"points must be planar [3, n] (pytracer_amd.rays.planar), not {points.shape}")
        n = points.shape[1]
        seqs, active = self._sh_planes(seqs, active, n)
        buf = np.empty(max(rb.sh_bytes(n, bits), 8), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _sh_lib.check(L.pt_rays_sh_project(self.device, block, len(block), p(points), p(active), p(seqs), n, C.byref(par), bits, p(buf),
                                           buf.nbytes))
        return rb.ProbeSet(buf, n, bits, evaluator=self.sh_eval)

    @staticmethod
    def _sh_planes(seqs, active, n: int):
        from . import rays as rb

        if seqs is not None:
            seqs = rb.stream_numbers(seqs)
            if seqs.shape != (n,):
                raise ValueError(f"seqs must hold one stream number per probe ({n}), not {seqs.shape}")
        if active is not None:
            active = np.ascontiguousarray(np.asarray(active).reshape(-1), dtype=np.int32)
            if active.shape != (n,):
                raise ValueError(f"active must hold one int32 per probe ({n}), not {active.shape}")
        return seqs, active

    def sh_directions(self, n: int, samples: int, init_state: int = 42, init_seq: int = 54, seqs=None, device: bool = False, stream=None,
                      out=None):
        """The directions the probes' samples take: ``d_ik = D(PCG(init_state, seqs[i] + k))`` (include/ptrace_sh.h), made by the
        device function the projection uses -> planar ``[3, n * samples]`` float64, sample ``j = i * samples + k``.
        ``device=True``: ``seqs`` is in HBM (or ``None``), the batch is enqueued on ``stream`` -> the output ``DeviceBuffer``
        (``out``, or a new one)."""
        from . import _sh_lib

        L, n = _sh_lib.lib(), int(n)
        par = _sh_lib.params(samples, init_state=init_state, init_seq=init_seq)
        total = max(n, 0) * max(par.samples, 0)
        if device:
            handle = getattr(stream, "handle", stream)
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((3, max(total, 1)), np.float64, self.device)
            ptr = self._plane_ptr
            _sh_lib.check(L.pt_rays_sh_directions_device(self.device, ptr(seqs, "seqs"), n, C.byref(par), ptr(out, "out"), int(out.nbytes),
                                                         C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None:
            raise ValueError("stream= and out= go with device=True (host batches are staged and synchronous)")
        seqs, _ = self._sh_planes(seqs, None, n)
        buf = np.empty((3, total), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _sh_lib.check(L.pt_rays_sh_directions(self.device, p(seqs), n, C.byref(par), p(buf), max(buf.nbytes, 0)))
        return buf

    def sh_eval(self, coeffs, dirs, index=None, kind: int = 0, n=None, device: bool = False, stream=None, out=None, m=None):
        """Evaluate ``m`` records against the coefficient block ``coeffs`` (``[27, n]`` float64, plane ``3 j + ch``): per record the
        band-limited radiance towards ``dirs[:, r]`` (``kind=PT_SH_RADIANCE``, 0) or the cosine-weighted mean over the hemisphere
        around it (``PT_SH_HEMISPHERE``, 1), of probe ``index[r]`` (``None``: probe ``r``; outside ``[0, n)``: zeros) -> planar
        ``[3, m]`` float64.  ``dirs``: planar ``[3, m]``, used as they are (not normalised).  No scene is read.  ``device=True``:
        the planes are in HBM (with ``n=`` and ``m=`` where they are raw addresses), the batch is enqueued on ``stream`` -> the
        output ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _sh_lib

        L = _sh_lib.lib()
        if device:
            handle = getattr(stream, "handle", stream)
            if n is None:
                if not hasattr(coeffs, "nbytes"):
                    raise ValueError("n= is needed when the coefficients are a raw device address")
                n = int(coeffs.nbytes) // 216
            if m is None:
                if not hasattr(dirs, "nbytes"):
                    raise ValueError("m= is needed when the directions are a raw device address")
                m = int(dirs.nbytes) // 24
            n, m = int(n), int(m)
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            ptr = self._plane_ptr
            _sh_lib.check(L.pt_rays_sh_eval_device(self.device, ptr(coeffs, "coeffs"), n, ptr(index, "index"), ptr(dirs, "dirs"), m, int(kind),
                                                   ptr(out, "out"), int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None or m is not None:
            raise ValueError("stream=, out=, n= and m= go with device=True (host batches are staged and synchronous)")
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64)
        if coeffs.ndim != 2 or coeffs.shape[0] != 27:
            raise ValueError(f"coeffs must be the [27, n] block of a probe set, not {coeffs.shape}")
        if dirs.ndim != 2 or dirs.shape[0] != 3:
            raise ValueError(f"dirs must be planar [3, m] (pytracer_amd.rays.planar), not {dirs.shape}")
        n, m = coeffs.shape[1], dirs.shape[1]
        if index is not None:
            index = np.asarray(index).reshape(-1)
            index = np.ascontiguousarray(np.where((index < 0) | (index >= 2 ** 31), -1, index), dtype=np.int32)  # (no wrap into range)
            if index.shape != (m,):
                raise ValueError(f"index must hold one int32 per record ({m}), not {index.shape}")
        buf = np.empty((3, m), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _sh_lib.check(L.pt_rays_sh_eval(self.device, p(coeffs), n, p(index), p(dirs), m, int(kind), p(buf), buf.nbytes))
        return buf

    # -- lit queries (include/ptrace_lit.h, libptrace_lit.so): records shaded from a lattice of probes ---------------------------
    @staticmethod
    def _lit_grid(grid):
        """``(pt_lit_grid, n)`` from a :class:`pytracer_amd.rays.ProbeGrid` (anything with ``origin``, ``step`` and ``dims``)."""
        from . import _lit_lib

        g = _lit_lib.grid(grid.origin, grid.step, grid.dims)
        return g, int(g.dims[0]) * int(g.dims[1]) * int(g.dims[2])

    def lit_eval(self, grid, coeffs, points, dirs, active=None, kind: int = 0, device: bool = False, stream=None, out=None, m=None):
        """Per record the coefficients of the eight probes of ``grid`` around ``points[:, r]``, blended by trilinear weights
        (``ProbeGrid.corners`` / ``blend``) and evaluated towards ``dirs[:, r]`` (``kind``: ``PT_SH_RADIANCE`` 0 or
        ``PT_SH_HEMISPHERE`` 1), in one kernel -> planar ``[3, m]`` float64.  ``coeffs``: the ``[27, n]`` block of the lattice's
        probes; ``points``, ``dirs``: planar ``[3, m]``; ``active``: optional int32, negative = zeros.  A NaN point gives zeros.
        No scene is read.  ``device=True``: the planes are in HBM (with ``m=`` where they are raw addresses), the batch is enqueued
        on ``stream`` -> the output ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _lit_lib

        L = _lit_lib.lib()
        g, n = self._lit_grid(grid)
        if device:
            handle = getattr(stream, "handle", stream)
            if m is None:
                if not hasattr(points, "nbytes"):
                    raise ValueError("m= is needed when the points are a raw device address")
                m = int(points.nbytes) // 24
            m = int(m)
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            ptr = self._plane_ptr
            co_bytes = int(coeffs.nbytes) if hasattr(coeffs, "nbytes") else 216 * n
            _lit_lib.check(L.pt_rays_lit_eval_device(self.device, C.byref(g), ptr(coeffs, "coeffs"), co_bytes, ptr(points, "points"),
                                                     ptr(dirs, "dirs"), ptr(active, "active"), m, int(kind), ptr(out, "out"), int(out.nbytes),
                                                     C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None or m is not None:
            raise ValueError("stream=, out= and m= go with device=True (host batches are staged and synchronous)")
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        points = np.ascontiguousarray(points, dtype=np.float64)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64)
        if coeffs.ndim != 2 or coeffs.shape[0] != 27:
            raise ValueError(f"coeffs must be the [27, n] block of a probe set, not {coeffs.shape}")
        if points.ndim != 2 or points.shape[0] != 3 or dirs.shape != points.shape:
            raise ValueError(f"points and dirs must be planar [3, m] (pytracer_amd.rays.planar), not {points.shape} and {dirs.shape}")
        m = points.shape[1]
        if active is not None:
            active = np.ascontiguousarray(np.asarray(active).reshape(-1), dtype=np.int32)
            if active.shape != (m,):
                raise ValueError(f"active must hold one int32 per record ({m}), not {active.shape}")
        buf = np.empty((3, m), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _lit_lib.check(L.pt_rays_lit_eval(self.device, C.byref(g), p(coeffs), coeffs.nbytes, p(points), p(dirs), p(active), m, int(kind), p(buf),
                                          buf.nbytes))
        return buf

    def lit_shade(self, grid, coeffs, shape_index, point, normal, uv, dirs, background=(0.0, 0.0, 0.0), device: bool = False, stream=None,
                  out=None, n=None):
        """Every hit record shaded from the lattice ``grid`` of probes ``coeffs`` (``[27, n_probes]``): ``background`` where nothing
        was hit, else ``emitted(uv) + brdf_color(uv) * E`` with ``E`` the blend at ``point`` evaluated as the cosine-weighted
        hemisphere mean around the unit normal (``DiffuseBRDF``) or as the radiance from the mirror direction (``SpecularBRDF``)
        -- :func:`pytracer_amd.rays.lit_shade_host` on the device, in one kernel.  ``point``, ``normal``, ``dirs``: ``[..., 3]``,
        ``uv``: ``[..., 2]``, ``dirs`` the directions of the rays that were traced -> ``[n, 3]`` float64 (a view of the three planes
        the library wrote).  ``device=True``: planes in HBM as for :meth:`shade_lights` (a hit frame's own, with ``n=``); -> the
        output ``DeviceBuffer`` of ``[3, n]`` float64."""
        from . import _lit_lib, rays as rb

        L, block = _lit_lib.lib(), self.kernel_args()
        g, n_probes = self._lit_grid(grid)
        bg = _lit_lib.rgb(background)
        if device:
            handle = getattr(stream, "handle", stream)
            n = self._device_count(shape_index, n)
            if out is None:
                from .devmem import DeviceBuffer

                out = DeviceBuffer((3, max(n, 1)), np.float64, self.device)
            ptr = self._plane_ptr
            slots = self.slot_table()
            co_bytes = int(coeffs.nbytes) if hasattr(coeffs, "nbytes") else 216 * n_probes
            _lit_lib.check(L.pt_rays_lit_shade_device(self.device, block, len(block), C.c_void_p(slots.data_ptr()), int(slots.nbytes), C.byref(g),
                                                      ptr(coeffs, "coeffs"), co_bytes, ptr(shape_index, "shape_index"), ptr(point, "point"),
                                                      ptr(normal, "normal"), ptr(uv, "uv"), ptr(dirs, "dirs"), n, bg, ptr(out, "out"),
                                                      int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None:
            raise ValueError("stream=, out= and n= go with device=True (host batches are staged and synchronous)")
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        if coeffs.ndim != 2 or coeffs.shape[0] != 27:
            raise ValueError(f"coeffs must be the [27, n] block of a probe set, not {coeffs.shape}")
        shape = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        n = shape.shape[0]
        planes = [rb.planar(point, 3), rb.planar(normal, 3), rb.planar(uv, 2), rb.planar(dirs, 3)]
        if any(p.shape[1] != n for p in planes):
            raise ValueError(f"{n} shape indices but {[p.shape[1] for p in planes]} points, normals, (u, v) pairs and directions")
        buf = np.empty((3, n), dtype=np.float64)
        _lit_lib.check(L.pt_rays_lit_shade(self.device, block, len(block), C.byref(g), coeffs.ctypes.data_as(C.c_void_p), coeffs.nbytes,
                                           shape.ctypes.data_as(C.c_void_p), *[p.ctypes.data_as(C.c_void_p) for p in planes], n, bg,
                                           buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return buf.T

    # -- denoise queries (include/ptrace_denoise.h, libptrace_denoise.so): an edge-avoiding filter for noisy frames ---------------
    def denoise_workspace_bytes(self, width: int, height: int, **params) -> int:
        """Bytes of the workspace :meth:`denoise` needs on the device for a ``width x height`` frame (``params``: its own)."""
        from . import _denoise_lib

        L, par = _denoise_lib.lib(), _denoise_lib.params(**params)
        need = int(L.pt_rays_denoise_workspace_bytes(_denoise_lib._addon.c_int(width, "width"), _denoise_lib._addon.c_int(height, "height"), C.byref(par)))
        if need == 0 and int(width) * int(height) != 0:
            raise _lib.PtraceError(-1, _denoise_lib.last_error())
        return need

    def denoise(self, colour, shape_index, normal, point, width: int, height: int, device: bool = False, stream=None, out=None,
                workspace=None, **params):
        """The edge-avoiding a-trous filter of include/ptrace_denoise.h over a ``width x height`` frame: ``passes`` passes of a 5x5
        B3 stencil with the steps 1, 2, 4, ..., every tap weighted by the guides -- skipped on another shape (``same_shape``), cut by
        the angle between the unit normals (``cos^(2^normal_power_log2)``), by the distance from the centre's tangent plane
        (``sigma_point``, per step) and optionally by the colour difference (``sigma_colour``); ``wrap_x`` joins the first and the
        last column.  ``colour``, ``normal``, ``point``: ``[..., 3]`` with ``width * height`` records, ``shape_index``: int32,
        negative = copied -> ``[height, width, 3]`` float64, :func:`pytracer_amd.rays.denoise_host` in every bit.  No scene is read.
        ``device=True``: the planes (``[3, m]`` fp64, int32) are in HBM, the passes are enqueued on ``stream`` -> the output
        ``DeviceBuffer`` (``out``, or a new one); ``workspace``: a ``DeviceBuffer`` of :meth:`denoise_workspace_bytes` (or a new one)."""
        from . import _denoise_lib, rays as rb

        L, par = _denoise_lib.lib(), _denoise_lib.params(**params)
        width, height = _denoise_lib._addon.c_int(width, "width"), _denoise_lib._addon.c_int(height, "height")
        m = width * height
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if workspace is None:
                workspace = DeviceBuffer((max(self.denoise_workspace_bytes(width, height, **params), 8),), np.uint8, self.device)
            ptr = self._plane_ptr
            _denoise_lib.check(L.pt_rays_denoise_device(self.device, width, height, C.byref(par), ptr(colour, "colour"), ptr(normal, "normal"),
                                                        ptr(point, "point"), ptr(shape_index, "shape_index"), ptr(out, "out"), int(out.nbytes),
                                                        ptr(workspace, "workspace"), int(workspace.nbytes), C.c_void_p(handle) if handle else None))
            for buf in (out, workspace):
                if hasattr(buf, "rendered_on"):
                    buf.rendered_on(stream)
            if hasattr(out, "rendered_on"):
                out._denoise_workspace = workspace  # in flight on `stream` as long as the output is: freed with it
            return out
        if stream is not None or out is not None or workspace is not None:
            raise ValueError("stream=, out= and workspace= go with device=True (host frames are staged and synchronous)")
        shape = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        planes = [rb.planar(colour, 3), rb.planar(normal, 3), rb.planar(point, 3)]
        if shape.shape[0] != m or any(p.shape[1] != m for p in planes):
            raise ValueError(f"a {width} x {height} frame has {m} records, not {shape.shape[0]} shape indices and "
                             f"{[p.shape[1] for p in planes]} colours, normals and points")
        buf = np.empty((3, m), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _denoise_lib.check(L.pt_rays_denoise(self.device, width, height, C.byref(par), p(planes[0]), p(planes[1]), p(planes[2]), p(shape), p(buf),
                                             buf.nbytes))
        return np.ascontiguousarray(buf.T).reshape(height, width, 3)

    # -- accumulate queries (include/ptrace_temporal.h, libptrace_temporal.so): last frame's radiance on this frame's hits --------
    def temporal(self, colour, shape_index, normal, point, prev_colour, prev_shape, prev_normal, prev_point, prev_count, prev_camera,
                 width: int, height: int, device: bool = False, stream=None, out=None, out_count=None, **params):
        """The accumulation of include/ptrace_temporal.h over a ``width x height`` frame: every hit point of this frame is projected
        onto the screen of ``prev_camera`` (a camera object, ``(kind, invm12, screen_distance, aspect_ratio)`` or a
        ``TemporalCamera``), the previous frame's colour is fetched there from up to four taps -- a tap is skipped without history
        (``prev_count <= 0``), on another shape (``same_shape``), where the unit normals' cosine is below ``normal_min`` or the tap's
        point lies more than ``point_tolerance`` from this pixel's tangent plane -- and blended with ``colour``: a running mean up to
        ``max_history`` frames, an exponential average from there.  ``colour``, ``normal``, ``point`` (and the previous frame's):
        ``[..., 3]`` with ``width * height`` records; ``shape_index``, ``prev_shape``, ``prev_count``: int32 ->
        ``(out [height, width, 3] float64, count [height, width] int32)``, :func:`pytracer_amd.rays.temporal_host` in every bit.
        No scene is read.  ``device=True``: the planes (``[3, m]`` fp64, int32) are in HBM, the one launch is enqueued on ``stream``
        -> the two output ``DeviceBuffer`` s (``out`` and ``out_count``, or new ones); neither may overlap an input."""
        from . import _temporal_lib, rays as rb

        L, par, cam = _temporal_lib.lib(), _temporal_lib.params(**params), _temporal_lib.camera(prev_camera)
        width, height = _temporal_lib._addon.c_int(width, "width"), _temporal_lib._addon.c_int(height, "height")
        m = width * height
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if out_count is None:
                out_count = DeviceBuffer((max(m, 1),), np.int32, self.device)
            ptr = self._plane_ptr
            _temporal_lib.check(L.pt_rays_temporal_accumulate_device(
                self.device, width, height, C.byref(par), C.byref(cam), ptr(colour, "colour"), ptr(shape_index, "shape_index"),
                ptr(normal, "normal"), ptr(point, "point"), ptr(prev_colour, "prev_colour"), ptr(prev_shape, "prev_shape"),
                ptr(prev_normal, "prev_normal"), ptr(prev_point, "prev_point"), ptr(prev_count, "prev_count"), ptr(out, "out"),
                int(out.nbytes), ptr(out_count, "out_count"), int(out_count.nbytes), C.c_void_p(handle) if handle else None))
            for buf in (out, out_count):
                if hasattr(buf, "rendered_on"):
                    buf.rendered_on(stream)
            return out, out_count
        if stream is not None or out is not None or out_count is not None:
            raise ValueError("stream=, out= and out_count= go with device=True (host frames are staged and synchronous)")
        ints = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (shape_index, prev_shape, prev_count)]
        planes = [rb.planar(a, 3) for a in (colour, normal, point, prev_colour, prev_normal, prev_point)]
        if any(a.shape[0] != m for a in ints) or any(p.shape[1] != m for p in planes):
            raise ValueError(f"a {width} x {height} frame has {m} records, not {[a.shape[0] for a in ints]} shape indices and counts and "
                             f"{[p.shape[1] for p in planes]} colours, normals and points")
        buf, cnt = np.empty((3, m), dtype=np.float64), np.empty((m,), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _temporal_lib.check(L.pt_rays_temporal_accumulate(self.device, width, height, C.byref(par), C.byref(cam), p(planes[0]), p(ints[0]),
                                                          p(planes[1]), p(planes[2]), p(planes[3]), p(ints[1]), p(planes[4]), p(planes[5]),
                                                          p(ints[2]), p(buf), buf.nbytes, p(cnt), cnt.nbytes))
        return np.ascontiguousarray(buf.T).reshape(height, width, 3), cnt.reshape(height, width)

    def temporal_clear(self, count, m=None, stream=None):
        """An empty history: the ``m`` int32 lengths of the device buffer ``count`` (default: all it holds) become 0 on ``stream``
        (``pt_rays_temporal_clear_device``) -> ``count``."""
        from . import _temporal_lib

        handle = getattr(stream, "handle", stream)
        m = self._device_count(count, m)
        nbytes = int(count.nbytes) if hasattr(count, "nbytes") else 4 * m
        _temporal_lib.check(_temporal_lib.lib().pt_rays_temporal_clear_device(self.device, m, self._plane_ptr(count, "count"), nbytes,
                                                                              C.c_void_p(handle) if handle else None))
        if hasattr(count, "rendered_on"):
            count.rendered_on(stream)
        return count

    # -- weighted accumulate queries (include/ptrace_weighted.h, libptrace_weighted.so): frames count by the samples they took -------
    def weighted(self, colour, samples, shape_index, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count,
                 prev_camera, width: int, height: int, device: bool = False, stream=None, out=None, out_moments=None, out_count=None, **params):
        """The accumulation of include/ptrace_weighted.h over a ``width x height`` frame: the taps of :meth:`temporal` found once, and
        from them the colour, the luminance moments ``(M1, M2)`` and the accumulated weight ``S`` blended with this frame's, whose
        weight is ``samples`` (int32 per record; ``None``: one everywhere; 0 or less: nothing was sampled there and the reprojected
        history is carried).  ``prev_moments``: ``[..., 3]`` = (M1, M2, S) of the previous frame.  ``params``: ``max_history``,
        ``max_weight`` (the cap of the history's weight, inf: none), ``blend_weight`` (the history's weight is the taps' blend, not
        their largest), ``same_shape``, ``normal_min``, ``point_tolerance`` -> ``(out [height, width, 3], moments [height, width, 3],
        count [height, width] int32)``, :func:`pytracer_amd.rays.weighted_host` in every bit; ``moments`` and ``count`` are what
        :meth:`variance_estimate` reads.  No scene is read.  ``device=True``: the planes (``[3, m]`` fp64, int32) are in HBM --
        ``samples`` may be the address of the ``TAKEN`` plane of a ragged gather -- the one launch is enqueued on ``stream`` -> the
        three output ``DeviceBuffer`` s (``out``, ``out_moments`` and ``out_count``, or new ones); none may overlap an input."""
        from . import _weighted_lib, rays as rb

        L, par, cam = _weighted_lib.lib(), _weighted_lib.params(**params), _weighted_lib.camera(prev_camera)
        width, height = _weighted_lib._addon.c_int(width, "width"), _weighted_lib._addon.c_int(height, "height")
        m = width * height
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if out_moments is None:
                out_moments = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if out_count is None:
                out_count = DeviceBuffer((max(m, 1),), np.int32, self.device)
            ptr = self._plane_ptr
            _weighted_lib.check(L.pt_rays_weighted_accumulate_device(
                self.device, width, height, C.byref(par), C.byref(cam), ptr(colour, "colour"), ptr(samples, "samples"),
                ptr(shape_index, "shape_index"), ptr(normal, "normal"), ptr(point, "point"), ptr(prev_colour, "prev_colour"),
                ptr(prev_moments, "prev_moments"), ptr(prev_shape, "prev_shape"), ptr(prev_normal, "prev_normal"), ptr(prev_point, "prev_point"),
                ptr(prev_count, "prev_count"), ptr(out, "out"), int(out.nbytes), ptr(out_moments, "out_moments"), int(out_moments.nbytes),
                ptr(out_count, "out_count"), int(out_count.nbytes), C.c_void_p(handle) if handle else None))
            for buf in (out, out_moments, out_count):
                if hasattr(buf, "rendered_on"):
                    buf.rendered_on(stream)
            return out, out_moments, out_count
        if stream is not None or out is not None or out_moments is not None or out_count is not None:
            raise ValueError("stream=, out=, out_moments= and out_count= go with device=True (host frames are staged and synchronous)")
        ints = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (shape_index, prev_shape, prev_count)]
        taken = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32).reshape(-1)
        planes = [rb.planar(a, 3) for a in (colour, normal, point, prev_colour, prev_moments, prev_normal, prev_point)]
        if any(a.shape[0] != m for a in ints) or any(p.shape[1] != m for p in planes) or (taken is not None and taken.shape[0] != m):
            raise ValueError(f"a {width} x {height} frame has {m} records, not {[a.shape[0] for a in ints]} shape indices and counts, "
                             f"{None if taken is None else taken.shape[0]} sample counts and {[p.shape[1] for p in planes]} colours, normals, "
                             "points and moments")
        buf, mom, cnt = np.empty((3, m), dtype=np.float64), np.empty((3, m), dtype=np.float64), np.empty((m,), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _weighted_lib.check(L.pt_rays_weighted_accumulate(self.device, width, height, C.byref(par), C.byref(cam), p(planes[0]), p(taken), p(ints[0]),
                                                          p(planes[1]), p(planes[2]), p(planes[3]), p(planes[4]), p(ints[1]), p(planes[5]),
                                                          p(planes[6]), p(ints[2]), p(buf), buf.nbytes, p(mom), mom.nbytes, p(cnt), cnt.nbytes))
        return (np.ascontiguousarray(buf.T).reshape(height, width, 3), np.ascontiguousarray(mom.T).reshape(height, width, 3),
                cnt.reshape(height, width))

    def weighted_clear(self, count, m=None, stream=None):
        """An empty history: the ``m`` int32 lengths of the device buffer ``count`` (default: all it holds) become 0 on ``stream``
        (``pt_rays_weighted_clear_device``) -> ``count``.  With lengths of 0 no colour, moment or weight of the history is read."""
        from . import _weighted_lib

        handle = getattr(stream, "handle", stream)
        m = self._device_count(count, m)
        nbytes = int(count.nbytes) if hasattr(count, "nbytes") else 4 * m
        _weighted_lib.check(_weighted_lib.lib().pt_rays_weighted_clear_device(self.device, m, self._plane_ptr(count, "count"), nbytes,
                                                                              C.c_void_p(handle) if handle else None))
        if hasattr(count, "rendered_on"):
            count.rendered_on(stream)
        return count

    # -- motion accumulate queries (include/ptrace_motion.h, libptrace_motion.so): histories follow the shapes that moved ----------------
    def motion(self, colour, samples, shape_index, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count,
               prev_camera, moved, motion, width: int, height: int, device: bool = False, stream=None, out=None, out_moments=None, out_count=None,
               n_shapes=None, **params):
        """:meth:`weighted` with a motion per shape (include/ptrace_motion.h): a record whose shape index ``s`` has ``moved[s] != 0``
        is carried into the PREVIOUS frame's world -- its point by the affine map ``motion[s][0:12]``, its normal by the 3 x 3
        ``motion[s][12:21]`` -- before it is projected onto the previous screen and tested against the taps, so the history of a shape
        that moved is fetched where that surface point was.  ``moved``: int32 per shape, ``motion``: ``[S, 24]`` fp64, as
        ``rays.shape_motion`` returns them; ``None`` for both: nothing moved, and every bit is :meth:`weighted`'s.  A shape index at
        or beyond ``S`` is a static shape.  Everything else as :meth:`weighted` takes and returns it;
        :func:`pytracer_amd.rays.motion_host` in every bit.  No scene is read.  ``device=True``: the planes and both tables are in
        HBM (:meth:`motion_table` uploads the tables; raw addresses need ``n_shapes=``), the one launch is enqueued on ``stream``;
        no output may overlap an input or a table."""
        from . import _motion_lib, rays as rb

        L, par, cam = _motion_lib.lib(), _motion_lib.params(**params), _motion_lib.camera(prev_camera)
        width, height = _motion_lib._addon.c_int(width, "width"), _motion_lib._addon.c_int(height, "height")
        m = width * height
        if device:
            from .devmem import DeviceBuffer

            if (moved is None) != (motion is None):
                raise ValueError("moved and motion come together (or neither: nothing moved)")
            if n_shapes is None:
                if moved is None:
                    n_shapes = 0
                elif hasattr(moved, "nbytes"):
                    n_shapes = int(moved.nbytes) // 4
                elif callable(getattr(moved, "numel", None)):
                    n_shapes = int(moved.numel())
                else:
                    raise ValueError("n_shapes= is needed when the tables are raw device addresses")
            n_shapes = _motion_lib._addon.c_int(n_shapes, "n_shapes")
            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if out_moments is None:
                out_moments = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if out_count is None:
                out_count = DeviceBuffer((max(m, 1),), np.int32, self.device)
            ptr = self._plane_ptr
            _motion_lib.check(L.pt_rays_motion_accumulate_device(
                self.device, width, height, C.byref(par), C.byref(cam), ptr(colour, "colour"), ptr(samples, "samples"),
                ptr(shape_index, "shape_index"), ptr(normal, "normal"), ptr(point, "point"), ptr(prev_colour, "prev_colour"),
                ptr(prev_moments, "prev_moments"), ptr(prev_shape, "prev_shape"), ptr(prev_normal, "prev_normal"), ptr(prev_point, "prev_point"),
                ptr(prev_count, "prev_count"), n_shapes, ptr(moved, "moved"), ptr(motion, "motion"), ptr(out, "out"), int(out.nbytes),
                ptr(out_moments, "out_moments"), int(out_moments.nbytes), ptr(out_count, "out_count"), int(out_count.nbytes),
                C.c_void_p(handle) if handle else None))
            for buf in (out, out_moments, out_count):
                if hasattr(buf, "rendered_on"):
                    buf.rendered_on(stream)
            return out, out_moments, out_count
        if stream is not None or out is not None or out_moments is not None or out_count is not None or n_shapes is not None:
            raise ValueError("stream=, out=, out_moments=, out_count= and n_shapes= go with device=True (host frames are staged and synchronous)")
        n_shapes, moved, motion = _motion_lib.tables(moved, motion)
        ints = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (shape_index, prev_shape, prev_count)]
        taken = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32).reshape(-1)
        planes = [rb.planar(a, 3) for a in (colour, normal, point, prev_colour, prev_moments, prev_normal, prev_point)]
        if any(a.shape[0] != m for a in ints) or any(p.shape[1] != m for p in planes) or (taken is not None and taken.shape[0] != m):
            raise ValueError(f"a {width} x {height} frame has {m} records, not {[a.shape[0] for a in ints]} shape indices and counts, "
                             f"{None if taken is None else taken.shape[0]} sample counts and {[p.shape[1] for p in planes]} colours, normals, "
                             "points and moments")
        buf, mom, cnt = np.empty((3, m), dtype=np.float64), np.empty((3, m), dtype=np.float64), np.empty((m,), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _motion_lib.check(L.pt_rays_motion_accumulate(self.device, width, height, C.byref(par), C.byref(cam), p(planes[0]), p(taken), p(ints[0]),
                                                      p(planes[1]), p(planes[2]), p(planes[3]), p(planes[4]), p(ints[1]), p(planes[5]),
                                                      p(planes[6]), p(ints[2]), n_shapes, p(moved), p(motion), p(buf), buf.nbytes, p(mom),
                                                      mom.nbytes, p(cnt), cnt.nbytes))
        return (np.ascontiguousarray(buf.T).reshape(height, width, 3), np.ascontiguousarray(mom.T).reshape(height, width, 3),
                cnt.reshape(height, width))

    def motion_table(self, moved, motion):
        """The two tables of :meth:`motion` uploaded to this scene's device -> ``(moved, motion)`` as device tensors (int32 ``[S]``
        and fp64 ``[S, 24]``; the allocator aligns them beyond the 64 bytes a record wants), complete when this returns, for
        ``device=True`` calls on any stream.  The upload goes through PyTorch-ROCm, which the project uses for such plumbing: the
        C-ABI has no host-to-device copy of its own.  ``S = 0`` -> ``(None, None)``: nothing moved."""
        from . import _motion_lib

        n_shapes, moved, motion = _motion_lib.tables(moved, motion)
        if n_shapes == 0:
            return None, None
        if n_shapes > _motion_lib.MAX_SHAPES:
            raise ValueError(f"n_shapes={n_shapes}: 0 to 2^20")
        import torch

        where = torch.device("cuda", self.device)
        return torch.from_numpy(moved.copy()).to(where), torch.from_numpy(motion.copy()).to(where)

    def motion_clear(self, count, m=None, stream=None):
        """An empty history: the ``m`` int32 lengths of the device buffer ``count`` (default: all it holds) become 0 on ``stream``
        (``pt_rays_motion_clear_device``) -> ``count``.  With lengths of 0 no colour, moment or weight of the history is read."""
        from . import _motion_lib

        handle = getattr(stream, "handle", stream)
        m = self._device_count(count, m)
        nbytes = int(count.nbytes) if hasattr(count, "nbytes") else 4 * m
        _motion_lib.check(_motion_lib.lib().pt_rays_motion_clear_device(self.device, m, self._plane_ptr(count, "count"), nbytes,
                                                                        C.c_void_p(handle) if handle else None))
        if hasattr(count, "rendered_on"):
            count.rendered_on(stream)
        return count

    # -- gradient accumulate queries (include/ptrace_gradient.h, libptrace_gradient.so): histories shorten where the light changed ------
    def gradient_probes(self, shape_index, normal, point, moved, motion, width: int, height: int, stratum: int = 3, phase: int = 0,
                        samples: int = 1, init_seq: int = 54, device: bool = False, stream=None, out=None, n_shapes=None):
        """The probes of a ``width x height`` frame (include/ptrace_gradient.h): one per ``stratum x stratum`` block, at the pixel the
        hash of ``(phase, block)`` picks, carried into the PREVIOUS world by the tables of :meth:`motion` -> ``(probe_index int32[ns],
        probe_point [ns, 3], probe_normal [ns, 3], probe_seq uint64[ns])``, :func:`pytracer_amd.rays.gradient_probes_host` in every
        bit.  They are what :meth:`gather` takes as ``active``, ``points``, ``normals`` and ``seqs`` -- on the previous frame's scene,
        with this frame's ``samples`` and ``init_seq``.  No scene is read.  ``device=True``: the planes and tables are in HBM, the one
        launch is enqueued on ``stream`` -> four ``DeviceBuffer`` s (``out``: a tuple of four, or new ones), index ``[ns]``, point
        and normal planar ``[3, ns]``, seq ``[ns]``."""
        from . import _gradient_lib, rays as rb

        L = _gradient_lib.lib()
        width, height = _gradient_lib._addon.c_int(width, "width"), _gradient_lib._addon.c_int(height, "height")
        stratum, samples = _gradient_lib._addon.c_int(stratum, "stratum"), _gradient_lib._addon.c_int(samples, "samples")
        phase, init_seq = int(phase) & (2 ** 64 - 1), int(init_seq) & (2 ** 64 - 1)
        m = width * height
        ns = int(L.pt_rays_gradient_strata(width, height, stratum))
        if device:
            from .devmem import DeviceBuffer

            if (moved is None) != (motion is None):
                raise ValueError("moved and motion come together (or neither: nothing moved)")
            if n_shapes is None:
                if moved is None:
                    n_shapes = 0
                elif hasattr(moved, "nbytes"):
                    n_shapes = int(moved.nbytes) // 4
                elif callable(getattr(moved, "numel", None)):
                    n_shapes = int(moved.numel())
                else:
                    raise ValueError("n_shapes= is needed when the tables are raw device addresses")
            n_shapes = _gradient_lib._addon.c_int(n_shapes, "n_shapes")
            handle = getattr(stream, "handle", stream)
            if out is None:
                out = (DeviceBuffer((max(ns, 1),), np.int32, self.device), DeviceBuffer((3, max(ns, 1)), np.float64, self.device),
                       DeviceBuffer((3, max(ns, 1)), np.float64, self.device), DeviceBuffer((max(ns, 1),), np.uint64, self.device))
            ptr = self._plane_ptr
            _gradient_lib.check(L.pt_rays_gradient_probes_device(
                self.device, width, height, stratum, phase, samples, init_seq, ptr(shape_index, "shape_index"), ptr(normal, "normal"),
                ptr(point, "point"), n_shapes, ptr(moved, "moved"), ptr(motion, "motion"), ptr(out[0], "probe_index"), int(out[0].nbytes),
                ptr(out[1], "probe_point"), int(out[1].nbytes), ptr(out[2], "probe_normal"), int(out[2].nbytes), ptr(out[3], "probe_seq"),
                int(out[3].nbytes), C.c_void_p(handle) if handle else None))
            for buf in out:
                if hasattr(buf, "rendered_on"):
                    buf.rendered_on(stream)
            return out
        if stream is not None or out is not None or n_shapes is not None:
            raise ValueError("stream=, out= and n_shapes= go with device=True (host frames are staged and synchronous)")
        n_shapes, moved, motion = _gradient_lib.tables(moved, motion)
        sh = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        planes = [rb.planar(a, 3) for a in (normal, point)]
        if sh.shape[0] != m or any(p.shape[1] != m for p in planes):
            raise ValueError(f"a {width} x {height} frame has {m} records, not {sh.shape[0]} shape indices and {[p.shape[1] for p in planes]} "
                             "normals and points")
        index, pts, nrm, seq = np.empty(ns, np.int32), np.empty((3, ns)), np.empty((3, ns)), np.empty(ns, np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _gradient_lib.check(L.pt_rays_gradient_probes(self.device, width, height, stratum, phase, samples, init_seq, p(sh), p(planes[0]),
                                                      p(planes[1]), n_shapes, p(moved), p(motion), p(index), index.nbytes, p(pts), pts.nbytes,
                                                      p(nrm), nrm.nbytes, p(seq), seq.nbytes))
        return index, np.ascontiguousarray(pts.T), np.ascontiguousarray(nrm.T), seq

    def gradient_keep(self, colour, shape_index, probe_index, probe_old, width: int, height: int, device: bool = False, stream=None, out=None,
                      **params):
        """The share of its history every pixel of a ``width x height`` frame keeps (include/ptrace_gradient.h): from this frame's
        ``colour`` at the probes' pixels and ``probe_old``, the probes' gather in the previous world, over the ``(2 radius + 1)^2``
        strata around the pixel.  ``params``: ``stratum``, ``radius``, ``gain``, ``same_shape_probes`` -> ``keep [height, width]``
        float64 in [0, 1], :func:`pytracer_amd.rays.gradient_keep_host` in every bit.  No scene is read.  ``device=True``: the planes
        are in HBM (``colour`` and ``probe_old`` planar), the one launch is enqueued on ``stream`` -> the output ``DeviceBuffer``."""
        from . import _gradient_lib, rays as rb

        L, par = _gradient_lib.lib(), _gradient_lib.params(**params)
        width, height = _gradient_lib._addon.c_int(width, "width"), _gradient_lib._addon.c_int(height, "height")
        m = width * height
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((max(m, 1),), np.float64, self.device)
            ptr = self._plane_ptr
            _gradient_lib.check(L.pt_rays_gradient_keep_device(self.device, width, height, C.byref(par), ptr(colour, "colour"),
                                                               ptr(shape_index, "shape_index"), ptr(probe_index, "probe_index"),
                                                               ptr(probe_old, "probe_old"), ptr(out, "out"), int(out.nbytes),
                                                               C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None:
            raise ValueError("stream= and out= go with device=True (host frames are staged and synchronous)")
        ns = int(L.pt_rays_gradient_strata(width, height, par.stratum))
        sh = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        index = np.ascontiguousarray(probe_index, dtype=np.int32).reshape(-1)
        col, old = rb.planar(colour, 3), rb.planar(probe_old, 3)
        if sh.shape[0] != m or col.shape[1] != m or (1 <= par.stratum <= _gradient_lib.MAX_STRATUM and (index.shape[0] != ns or old.shape[1] != ns)):
            raise ValueError(f"a {width} x {height} frame has {m} records and {ns} probes, not {sh.shape[0]} shape indices, {col.shape[1]} colours, "
                             f"{index.shape[0]} probe indices and {old.shape[1]} old colours")
        keep = np.empty(m, np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _gradient_lib.check(L.pt_rays_gradient_keep(self.device, width, height, C.byref(par), p(col), p(sh), p(index), p(old), p(keep), keep.nbytes))
        return keep.reshape(height, width)

    def gradient_accumulate(self, colour, samples, shape_index, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point,
                            prev_count, prev_camera, moved, motion, keep, width: int, height: int, device: bool = False, stream=None, out=None,
                            out_moments=None, out_count=None, n_shapes=None, **params):
        """:meth:`motion` with one more plane (include/ptrace_gradient.h): ``keep`` (float64 per record, :meth:`gradient_keep`'s
        output; ``None``: everything is kept and every bit is :meth:`motion`'s), clamped to [0, 1], multiplies the weight of the
        reprojected history and, under a floor, its length, before this frame's samples are blended in.  Everything else as
        :meth:`motion` takes and returns it; :func:`pytracer_amd.rays.gradient_accumulate_host` in every bit.  No scene is read."""
        from . import _gradient_lib, rays as rb

        L, par, cam = _gradient_lib.lib(), _gradient_lib.history(**params), _gradient_lib.camera(prev_camera)
        width, height = _gradient_lib._addon.c_int(width, "width"), _gradient_lib._addon.c_int(height, "height")
        m = width * height
        if device:
            from .devmem import DeviceBuffer

            if (moved is None) != (motion is None):
                raise ValueError("moved and motion come together (or neither: nothing moved)")
            if n_shapes is None:
                if moved is None:
                    n_shapes = 0
                elif hasattr(moved, "nbytes"):
                    n_shapes = int(moved.nbytes) // 4
                elif callable(getattr(moved, "numel", None)):
                    n_shapes = int(moved.numel())
                else:
                    raise ValueError("n_shapes= is needed when the tables are raw device addresses")
            n_shapes = _gradient_lib._addon.c_int(n_shapes, "n_shapes")
            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if out_moments is None:
                out_moments = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if out_count is None:
                out_count = DeviceBuffer((max(m, 1),), np.int32, self.device)
            ptr = self._plane_ptr
            _gradient_lib.check(L.pt_rays_gradient_accumulate_device(
                self.device, width, height, C.byref(par), C.byref(cam), ptr(colour, "colour"), ptr(samples, "samples"),
                ptr(shape_index, "shape_index"), ptr(normal, "normal"), ptr(point, "point"), ptr(prev_colour, "prev_colour"),
                ptr(prev_moments, "prev_moments"), ptr(prev_shape, "prev_shape"), ptr(prev_normal, "prev_normal"), ptr(prev_point, "prev_point"),
                ptr(prev_count, "prev_count"), n_shapes, ptr(moved, "moved"), ptr(motion, "motion"), ptr(keep, "keep"), ptr(out, "out"),
                int(out.nbytes), ptr(out_moments, "out_moments"), int(out_moments.nbytes), ptr(out_count, "out_count"), int(out_count.nbytes),
                C.c_void_p(handle) if handle else None))
            for buf in (out, out_moments, out_count):
                if hasattr(buf, "rendered_on"):
                    buf.rendered_on(stream)
            return out, out_moments, out_count
        if stream is not None or out is not None or out_moments is not None or out_count is not None or n_shapes is not None:
            raise ValueError("stream=, out=, out_moments=, out_count= and n_shapes= go with device=True (host frames are staged and synchronous)")
        n_shapes, moved, motion = _gradient_lib.tables(moved, motion)
        ints = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (shape_index, prev_shape, prev_count)]
        taken = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32).reshape(-1)
        kept = None if keep is None else np.ascontiguousarray(keep, dtype=np.float64).reshape(-1)
        planes = [rb.planar(a, 3) for a in (colour, normal, point, prev_colour, prev_moments, prev_normal, prev_point)]
        if (any(a.shape[0] != m for a in ints) or any(p.shape[1] != m for p in planes) or (taken is not None and taken.shape[0] != m)
                or (kept is not None and kept.shape[0] != m)):
            raise ValueError(f"a {width} x {height} frame has {m} records, not {[a.shape[0] for a in ints]} shape indices and counts, "
                             f"{None if taken is None else taken.shape[0]} sample counts, {None if kept is None else kept.shape[0]} keep values "
                             f"and {[p.shape[1] for p in planes]} colours, normals, points and moments")
        buf, mom, cnt = np.empty((3, m), dtype=np.float64), np.empty((3, m), dtype=np.float64), np.empty((m,), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _gradient_lib.check(L.pt_rays_gradient_accumulate(self.device, width, height, C.byref(par), C.byref(cam), p(planes[0]), p(taken), p(ints[0]),
                                                          p(planes[1]), p(planes[2]), p(planes[3]), p(planes[4]), p(ints[1]), p(planes[5]),
                                                          p(planes[6]), p(ints[2]), n_shapes, p(moved), p(motion), p(kept), p(buf), buf.nbytes,
                                                          p(mom), mom.nbytes, p(cnt), cnt.nbytes))
        return (np.ascontiguousarray(buf.T).reshape(height, width, 3), np.ascontiguousarray(mom.T).reshape(height, width, 3),
                cnt.reshape(height, width))

    def gradient_clear(self, count, m=None, stream=None):
        """An empty history: the ``m`` int32 lengths of the device buffer ``count`` (default: all it holds) become 0 on ``stream``
        (``pt_rays_gradient_clear_device``) -> ``count``.  With lengths of 0 no colour, moment or weight of the history is read."""
        from . import _gradient_lib

        handle = getattr(stream, "handle", stream)
        m = self._device_count(count, m)
        nbytes = int(count.nbytes) if hasattr(count, "nbytes") else 4 * m
        _gradient_lib.check(_gradient_lib.lib().pt_rays_gradient_clear_device(self.device, m, self._plane_ptr(count, "count"), nbytes,
                                                                              C.c_void_p(handle) if handle else None))
        if hasattr(count, "rendered_on"):
            count.rendered_on(stream)
        return count

    # -- variance queries (include/ptrace_variance.h, libptrace_variance.so): moments, a per-pixel variance and a filter guided by it --
    @staticmethod
    def _variance_frame(width, height):
        from . import _addon

        width, height = _addon.c_int(width, "width"), _addon.c_int(height, "height")
        return width, height, width * height

    def variance_moments(self, colour, shape_index, width: int, height: int, device: bool = False, stream=None, out=None):
        """The luminance moments of include/ptrace_variance.h of a ``width x height`` frame: per record ``(l, l * l, 0)`` with ``l``
        the luminosity of ``colour`` (``[..., 3]``), zeros where ``shape_index`` is negative -> ``[height, width, 3]`` float64,
        :func:`pytracer_amd.rays.luminance_moments_host` in every bit: a frame for :meth:`temporal`, as its ``colour``.
        ``device=True``: the planes (``[3, m]`` fp64, int32) are in HBM, the launch is enqueued on ``stream`` -> the output
        ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _variance_lib, rays as rb

        L = _variance_lib.lib()
        width, height, m = self._variance_frame(width, height)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            ptr = self._plane_ptr
            _variance_lib.check(L.pt_rays_variance_moments_device(self.device, width, height, ptr(colour, "colour"), ptr(shape_index, "shape_index"),
                                                                  ptr(out, "out"), int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None:
            raise ValueError("stream= and out= go with device=True (host frames are staged and synchronous)")
        shape = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        col = rb.planar(colour, 3)
        if shape.shape[0] != m or col.shape[1] != m:
            raise ValueError(f"a {width} x {height} frame has {m} records, not {shape.shape[0]} shape indices and {col.shape[1]} colours")
        buf = np.empty((3, m), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _variance_lib.check(L.pt_rays_variance_moments(self.device, width, height, p(col), p(shape), p(buf), buf.nbytes))
        return np.ascontiguousarray(buf.T).reshape(height, width, 3)

    def variance_estimate(self, moments, count, shape_index, normal, point, width: int, height: int, device: bool = False, stream=None, out=None,
                          **params):
        """The variance estimate of include/ptrace_variance.h over a ``width x height`` frame, from the accumulated ``moments``
        (``[..., 3]``: first and second luminance moment, and a third channel that is not read) and the history lengths ``count``:
        ``max(mu2 - mu1^2, 0) / n`` where ``n >= min_history``, else the same from the means of the moments over the accepted taps
        of a 7x7 window (``same_shape``, ``wrap_x``, ``normal_min``, ``point_tolerance``) -> ``[height, width]`` float64,
        :func:`pytracer_amd.rays.variance_estimate_host` in every bit.  ``device=True``: the planes are in HBM, the launch is
        enqueued on ``stream`` -> the output ``DeviceBuffer`` of ``m`` fp64 (``out``, or a new one)."""
        from . import _variance_lib, rays as rb

        L, par = _variance_lib.lib(), _variance_lib.params(**params)
        width, height, m = self._variance_frame(width, height)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((max(m, 1),), np.float64, self.device)
            ptr = self._plane_ptr
            _variance_lib.check(L.pt_rays_variance_estimate_device(self.device, width, height, C.byref(par), ptr(moments, "moments"),
                                                                   ptr(count, "count"), ptr(shape_index, "shape_index"), ptr(normal, "normal"),
                                                                   ptr(point, "point"), ptr(out, "out"), int(out.nbytes),
                                                                   C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None:
            raise ValueError("stream= and out= go with device=True (host frames are staged and synchronous)")
        ints = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (count, shape_index)]
        planes = [rb.planar(a, 3) for a in (moments, normal, point)]
        if any(a.shape[0] != m for a in ints) or any(p.shape[1] != m for p in planes):
            raise ValueError(f"a {width} x {height} frame has {m} records, not {[a.shape[0] for a in ints]} counts and shape indices and "
                             f"{[p.shape[1] for p in planes]} moments, normals and points")
        buf = np.empty((m,), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _variance_lib.check(L.pt_rays_variance_estimate(self.device, width, height, C.byref(par), p(planes[0]), p(ints[0]), p(ints[1]), p(planes[1]),
                                                        p(planes[2]), p(buf), buf.nbytes))
        return buf.reshape(height, width)

    def variance_workspace_bytes(self, width: int, height: int, **params) -> int:
        """Bytes of the workspace :meth:`variance_filter` needs on the device for a ``width x height`` frame (``params``: its own)."""
        from . import _variance_lib

        L, par = _variance_lib.lib(), _variance_lib.params(**params)
        width, height, m = self._variance_frame(width, height)
        need = int(L.pt_rays_variance_workspace_bytes(width, height, C.byref(par)))
        if need == 0 and m != 0:
            raise _lib.PtraceError(-1, _variance_lib.last_error())
        return need

    def variance_filter(self, colour, variance, shape_index, normal, point, width: int, height: int, device: bool = False, stream=None, out=None,
                        out_variance=None, workspace=None, **params):
        """The variance-guided a-trous filter of include/ptrace_variance.h over a ``width x height`` frame: the stencil, the passes
        and the geometric weights of :meth:`denoise`, with its colour weight replaced by ``1 / (1 + dl^2 / (sigma_luminance^2 * g +
        epsilon))`` -- ``dl`` the luminance difference, ``g`` the 3x3-prefiltered ``variance`` at the pixel -- and the variance
        filtered along with the colour (weights squared) -> ``(colour [height, width, 3], variance [height, width])`` float64,
        :func:`pytracer_amd.rays.variance_filter_host` in every bit.  No scene is read.  ``device=True``: the planes (``[3, m]`` and
        ``[m]`` fp64, int32) are in HBM, the passes are enqueued on ``stream`` -> the two output ``DeviceBuffer`` s (``out`` and
        ``out_variance``, or new ones); ``workspace``: a ``DeviceBuffer`` of :meth:`variance_workspace_bytes` (or a new one)."""
        from . import _variance_lib, rays as rb

        L, par = _variance_lib.lib(), _variance_lib.params(**params)
        width, height, m = self._variance_frame(width, height)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if out is None:
                out = DeviceBuffer((3, max(m, 1)), np.float64, self.device)
            if out_variance is None:
                out_variance = DeviceBuffer((max(m, 1),), np.float64, self.device)
            if workspace is None:
                workspace = DeviceBuffer((max(self.variance_workspace_bytes(width, height, **params), 8),), np.uint8, self.device)
            ptr = self._plane_ptr
            _variance_lib.check(L.pt_rays_variance_filter_device(
                self.device, width, height, C.byref(par), ptr(colour, "colour"), ptr(variance, "variance"), ptr(normal, "normal"),
                ptr(point, "point"), ptr(shape_index, "shape_index"), ptr(out, "out"), int(out.nbytes), ptr(out_variance, "out_variance"),
                int(out_variance.nbytes), ptr(workspace, "workspace"), int(workspace.nbytes), C.c_void_p(handle) if handle else None))
            for buf in (out, out_variance, workspace):
                if hasattr(buf, "rendered_on"):
                    buf.rendered_on(stream)
            if hasattr(out, "rendered_on"):
                out._variance_workspace = workspace  # in flight on `stream` as long as the output is: freed with it
            return out, out_variance
        if stream is not None or out is not None or out_variance is not None or workspace is not None:
            raise ValueError("stream=, out=, out_variance= and workspace= go with device=True (host frames are staged and synchronous)")
        shape = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        var = np.ascontiguousarray(variance, dtype=np.float64).reshape(-1)
        planes = [rb.planar(colour, 3), rb.planar(normal, 3), rb.planar(point, 3)]
        if shape.shape[0] != m or var.shape[0] != m or any(p.shape[1] != m for p in planes):
            raise ValueError(f"a {width} x {height} frame has {m} records, not {shape.shape[0]} shape indices, {var.shape[0]} variances and "
                             f"{[p.shape[1] for p in planes]} colours, normals and points")
        buf, vbuf = np.empty((3, m), dtype=np.float64), np.empty((m,), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _variance_lib.check(L.pt_rays_variance_filter(self.device, width, height, C.byref(par), p(planes[0]), p(var), p(planes[1]), p(planes[2]),
                                                      p(shape), p(buf), buf.nbytes, p(vbuf), vbuf.nbytes))
        return np.ascontiguousarray(buf.T).reshape(height, width, 3), vbuf.reshape(height, width)

    # -- adaptive queries (include/ptrace_adaptive.h, libptrace_adaptive.so): sample counts from a variance, their prefix sum, a ragged gather --
    def sample_counts(self, variance, colour, shape_index, device: bool = False, stream=None, out=None, m=None, **params):
        """The counts query of include/ptrace_adaptive.h: per record ``ceil(gain * variance / (tolerance * max(lum(colour),
        luminance_floor))^2)`` clamped into ``[min_samples, max_samples]``, ``max_samples`` where the variance is negative or NaN, 0
        where ``shape_index`` is negative -> ``int32[m]``, :func:`pytracer_amd.rays.sample_counts_host` in every bit.  ``variance``
        ``[m]``, ``colour`` ``[m, 3]``.  ``device=True``: the planes (``[m]`` and ``[3, m]`` fp64, int32) are in HBM (``m=`` where they
        are raw addresses), the launch is enqueued on ``stream`` -> the output ``DeviceBuffer`` of ``m`` int32 (``out``, or a new one)."""
        from . import _adaptive_lib, rays as rb

        L, par = _adaptive_lib.lib(), _adaptive_lib.count_params(**params)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if m is None:
                if not hasattr(variance, "nbytes"):
                    raise ValueError("m= is needed when the variance is a raw device address")
                m = int(variance.nbytes) // 8
            m = int(m)
            if out is None:
                out = DeviceBuffer((max(m, 1),), np.int32, self.device)
            ptr = self._plane_ptr
            _adaptive_lib.check(L.pt_rays_adaptive_counts_device(self.device, m, C.byref(par), ptr(variance, "variance"), ptr(colour, "colour"),
                                                                 ptr(shape_index, "shape_index"), ptr(out, "out"), int(out.nbytes),
                                                                 C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            return out
        if stream is not None or out is not None or m is not None:
            raise ValueError("stream=, out= and m= go with device=True (host planes are staged and synchronous)")
        var = np.ascontiguousarray(variance, dtype=np.float64).reshape(-1)
        shape = np.ascontiguousarray(shape_index, dtype=np.int32).reshape(-1)
        col = rb.planar(colour, 3)
        m = var.shape[0]
        if shape.shape[0] != m or col.shape[1] != m:
            raise ValueError(f"{m} variances, {col.shape[1]} colours and {shape.shape[0]} shape indices")
        buf = np.zeros((m,), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _adaptive_lib.check(L.pt_rays_adaptive_counts(self.device, m, C.byref(par), p(var), p(col), p(shape), p(buf), buf.nbytes))
        return buf

    def sample_offsets(self, counts, device: bool = False, stream=None, out=None, workspace=None, n=None):
        """The offsets query of include/ptrace_adaptive.h: ``int64[n + 1]``, the exclusive prefix sum of ``max(counts, 0)`` taken on
        the device (three launches: sums of 256, their scan, the final pass); the last value is the total.
        :func:`pytracer_amd.rays.sample_offsets_host` in every bit.  ``device=True``: ``counts`` is int32 in HBM (``n=`` where it is
        a raw address), the launches are enqueued on ``stream`` -> the output ``DeviceBuffer`` of ``n + 1`` int64 (``out``, or a new
        one); ``workspace``: ``pt_rays_adaptive_offsets_workspace_bytes(n)`` bytes (or a new buffer)."""
        from . import _adaptive_lib

        L = _adaptive_lib.lib()
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            n = self._device_count(counts, n)
            if out is None:
                out = DeviceBuffer((n + 1,), np.int64, self.device)
            if workspace is None:
                workspace = DeviceBuffer((max(int(L.pt_rays_adaptive_offsets_workspace_bytes(n)), 8),), np.uint8, self.device)
                out._offsets_workspace = workspace  # in flight on `stream` as long as the output is: freed with it
            ptr = self._plane_ptr
            _adaptive_lib.check(L.pt_rays_adaptive_offsets_device(self.device, n, ptr(counts, "counts"), ptr(out, "out"), int(out.nbytes),
                                                                  ptr(workspace, "workspace"), int(workspace.nbytes),
                                                                  C.c_void_p(handle) if handle else None))
            for buf in (out, workspace):
                if hasattr(buf, "rendered_on"):
                    buf.rendered_on(stream)
            return out
        if stream is not None or out is not None or workspace is not None or n is not None:
            raise ValueError("stream=, out=, workspace= and n= go with device=True (host planes are staged and synchronous)")
        counts = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int32)
        buf = np.zeros((counts.shape[0] + 1,), dtype=np.int64)
        _adaptive_lib.check(L.pt_rays_adaptive_offsets(self.device, counts.shape[0], counts.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p),
                                                       buf.nbytes))
        return buf

    def adaptive_workspace_bytes(self, n: int, capacity: int, num_of_rays: int = 1, max_depth: int = 10, depth: int = 0) -> int:
        """Bytes of the workspace ``gather_ragged(device=True)`` needs for ``n`` records and sample planes of ``capacity`` samples
        (``pt_rays_adaptive_workspace_bytes``: the node stacks, sized by the lanes a launch keeps resident, and four 8-byte planes of
        ``capacity`` values)."""
        from . import _adaptive_lib

        need = int(_adaptive_lib.lib().pt_rays_adaptive_workspace_bytes(self.device, int(n), int(capacity), int(num_of_rays), int(max_depth),
                                                                        int(depth)))
        if need == 0:
            raise ValueError(f"no workspace size for these arguments: {_adaptive_lib.last_error()}")
        return need

    def gather_ragged(self, points, normals, counts, offsets, capacity: int, init_state: int = 42, seqs=None, active=None, num_of_rays: int = 1,
                      max_depth: int = 10, russian_roulette_limit: int = 3, background=(0.0, 0.0, 0.0), depth: int = 0, channels="all",
                      init_seq: int = 54, device: bool = False, stream=None, out=None, workspace=None, n=None):
        """:meth:`gather` with ``samples`` replaced by the per-record planes ``counts`` (``int32[n]``) and ``offsets`` (``int64[n +
        1]``, :meth:`sample_offsets` of those counts): record ``i`` takes ``K_i = min(max(counts[i], 0), max(capacity - offsets[i],
        0))`` samples, sample ``k`` from ``PCG(init_state, seqs[i] + k)`` (``seqs=None``: ``init_seq + offsets[i]``), and its radiance
        and count are bit for bit :meth:`gather` 's for that record alone with ``samples = K_i`` (include/ptrace_adaptive.h).
        ``capacity``: the samples the workspace's planes hold -- the hard budget.  ``channels``: ``"count"``, ``"taken"``, ``"all"``,
        ``"none"`` or ``PT_ADAPTIVE_*`` bits -> :class:`pytracer_amd.rays.RaggedRadiance`.  ``device=True``: every plane is a
        ``DeviceBuffer``, a device tensor or a raw address (then with ``n=``); the batch is enqueued on ``stream`` with ``workspace``
        (:meth:`adaptive_workspace_bytes` bytes; ``None``: a new buffer) -> the output ``DeviceBuffer`` (``out``, or a new one)."""
        from . import _adaptive_lib, rays as rb

        L, block, bits = _adaptive_lib.lib(), self.kernel_args(), rb.adaptive_channels(channels)
        par = _adaptive_lib.params(num_of_rays, max_depth, russian_roulette_limit, depth, init_state, init_seq, background, capacity)
        if device:
            from .devmem import DeviceBuffer

            handle = getattr(stream, "handle", stream)
            if n is None:
                if not hasattr(points, "nbytes"):
                    raise ValueError("n= is needed when the points are a raw device address")
                n = int(points.nbytes) // 24
            n = int(n)
            if out is None:
                out = DeviceBuffer((max(rb.adaptive_bytes(n, bits), 8),), np.uint8, self.device)
            if workspace is None and n > 0:
                # (0: arguments the library refuses -- the call below then says which, with its own error code)
                need = int(L.pt_rays_adaptive_workspace_bytes(self.device, n, par.capacity, par.num_of_rays, par.max_depth, par.depth0))
                if need:
                    workspace = DeviceBuffer((need,), np.uint8, self.device)
                    out._gather_workspace = workspace  # in flight on `stream` as long as the output is: freed with it
            ptr = self._plane_ptr
            _adaptive_lib.check(L.pt_rays_adaptive_gather_device(
                self.device, block, len(block), ptr(points, "points"), ptr(normals, "normals"), ptr(active, "active"), ptr(seqs, "seqs"),
                ptr(counts, "counts"), ptr(offsets, "offsets"), n, C.byref(par), bits, ptr(workspace, "workspace"),
                int(workspace.nbytes) if workspace is not None else 0, ptr(out, "out"), int(out.nbytes), C.c_void_p(handle) if handle else None))
            if hasattr(out, "rendered_on"):
                out.rendered_on(stream)
            if hasattr(workspace, "rendered_on"):
                workspace.rendered_on(stream)
            return out
        if stream is not None or out is not None or n is not None or workspace is not None:
            raise ValueError("stream=, out=, workspace= and n= go with device=True (host batches are staged and synchronous)")
        points = np.ascontiguousarray(points, dtype=np.float64)
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        if points.ndim != 2 or points.shape[0] != 3 or normals.shape != points.shape:
            raise ValueError(f"points and normals must both be planar [3, n] (pytracer_amd.rays.planar), not {points.shape} and {normals.shape}")
        n = points.shape[1]
        counts = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int32)
        offsets = np.ascontiguousarray(np.asarray(offsets).reshape(-1), dtype=np.int64)
        if counts.shape != (n,) or offsets.shape != (n + 1,):
            raise ValueError(f"{n} records take {n} counts and {n + 1} offsets, not {counts.shape[0]} and {offsets.shape[0]}")
        if seqs is not None:
            seqs = rb.stream_numbers(seqs)
            if seqs.shape != (n,):
                raise ValueError(f"seqs must hold one stream number per record ({n}), not {seqs.shape}")
        if active is not None:
            active = np.ascontiguousarray(np.asarray(active).reshape(-1), dtype=np.int32)
            if active.shape != (n,):
                raise ValueError(f"active must hold one int32 per record ({n}), not {active.shape}")
        buf = np.zeros(rb.adaptive_bytes(n, bits), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _adaptive_lib.check(L.pt_rays_adaptive_gather(self.device, block, len(block), p(points), p(normals), p(active), p(seqs), p(counts),
                                                      p(offsets), n, C.byref(par), bits, p(buf), buf.nbytes))
        return rb.RaggedRadiance(buf, n, bits)

    def cull_probe(self, cam: abi.Camera, width: int, height: int, x0: int, x1: int, row0: int, row1: int,
                   pixel=None) -> np.ndarray:
        """Diagnostics: which shapes (by ``World.shapes`` index) the conservative cull of the primary rays through
        the image rectangle ``[x0, x1] x [row0, row1 + 1]`` keeps -- or, with ``pixel=(x, row)``, the cone of that one
        pixel inside the rectangle -- evaluated on the device exactly as the render kernels evaluate it."""
        keep = np.zeros(max(1, self.flat.n_shapes), dtype=np.int32)
        px, py = pixel if pixel is not None else (-1, -1)
        _lib.check(_lib.lib().pt_debug_cull_probe(self._h, C.byref(cam), int(width), int(height), int(x0), int(x1), int(row0),
                                                  int(row1), int(px), int(py), keep.ctypes.data_as(C.c_void_p)))
        return keep[: self.flat.n_shapes].astype(bool)

    def hit_probe(self, rays, shape_index: int = -1) -> np.ndarray:
        """Diagnostics (include/ptrace_debug.h): ``Shape.ray_intersection`` of shape ``shape_index`` of ``World.shapes``
        (or, with -1, ``World.ray_intersection``) for ``[n, 8]`` rays (origin, dir, tmin, tmax), evaluated by the
        kernels' own query and hit-record code.  -> ``[n, 12]``: hit, t, world point, normalised normal, u, v, index."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 12), dtype=np.float64)
        _lib.check(_lib.lib().pt_debug_hit_probe(self._h, int(shape_index), rays.ctypes.data_as(C.c_void_p), rays.shape[0],
                                                 out.ctypes.data_as(C.c_void_p)))
        return out

    def lanes_probe(self, rays, anyhit: bool = False) -> np.ndarray:
        """Diagnostics (include/ptrace_debug.h): the same rays through the query the scattered and shadow rays use
        (conservative fp32 filter or grid walk, then exact visits).  -> ``[n, 4]``: hit (or blocked), t, index, 0."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 4), dtype=np.float64)
        _lib.check(_lib.lib().pt_debug_lanes_probe(self._h, int(bool(anyhit)), rays.ctypes.data_as(C.c_void_p), rays.shape[0],
                                                   out.ctypes.data_as(C.c_void_p)))
        return out

    def sync(self) -> None:
        _lib.check(_lib.lib().pt_sync(self._h))

    def set_count_rays(self, enable: bool) -> None:
        _lib.check(_lib.lib().pt_set_count_rays(self._h, int(bool(enable))))

    def set_dome_shortcut(self, enable: bool) -> None:
        """Measurement switch: off = every primary ray is generated and traced (same image)."""
        _lib.check(_lib.lib().pt_set_dome_shortcut(self._h, int(bool(enable))))

    def set_timing(self, enable: bool) -> None:
        """hipEvent pair around each render kernel on/off (off: frames run back to back)."""
        _lib.check(_lib.lib().pt_set_timing(self._h, int(bool(enable))))

    def profile_begin(self, capacity: int) -> None:
        """Bracket every following render kernel with its own hipEvent pair (up to ``capacity``)."""
        _lib.check(_lib.lib().pt_profile_begin(self._h, int(capacity)))

    def profile_end(self) -> Tuple[float, int]:
        """-> (summed kernel time in ms, launches) since ``profile_begin``; synchronises."""
        total, n = C.c_double(0.0), C.c_int(0)
        _lib.check(_lib.lib().pt_profile_end(self._h, C.byref(total), C.byref(n)))
        return float(total.value), int(n.value)

    def stats(self) -> abi.Stats:
        st = abi.Stats()
        _lib.check(_lib.lib().pt_get_stats(self._h, C.byref(st)))
        return st

    def handed_over(self) -> Tuple[int, int]:
        """Diagnostics, ``num_of_rays > 1``: (pixels the one-queue kernel handed to the tree kernel in the last frame, the ray
        budget the device derived from the frame's flagged pixels)."""
        n, b = C.c_ulonglong(0), C.c_ulonglong(0)
        _lib.check(_lib.lib().pt_debug_handed_over(self._h, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)


def device_info(device: int = 0) -> Tuple[int, int]:
    """-> (compute units, peak shader clock in kHz)."""
    cu, khz = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().pt_device_info(int(device), C.byref(cu), C.byref(khz)))
    return int(cu.value), int(khz.value)


def device_count() -> int:
    return int(_lib.lib().pt_device_count())


def plan(flat, cam: abi.Camera, params: abi.Params, n_cu: int = 256, dome_shortcut: bool = True) -> abi.PlanInfo:
    """What ``pt_render`` would launch for this scene, camera and parameters -- kernels, grids, LDS, frame-stack home,
    thresholds -- from the library's host-side planner (``pt_debug_plan``, csrc/pt_plan.h).  Touches no device."""
    info = abi.PlanInfo()
    desc = flat.desc()
    _lib.check(_lib.lib().pt_debug_plan(C.byref(desc), C.byref(cam), C.byref(params), int(n_cu), 1 if dome_shortcut else 0, C.byref(info)))
    return info


def plan_hits(flat, cam: abi.Camera, params: abi.Params, channels=abi.HIT_ALL, n_cu: int = 256) -> abi.PlanInfo:
    """What ``pt_render_hits`` would launch (``pt_debug_plan_hits``, csrc/pt_hits_plan.h).  Touches no device."""
    info = abi.PlanInfo()
    desc = flat.desc()
    _lib.check(_lib.lib().pt_debug_plan_hits(C.byref(desc), C.byref(cam), C.byref(params), abi.hit_channels(channels), int(n_cu),
                                             C.byref(info)))
    return info


def set_tuning(name: str, value: int) -> None:
    """One of the library's debug / measurement switches (csrc/pt_plan.h: PT_TUNING_TABLE), by field or ``PTRACE_*`` name.
    Takes effect for the next frame of every scene of the process; none changes a pixel."""
    _lib.check(_lib.lib().pt_debug_set_tuning(name.encode(), int(value)))


def get_tuning(name: str) -> int:
    v = C.c_longlong(0)
    _lib.check(_lib.lib().pt_debug_get_tuning(name.encode(), C.byref(v)))
    return int(v.value)


def device_kernargs() -> bool:
    """True iff ``HIP_FORCE_DEV_KERNARG`` asks the HIP runtime for kernel arguments in device memory
    (``pytracer_amd.prefer_device_kernargs()`` before the first HIP call; ``pt_device_kernargs``)."""
    return bool(_lib.lib().pt_device_kernargs())


def camera_probe(cam: abi.Camera, width: int, height: int, pix) -> np.ndarray:
    """Diagnostics: ``ImageTracer.fire_ray`` for ``[n, 4]`` (col, row, u_pixel, v_pixel) -> ``[n, 7]`` (origin, dir, tmin)."""
    pix = np.ascontiguousarray(pix, dtype=np.float64).reshape(-1, 4)
    out = np.zeros((pix.shape[0], 7), dtype=np.float64)
    _lib.check(_lib.lib().pt_debug_camera_probe(C.byref(cam), int(width), int(height), pix.ctypes.data_as(C.c_void_p),
                                                pix.shape[0], out.ctypes.data_as(C.c_void_p)))
    return out


def scatter_probe(rows) -> Tuple[np.ndarray, np.ndarray]:
    """Diagnostics: ``BRDF.scatter_ray`` for ``[n, 12]`` (brdf kind, PCG init_state, init_seq, normal, incoming, point)
    -> (``[n, 7]`` origin, dir, tmin; ``[n]`` generator states after the call)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 12)
    out = np.zeros((rows.shape[0], 7), dtype=np.float64)
    st = np.zeros(rows.shape[0], dtype=np.uint64)
    _lib.check(_lib.lib().pt_debug_scatter_probe(rows.ctypes.data_as(C.c_void_p), rows.shape[0], out.ctypes.data_as(C.c_void_p),
                                                 st.ctypes.data_as(C.c_void_p)))
    return out, st


def probe(op: int, x, y=None) -> np.ndarray:
    """Evaluate a device primitive elementwise (tests: IEEE exactness / ulp distance to libm)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = x if y is None else np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty_like(x)
    _lib.check(_lib.lib().pt_debug_probe(op, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p),
                                         out.ctypes.data_as(C.c_void_p), x.size))
    return out
