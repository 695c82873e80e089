#!/usr/bin/env python3
"""Throughput of ray batches (libptrace_rays.so: pt_rays_trace_device) on the C2 frame's rays, fed back as batches.

    python tools/raybench.py [--width 1280 --height 720 --warmup 3 --steps 10]

Three device-resident batches from BASELINE's C2 (32 spheres + ground plane): the frame's pixel-centre primary rays (as the
hit-record frame itself leaves them), the mirror bounces off their hits (d - 2 (d.n) n, tmin 1e-3) and the shadow segments
from the hit points to a light at (0, 0, 10) (any-hit).  Per batch: warm-up launches, then a timed loop of
``pt_rays_trace_device`` on a stream of its own between two events.  One process; prints Mray/s per batch and the
``pt_render_hits`` kernel time of the same frame beside the primary batch (that frame culls per tile; a batch cannot).
Needs torch only to put the batches into device memory and to read the events.

    python tools/raybench.py --shade [...]

The surface queries (libptrace_surface.so) on the same frame of C2 with two point lights, (-2, 3, 6) and (1, -4, 5) radius 2:
``surface`` (both colours) and ``shade_lights`` on the frame's hit records, read in place out of the hit-record buffer in HBM,
timed the same way; then the two-step point-light frame -- the ``pt_render_hits`` kernel plus ``shade_lights`` -- beside the
fused RENDERER_POINTLIGHT frame kernel (``stats().kernel_ms``), which culls per tile and keeps the record in registers.

    python tools/raybench.py --scatter [...]

The bounce (libptrace_scatter.so: pt_rays_scatter_device) on the hit records of the C2 frame, read in place out of the
hit-record buffer in HBM, a generator per record, both channels, with ``roulette`` 0 and 1, timed the same way: records/s and the
effective bandwidth from the bytes a record moves (112 B in, 132 B out; a record without a hit reads 20 B of them), beside the
6.29 TB/s a float4 copy reaches on this chip.  Then the whole ``PathTracerShader`` route (hit-record frame, then per depth a
scatter and a trace, the sums on the host) beside the fused ``PathTracer`` at ``num_of_rays=1, max_depth=3``: wall time of
``fire_all_rays``, and whether the two frames are byte-identical.

    python tools/raybench.py --radiance [...]

The radiance query (libptrace_radiance.so: pt_rays_radiance_device) on the C2 frame's primary rays, a generator per ray
(``PCG(45, 54 + i)``: the fused path tracer's ``pcg_mode="sample"`` at ``samples_per_side=0``), ``max_depth=3``, limit 3, timed the
same way with ``num_of_rays`` 1 and 10: rays traced per second, beside the fused path-tracer frame of the same parameters
(``stats().kernel_ms``; the frames are compared byte for byte) and, at ``num_of_rays=1``, beside the chain in HBM that the four
steps before it make: trace + 3 x (scatter + trace), every batch read in place out of the one before.

    python tools/raybench.py --gather [...]

The gather query (libptrace_gather.so: pt_rays_gather_device) on the first hits of the C2 frame, ``max_depth=3``, limit 3, sample
``k`` of record ``i`` drawing from ``PCG(45, 54 + i K + k)``: K = 16 and ``num_of_rays`` 1 on every record, K = 64 on every 8th, K = 16
with ``num_of_rays`` 2.  Beside each, in the same process, the route a caller has without it, minus its host work: the ``n K`` sample
rays and their generators made beforehand in HBM (the scatter query on records that name a diffuse shape; not timed), then
``pt_rays_radiance_device`` on them, timed the same way; the host's sum of that output in sample order is compared with the gather's
output bit for bit.  Last, the time of the radiance query with ``num_of_rays = K`` on ONE ray per record (the frame's primary ray):
another estimator -- one generator per record, K children at every depth -- reported for comparison.

    python tools/raybench.py --bake [--map 512 --samples 16 --repeats 5 ...]

The bake query (libptrace_bake.so: pt_rays_bake_device): a ``--map x --map`` light map at ``--samples`` samples of the first diffuse
sphere of C2 behind its sky sphere, ``num_of_rays=1``, ``max_depth=3``, limit 3, depth 1, with and without jitter.  Beside it, in
the same process, the gather query on the same texel-centre records, prepared in HBM by ``pt_rays_surface_points_device`` (timed
on its own, not part of the gather's time), at the same K and the same streams: the centre-mode bake must equal it bit for bit.
The three are timed ALTERNATING, ``--repeats`` rounds of ``--warmup`` + ``--steps`` launches each between two events; printed are
every round's time, the median per query and the spread of the rounds (max - min over the median).  Then the purpose as two
times: the flat frame of the baked ``demo`` world (its ground plane and sky carrying their outgoing maps) beside the path-traced
frame of ``demo`` at the CLI's defaults (640x480, ``num_of_rays=10``, ``max_depth=3``), kernel times from ``stats()``."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shade", action="store_true", help="time the surface queries instead of the ray batches")
    ap.add_argument("--scatter", action="store_true", help="time the bounce (roulette + scatter_ray) and the PathTracerShader route")
    ap.add_argument("--radiance", action="store_true", help="time the radiance query beside the chain in HBM and the fused path tracer")
    ap.add_argument("--gather", action="store_true", help="time the gather query beside path_radiance on the same sample rays prepared in HBM")
    ap.add_argument("--bake", action="store_true", help="time the bake query beside the gather on the same texel-centre records prepared in HBM")
    ap.add_argument("--map", type=int, default=512, help="--bake: texels per side of the map")
    ap.add_argument("--samples", type=int, default=16, help="--bake: samples per texel")
    ap.add_argument("--repeats", type=int, default=5, help="--bake: alternating rounds per query")
    args = ap.parse_args()
    if args.bake:
        return bake(args)
    if args.gather:
        return gather(args)
    if args.radiance:
        return radiance(args)
    if args.shade:
        return shade(args)
    if args.scatter:
        return scatter(args)
    import torch

    from pytracer_amd import _rays_lib, abi, flatten, rays as rb, scenes
    from pytracer_amd.device import DeviceScene

    W, H = args.width, args.height
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    cam = flatten.flatten_camera(scenes.synthetic_camera(W, H))
    p = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    R = _rays_lib.lib()
    with DeviceScene(flat) as ds:
        frame = ds.render_hits(cam, p, abi.HIT_ALL)
        frame_ms = []
        for _ in range(args.warmup + args.steps):
            ds.render_hits(cam, p, abi.HIT_T | abi.HIT_POINT | abi.HIT_NORMAL | abi.HIT_UV)
            frame_ms.append(ds.stats().kernel_ms)
        frame_ms = float(np.median(frame_ms[args.warmup:]))
        n = W * H
        o, d = frame.ray_origin.reshape(n, 3), frame.ray_dir.reshape(n, 3)
        hit = frame.hit.reshape(n)
        pt, nrm = frame.point.reshape(n, 3)[hit], frame.normal.reshape(n, 3)[hit]
        dn = np.sum(d[hit] * nrm, axis=1)
        batches = [("primary rays, closest hit", rb.ray_planes(o, d), 0, rb.RAY_CHANNELS),
                   ("mirror bounces, closest hit", rb.ray_planes(pt, d[hit] - 2.0 * dn[:, None] * nrm, tmin=1e-3), 0, rb.RAY_CHANNELS),
                   ("shadow segments, any-hit", rb.visibility_rays(pt, (0.0, 0.0, 10.0)), 1, 0)]
        block = ds.kernel_args()
        stream = torch.cuda.Stream()
        print(f"C2 {W}x{H}: pt_render_hits (t, point, normal, uv) kernel {frame_ms:.3f} ms = {n / frame_ms / 1e3:.1f} Mray/s, culled per tile")
        for label, rays, anyhit, channels in batches:
            m = rays.shape[1]
            rays_dev = torch.from_numpy(rays).cuda()
            out = torch.empty(int(R.pt_rays_bytes(m, channels, anyhit)), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def go():
                _rays_lib.check(R.pt_rays_trace_device(0, block, len(block), C.c_void_p(rays_dev.data_ptr()), m, channels, anyhit,
                                                       C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(stream.cuda_stream)))

            for _ in range(args.warmup):
                go()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                go()
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.steps
            plane = out[: m * 4].view(torch.int32)
            some = int((plane > 0).sum()) if anyhit else int((plane >= 0).sum())
            print(f"{label:30s} {m:8d} rays  {ms:8.3f} ms  {m / ms / 1e3:8.1f} Mray/s  ({some} {'blocked' if anyhit else 'hit'})"
                  + (f"  = {ms / frame_ms:.2f} x the frame's kernel time" if label.startswith("primary") else ""))


def shade(args):
    import torch

    from pytracer_amd import abi, flatten, hostmodel as hm, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer

    W, H = args.width, args.height
    n = W * H
    world = scenes.synthetic_world(32, with_plane=True)
    world.add_light(hm.PointLight(hm.Vec(-2.0, 3.0, 6.0), hm.Color(1.0, 0.9, 0.8), 0.0))
    world.add_light(hm.PointLight(hm.Vec(1.0, -4.0, 5.0), hm.Color(0.2, 0.3, 0.9), 2.0))
    flat = flatten.flatten_world(world)
    cam = flatten.flatten_camera(scenes.synthetic_camera(W, H))
    p_hits = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    p_fused = abi.make_params(W, H, abi.RENDERER_POINTLIGHT, samples_per_side=0)
    with DeviceScene(flat) as ds:
        def kernel_ms(call):
            ms = []
            for _ in range(args.warmup + args.steps):
                call()
                ms.append(ds.stats().kernel_ms)
            return float(np.median(ms[args.warmup:]))

        fused_ms = kernel_ms(lambda: ds.render(cam, p_fused))
        fused = ds.render(cam, p_fused)
        hits_ms = kernel_ms(lambda: ds.render_hits(cam, p_hits, abi.HIT_ALL))
        frame = ds.render_hits(cam, p_hits, abi.HIT_ALL)
        buf = torch.from_numpy(frame.buffer).cuda()
        base = buf.data_ptr()
        at = lambda ch, comp=0: base + abi.hits_plane_offset(p_hits, abi.HIT_ALL, ch, comp)  # noqa: E731
        colours = DeviceBuffer((3, n), np.float64)
        mats = DeviceBuffer((rb.surface_bytes(n, rb.SURF_ALL),), np.uint8)
        ds.slot_table()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        calls = [("surface (brdf colour, emitted)", lambda: ds.surface(base, at(abi.HIT_UV), "all", device=True, stream=stream.cuda_stream, out=mats, n=n)),
                 ("shade_lights (2 lights)", lambda: ds.shade_lights(base, at(abi.HIT_POINT), at(abi.HIT_NORMAL), at(abi.HIT_UV), at(abi.HIT_RAY, 3),
                                                                     device=True, stream=stream.cuda_stream, out=colours, n=n))]
        print(f"C2 + 2 lights {W}x{H}: fused RENDERER_POINTLIGHT kernel {fused_ms:.3f} ms; pt_render_hits (all channels) kernel {hits_ms:.3f} ms")
        took = {}
        for label, go in calls:
            for _ in range(args.warmup):
                go()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                go()
            e1.record(stream)
            e1.synchronize()
            took[label] = ms = e0.elapsed_time(e1) / args.steps
            print(f"{label:32s} {n:8d} records  {ms:8.3f} ms  {n / ms / 1e3:8.1f} Mrecord/s")
        two_step = hits_ms + took["shade_lights (2 lights)"]
        same = colours.numpy().reshape(3, H, W).transpose(1, 2, 0).tobytes() == fused.tobytes()
        print(f"pt_render_hits + shade_lights {two_step:.3f} ms = {two_step / fused_ms:.2f} x the fused kernel; the two frames are "
              f"{'byte-identical' if same else 'DIFFERENT'}")
        return 0 if same else 1


COPY_TBS = 6.29  # a float4 copy kernel on this chip (the ceiling a streaming kernel is held against)
SCATTER_BYTES_IN, SCATTER_BYTES_OUT = 112, 132  # per record with a hit, both channels (include/ptrace_scatter.h)


def scatter(args):
    import time

    import torch

    from pytracer_amd import abi, flatten, hostmodel as hm, rays as rb, scenes, shaders
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer
    from pytracer_amd.tracer import GpuImageTracer

    W, H = args.width, args.height
    n = W * H
    world = scenes.synthetic_world(32, with_plane=True)
    flat = flatten.flatten_world(world)
    camera = scenes.synthetic_camera(W, H)
    cam = flatten.flatten_camera(camera)
    p_hits = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    with DeviceScene(flat) as ds:
        frame = ds.render_hits(cam, p_hits, abi.HIT_ALL)
        hit = int(frame.hit.sum())
        buf = torch.from_numpy(frame.buffer).cuda()
        base = buf.data_ptr()
        at = lambda ch, comp=0: base + abi.hits_plane_offset(p_hits, abi.HIT_ALL, ch, comp)  # noqa: E731
        pcg = torch.from_numpy(rb.pcg_streams(42, 54 + np.arange(n, dtype=np.uint64)).view(np.int64)).cuda()
        out = DeviceBuffer((rb.scatter_bytes(n, rb.SCAT_ALL),), np.uint8)
        ds.slot_table()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        print(f"C2 {W}x{H}: {n} records in the hit-record frame, {hit} with a hit; {SCATTER_BYTES_IN} B in + {SCATTER_BYTES_OUT} B out per record")
        for roulette in (0, 1):
            def go():
                ds.scatter(base, at(abi.HIT_POINT), at(abi.HIT_NORMAL), at(abi.HIT_UV), at(abi.HIT_RAY, 3), pcg, roulette, "all",
                           device=True, stream=stream.cuda_stream, out=out, n=n)

            for _ in range(args.warmup):
                go()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                go()
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.steps
            sc = rb.ScatteredRays(out.numpy(), n)
            tbs = n * (SCATTER_BYTES_IN + SCATTER_BYTES_OUT) / (ms * 1e-3) / 1e12
            print(f"scatter roulette={roulette} (weight, emitted) {n:8d} records  {ms:8.3f} ms  {n / ms / 1e3:8.1f} Mrecord/s  "
                  f"{tbs:5.2f} TB/s effective = {tbs / COPY_TBS:.2f} x the {COPY_TBS} TB/s of a float4 copy  "
                  f"({int((sc.status == 1).sum())} scattered, {int((sc.status == 0).sum())} terminated)")
    # the whole route beside the fused renderer
    bg = hm.Color(0.1, 0.2, 0.3)
    images = {}
    for label, make in (("fused PathTracer", lambda t: hm.PathTracer(world, bg, hm.PCG(45, 54), 1, 3, 2)),
                        ("PathTracerShader", lambda t: shaders.PathTracerShader(world, t, bg, hm.PCG(45, 54), 1, 3, 2))):
        image = hm.HdrImage(W, H)
        tracer = GpuImageTracer(image, camera, samples_per_side=0, pcg=hm.PCG(45, 54), pcg_mode="sample")
        func = make(tracer)
        wall = []
        for _ in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            tracer.fire_all_rays(func)
            wall.append((time.perf_counter() - t0) * 1e3)
        images[label] = np.array(image.array)
        kernel = f", kernel {tracer.last_stats.kernel_ms:.3f} ms" if label.startswith("fused") else ""
        print(f"{label:18s} num_of_rays=1 max_depth=3 limit=2: fire_all_rays {float(np.median(wall[args.warmup:])):9.3f} ms wall{kernel}  "
              f"(last_path {tracer.last_path})")
        tracer.close()
    same = images["fused PathTracer"].tobytes() == images["PathTracerShader"].tobytes()
    print(f"the two frames are {'byte-identical' if same else 'DIFFERENT'}")
    return 0 if same else 1


def radiance(args):
    import torch

    from pytracer_amd import abi, flatten, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer, DeviceSpan

    W, H = args.width, args.height
    n = W * H
    D, LIMIT, BG = 3, 3, (0.1, 0.2, 0.3)
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    cam = flatten.flatten_camera(scenes.synthetic_camera(W, H))
    p_hits = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    ok = True
    with DeviceScene(flat) as ds:
        frame = ds.render_hits(cam, p_hits, abi.HIT_RAY)
        block = rb.ray_planes(frame.ray_origin.reshape(n, 3), frame.ray_dir.reshape(n, 3))
        rays_dev = torch.from_numpy(block).cuda()
        gen = rb.pcg_streams(45, 54 + np.arange(n, dtype=np.uint64))
        pcg_dev = torch.from_numpy(gen.view(np.int64)).cuda()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()

        def timed(go, steps):
            for _ in range(args.warmup):
                go()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(steps):
                go()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / steps

        print(f"C2 {W}x{H}: {n} primary rays, max_depth={D}, russian_roulette_limit={LIMIT}")
        for N in (1, 10):
            steps = args.steps if N == 1 else max(2, args.steps // 3)
            ws = DeviceBuffer((ds.radiance_workspace_bytes(n, N, D),), np.uint8)
            out = DeviceBuffer((rb.radiance_bytes(n, rb.RAD_ALL),), np.uint8)
            ms = timed(lambda: ds.radiance(rays_dev, pcg_dev, N, D, LIMIT, BG, 0, "all", device=True, stream=stream.cuda_stream, out=out,
                                           workspace=ws), steps)
            res = rb.RayRadiance(out.numpy(), n)
            traced = int(res.n_rays.sum())
            par = abi.make_params(W, H, abi.RENDERER_PATHTRACER, samples_per_side=0, num_of_rays=N, max_depth=D, rr_limit=LIMIT,
                                  pcg_mode=abi.PCG_SAMPLE, path_state=45, path_seq=54, background=BG)
            fused_ms = []
            for _ in range(args.warmup + steps):
                img = ds.render(cam, par)
                fused_ms.append(ds.stats().kernel_ms)
            fused_ms = float(np.median(fused_ms[args.warmup:]))
            same = np.ascontiguousarray(res.radiance).reshape(H, W, 3).tobytes() == np.ascontiguousarray(img, dtype=np.float64).tobytes()
            ok = ok and same
            print(f"radiance num_of_rays={N:2d}  {ms:9.3f} ms  {traced:9d} rays traced  {traced / ms / 1e3:8.1f} Mray/s  "
                  f"workspace {ws.nbytes / 2 ** 20:.1f} MiB  | fused frame kernel(s) {fused_ms:9.3f} ms (kernel {ds.stats().kernel}, "
                  f"{int(ds.stats().n_rays)} rays): the query takes {ms / fused_ms:.2f} x; frames {'byte-identical' if same else 'DIFFERENT'}")
            if N != 1:
                continue
            # the chain of the four steps before, in HBM: trace, then per depth scatter and trace
            ALL = rb.RAY_CHANNELS
            hit_bufs = [DeviceBuffer((rb.rays_bytes(n, ALL),), np.uint8) for _ in range(2)]
            scat_bufs = [DeviceBuffer((rb.scatter_bytes(n, rb.SCAT_ALL),), np.uint8) for _ in range(2)]
            ds.slot_table()
            soff = lambda sel, comp=0: rb.scatter_plane_offset(n, rb.SCAT_ALL, sel, comp)  # noqa: E731

            def planes(buf):
                base = buf.data_ptr()
                return [base] + [base + rb.rays_plane_offset(n, ALL, False, ch, 0) for ch in (abi.HIT_POINT, abi.HIT_NORMAL, abi.HIT_UV)]

            def chain():
                st = stream.cuda_stream
                hits = ds.trace_rays(rays_dev, ALL, device=True, stream=st, out=hit_bufs[0])
                dirs, pcg = rays_dev.data_ptr() + 3 * n * 8, pcg_dev
                for depth in range(D):
                    sc = ds.scatter(*planes(hits), dirs, pcg, depth >= LIMIT, "all", device=True, stream=st, out=scat_bufs[depth & 1], n=n)
                    hits = ds.trace_rays(DeviceSpan(sc, 64 * n, soff(rb.SCAT_RAYS)), ALL, device=True, stream=st, out=hit_bufs[(depth + 1) & 1])
                    dirs = sc.data_ptr() + soff(rb.SCAT_RAYS, 3)
                    pcg = (sc.data_ptr() + soff(rb.SCAT_PCG, 0), sc.data_ptr() + soff(rb.SCAT_PCG, 1))

            chain_ms = timed(chain, steps)
            print(f"chain in HBM: trace + {D} x (scatter + trace)  {chain_ms:9.3f} ms (7 launches; without the last depth's scatter and the "
                  f"sums): the query takes {ms / chain_ms:.2f} x")
    return 0 if ok else 1


def gather(args):
    import torch

    from pytracer_amd import abi, flatten, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer, DeviceSpan

    W, H = args.width, args.height
    D, LIMIT, BG, S0, Q0 = 3, 3, (0.1, 0.2, 0.3), 45, 54
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    cam = flatten.flatten_camera(scenes.synthetic_camera(W, H))
    p_hits = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    ok = True
    with DeviceScene(flat) as ds:
        frame = ds.render_hits(cam, p_hits, abi.HIT_POINT | abi.HIT_NORMAL | abi.HIT_RAY)
        hit = np.asarray(frame.hit).reshape(-1)
        points, normals = np.asarray(frame.point).reshape(-1, 3)[hit], np.asarray(frame.normal).reshape(-1, 3)[hit]
        origins, dirs = np.asarray(frame.ray_origin).reshape(-1, 3)[hit], np.asarray(frame.ray_dir).reshape(-1, 3)[hit]
        # a shape whose BRDF is diffuse and whose pigment is not black: the scatter query, told that every record lies on it, makes
        # DiffuseBRDF.scatter_ray at the record's own point and normal -- the gather's hemisphere ray
        one = np.zeros((1, 3))
        diffuse = next(s for s in range(flat.n_shapes)
                       if (lambda sc: sc.status[0] == 1 and sc.rays[6, 0] == 1.0e-3)(ds.scatter([s], one, one + 1.0, np.zeros((1, 2)), one + 1.0,
                                                                                                 rb.pcg_streams(S0, [Q0]), False, "none")))
        stream = torch.cuda.Stream()
        st = stream.cuda_stream

        def timed(go, steps, warmup):
            for _ in range(warmup):
                go()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(steps):
                go()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / steps

        print(f"C2 {W}x{H}: {points.shape[0]} first hits, max_depth={D}, russian_roulette_limit={LIMIT}; sample k of record i draws from "
              f"PCG({S0}, {Q0} + i K + k)")
        for K, N, every in ((16, 1, 1), (64, 1, 8), (16, 2, 1)):
            pts, nrm = np.ascontiguousarray(points[::every].T), np.ascontiguousarray(normals[::every].T)
            m = pts.shape[1]
            total = m * K
            pts_dev, nrm_dev = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
            # -- the gather: records in, means out
            ws = DeviceBuffer((ds.gather_workspace_bytes(m, K, N, D),), np.uint8)
            out = DeviceBuffer((rb.gather_bytes(m, rb.GATHER_ALL),), np.uint8)
            torch.cuda.synchronize()
            ms = timed(lambda: ds.gather(pts_dev, nrm_dev, K, S0, None, None, N, D, LIMIT, BG, 0, "all", init_seq=Q0, device=True, stream=st,
                                         out=out, workspace=ws), args.steps, args.warmup)
            res = rb.GatheredRadiance(out.numpy(), m)
            traced = int(res.n_rays.sum())
            # -- today's route, its host work left out: the n K sample rays and generators prepared in HBM (not timed) ...
            rep = lambda t: t.repeat_interleave(K, dim=1).contiguous()  # noqa: E731  (record-major: sample j = i K + k)
            gen_dev = torch.from_numpy(rb.pcg_streams(S0, Q0 + np.arange(total, dtype=np.uint64)).view(np.int64)).cuda()
            shape_dev = torch.full((total,), diffuse, dtype=torch.int32, device="cuda")
            uv_dev = torch.zeros((2, total), dtype=torch.float64, device="cuda")
            sample_pts, sample_nrm = rep(pts_dev), rep(nrm_dev)
            torch.cuda.synchronize()
            sc = ds.scatter(shape_dev, sample_pts, sample_nrm, uv_dev, sample_nrm, gen_dev, False, "none", device=True, stream=st, n=total)
            soff = lambda sel, comp=0: rb.scatter_plane_offset(total, 0, sel, comp)  # noqa: E731
            rays_span = DeviceSpan(sc, 64 * total, soff(rb.SCAT_RAYS))
            pcg_pair = (sc.data_ptr() + soff(rb.SCAT_PCG, 0), sc.data_ptr() + soff(rb.SCAT_PCG, 1))
            del shape_dev, uv_dev, sample_pts, sample_nrm, gen_dev
            # ... then the radiance query on them, timed the same way
            rws = DeviceBuffer((ds.radiance_workspace_bytes(total, N, D),), np.uint8)
            rout = DeviceBuffer((rb.radiance_bytes(total, rb.RAD_COUNT),), np.uint8)
            route_ms = timed(lambda: ds.radiance(rays_span, pcg_pair, N, D, LIMIT, BG, 0, "count", device=True, stream=st, out=rout,
                                                 workspace=rws, n=total), args.steps, args.warmup)
            rad = rb.RayRadiance(rout.numpy(), total, "count")
            acc = np.zeros((m, 3))
            per_sample = np.asarray(rad.radiance).reshape(m, K, 3)
            for k in range(K):
                acc = acc + per_sample[:, k, :]
            same = (acc * (1.0 / K)).tobytes() == np.ascontiguousarray(res.radiance).tobytes() and \
                np.array_equal(np.asarray(rad.n_rays).reshape(m, K).sum(axis=1, dtype=np.uint64), res.n_rays)
            ok = ok and same
            print(f"gather K={K:2d} num_of_rays={N}  {m:7d} records  {ms:9.3f} ms  {traced:10d} rays traced  {traced / ms / 1e3:8.1f} Mray/s  "
                  f"workspace {ws.nbytes / 2 ** 20:.1f} MiB  | path_radiance on the same {total} sample rays in HBM {route_ms:9.3f} ms: the gather "
                  f"takes {ms / route_ms:.2f} x; its output {'equals' if same else 'DIFFERS FROM'} the host's ordered sum of theirs bit for bit")
            del sc, rout, rws, rad, per_sample
            if N != 1:
                continue
            # -- for comparison: num_of_rays = K on the record's one primary ray (another estimator: one generator per record)
            block = torch.from_numpy(rb.ray_planes(origins[::every], dirs[::every])).cuda()
            one_gen = torch.from_numpy(rb.pcg_streams(S0, Q0 + np.arange(m, dtype=np.uint64)).view(np.int64)).cuda()
            tws = DeviceBuffer((ds.radiance_workspace_bytes(m, K, D),), np.uint8)
            tout = DeviceBuffer((rb.radiance_bytes(m, rb.RAD_COUNT),), np.uint8)
            torch.cuda.synchronize()
            tree_ms = timed(lambda: ds.radiance(block, one_gen, K, D, LIMIT, BG, 0, "count", device=True, stream=st, out=tout, workspace=tws),
                            2, 1)
            tree_rays = int(rb.RayRadiance(tout.numpy(), m, "count").n_rays.sum())
            print(f"    radiance query, num_of_rays={K} on one primary ray per record (another estimator): {tree_ms:9.3f} ms, {tree_rays} rays "
                  f"traced, {tree_rays / tree_ms / 1e3:.1f} Mray/s")
    return 0 if ok else 1


def bake(args):
    import torch

    from pytracer_amd import abi, flatten, hostmodel as hm, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer, DeviceSpan

    M, K, N, D, LIMIT, DEPTH, BG, S0, Q0 = args.map, args.samples, 1, 3, 3, 1, (0.1, 0.2, 0.3), 45, 54
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    shape = next(i for i in range(1, flat.n_shapes) if flat.kind[i] == abi.SHAPE_SPHERE and flat.brdf_kind[i] == abi.BRDF_DIFFUSE)
    texels = M * M
    ok = True
    with DeviceScene(flat) as ds:
        stream = torch.cuda.Stream()
        st = stream.cuda_stream

        def timed(go):
            for _ in range(args.warmup):
                go()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                go()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / args.steps

        # the gather's records: the texel centres' surface points, made in HBM
        uv = np.ascontiguousarray(np.moveaxis(rb.texel_centres(M, M), -1, 0)).reshape(2, texels)
        uv_dev = torch.from_numpy(uv).cuda()
        shape_dev = torch.full((texels,), shape, dtype=torch.int32, device="cuda")
        points = DeviceBuffer((6, texels), np.float64)
        torch.cuda.synchronize()
        points_ms = timed(lambda: ds.surface_points(shape_dev, uv_dev, None, device=True, stream=st, out=points))
        pts, nrm = DeviceSpan(points, 24 * texels, 0), DeviceSpan(points, 24 * texels, 24 * texels)
        gws = DeviceBuffer((ds.gather_workspace_bytes(texels, K, N, D, DEPTH),), np.uint8)
        gout = DeviceBuffer((rb.gather_bytes(texels, rb.GATHER_ALL),), np.uint8)
        bws = DeviceBuffer((ds.bake_workspace_bytes(M, M, K, N, D, DEPTH),), np.uint8)
        bout = DeviceBuffer((rb.bake_bytes(texels, rb.BAKE_ALL),), np.uint8)
        queries = {
            "gather on the centres' records": lambda: ds.gather(pts, nrm, K, S0, None, None, N, D, LIMIT, BG, DEPTH, "all", init_seq=Q0,
                                                                 device=True, stream=st, out=gout, workspace=gws, n=texels),
            "bake, centres (no jitter)": lambda: ds.bake(shape, M, M, K, 1, False, None, S0, Q0, N, D, LIMIT, BG, DEPTH, "all", device=True,
                                                         stream=st, out=bout, workspace=bws),
            "bake, jitter": lambda: ds.bake(shape, M, M, K, 1, True, None, S0, Q0, N, D, LIMIT, BG, DEPTH, "all", device=True, stream=st,
                                            out=bout, workspace=bws),
        }
        rounds = {name: [] for name in queries}
        kept = {}
        for _ in range(args.repeats):  # alternating: a drift of the machine meets all three alike
            for name, go in queries.items():
                rounds[name].append(timed(go))
                kept[name] = (gout if name.startswith("gather") else bout).numpy().copy()
        print(f"C2, shape {shape} (a diffuse sphere): {M}x{M} texels x {K} samples = {texels * K} hemisphere rays, num_of_rays={N}, max_depth={D}, "
              f"limit={LIMIT}, depth={DEPTH}; {args.repeats} alternating rounds of {args.warmup} warm-up + {args.steps} timed launches")
        print(f"surface_points for the {texels} texel centres: {points_ms:.3f} ms (not part of the gather's time)")
        med = {}
        for name, ms in rounds.items():
            med[name] = float(np.median(ms))
            traced = int(kept[name][24 * texels:].view(np.uint64).sum())
            print(f"{name:32s} median {med[name]:9.3f} ms  spread {(max(ms) - min(ms)) / med[name]:6.2%}  rounds {' '.join(f'{x:.3f}' for x in ms)}  "
                  f"{traced} rays traced, {traced / med[name] / 1e3:.1f} Mray/s")
        same = kept["bake, centres (no jitter)"].tobytes() == kept["gather on the centres' records"].tobytes()
        ok = ok and same
        base = med["gather on the centres' records"]
        print(f"bake / gather: centres {med['bake, centres (no jitter)'] / base:.3f} x, jitter {med['bake, jitter'] / base:.3f} x (bar: 1.25 x); the centre-mode "
              f"map {'equals' if same else 'DIFFERS FROM'} the gather's output bit for bit")
    # the purpose, as two times: the baked demo world under FlatRenderer beside the path tracer at the CLI's defaults
    W, H = 640, 480
    world, camera = scenes.demo_world()
    cam = flatten.flatten_camera(hm.PerspectiveCamera(screen_distance=1.0, aspect_ratio=W / H, transformation=camera.transformation))
    with DeviceScene(flatten.flatten_world(world)) as ds:
        wq = rb.WorldQueries(ds)
        maps = {i: wq.outgoing_map(i, 256, 256, 64, init_state=S0, num_of_rays=1, max_depth=3) for i in (0, 1)}
        par = abi.make_params(W, H, abi.RENDERER_PATHTRACER, samples_per_side=1, num_of_rays=10, max_depth=3, pcg_mode=abi.PCG_SAMPLE,
                              path_state=45, path_seq=54)
        path_ms = []
        for _ in range(args.warmup + args.steps):
            ds.render(cam, par)
            path_ms.append(ds.stats().kernel_ms)
    with DeviceScene(flatten.flatten_world(scenes.baked_world(world, maps))) as ds:
        par = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
        flat_ms = []
        for _ in range(args.warmup + 10 * args.steps):
            ds.render(cam, par)
            flat_ms.append(ds.stats().kernel_ms)
        kernel = ds.stats().kernel
    path, flat_t = float(np.median(path_ms[args.warmup:])), float(np.median(flat_ms[args.warmup:]))
    print(f"demo {W}x{H}: path-traced frame (num_of_rays=10, max_depth=3) kernels {path:.3f} ms; flat frame of the baked world (planes 0 and 1 "
          f"as 256x256 maps at 64 samples) kernel {flat_t * 1e3:.1f} us (kernel {kernel}): {path / flat_t:.0f} x")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
