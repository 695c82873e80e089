#!/usr/bin/env python3
"""Throughput of ray batches (libptrace_rays.so: pt_rays_trace_device) on the C2 frame's rays, fed back as batches.

    python tools/raybench.py [--width 1280 --height 720 --warmup 3 --steps 10]

Three device-resident batches from BASELINE's C2 (32 spheres + ground plane): the frame's pixel-centre primary rays (as the
hit-record frame itself leaves them), the mirror bounces off their hits (d - 2 (d.n) n, tmin 1e-3) and the shadow segments
from the hit points to a light at (0, 0, 10) (any-hit).  Per batch: warm-up launches, then a timed loop of
``pt_rays_trace_device`` on a stream of its own between two events.  One process; prints Mray/s per batch and the
``pt_render_hits`` kernel time of the same frame beside the primary batch (that frame culls per tile; a batch cannot).
Needs torch only to put the batches into device memory and to read the events."""
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
    args = ap.parse_args()
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


if __name__ == "__main__":
    main()
