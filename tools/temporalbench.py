#!/usr/bin/env python3
"""Times the accumulate query (libptrace_temporal.so) on one GPU: beside its compulsory traffic, beside the filter it precedes and the
gathers it saves, and as a whole frame beside the frame it replaces.

    python tools/temporalbench.py [--width 1280] [--height 720] [--step-deg 1.0] [--warmup 10] [--steps 100] [--repeats 5] [--no-host]
                                  [--output FILE]

Workload: C2 (32 spheres + checkered ground plane) at ``width x height``.  Two hit frames are resident in HBM (``render_hits_into``):
the previous one and the current one, whose camera has turned by ``--step-deg`` about z; a 4-sample gather of each is resident in HBM
(``gather(device=True)``).  The previous frame's gather, accumulated from an empty history, is the history (every hit has the
length 1); the timed call accumulates the current frame onto it.  Timed ALTERNATING over the jobs, ``--repeats`` rounds of ``--warmup``
+ ``--steps`` calls each between two events on one stream, no host synchronisation inside the window:

    accumulate        one pt_rays_temporal_accumulate_device call
    filter            one pt_rays_denoise_device call, 4 passes, default parameters
    gather 4 / 16     the gathers of the current frame
    frame 4+a+f       gather 4, accumulate, filter: a TemporalGatherShader frame's device work
    frame 16+f        gather 16, filter: the DenoisedGatherShader frame it is meant to replace

The traffic floor of a call: 76 B read (shape, colour, point, normal) + 28 B written per pixel, plus the history it fetches -- 8 B
per tap looked at and 72 B per tap that passes the integer tests, at most 320 B per pixel, shared between neighbours through the
caches.  What binds the kernel is not determined here: that needs counters, collected in a run of their own.

The device's output must equal ``rays.temporal_host`` bit for bit (on the whole frame, unless ``--no-host``).  Needs torch only to
read the events."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--step-deg", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy mirror (and with it the bit comparison)")
    ap.add_argument("--output", type=str, default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch

    from pytracer_amd import abi, flatten, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer
    from pytracer_amd.hits import HitFrame

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    W, H = args.width, args.height
    m = W * H
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    before = scenes.synthetic_camera(W, H)
    now = scenes.turned_camera(before, args.step_deg)
    par = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
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

        def frame_in_hbm(camera):
            hits = DeviceBuffer((abi.hits_bytes(par, abi.HIT_ALL),), np.uint8)
            ds.render_hits_into(flatten.flatten_camera(camera), par, abi.HIT_ALL, hits, stream=st)
            return rb.DeviceGuides.of_hit_buffer(hits, par, abi.HIT_ALL)

        g0, g1 = frame_in_hbm(before), frame_in_hbm(now)
        gathered = {k: DeviceBuffer((rb.gather_bytes(m, 0),), np.uint8) for k in ("prev", 4, 16)}
        work = {k: DeviceBuffer((ds.gather_workspace_bytes(m, k, 1, 3, 1),), np.uint8) for k in (4, 16)}

        def gather(g, k, out, seq=54):
            ds.gather(g.point, g.normal, k, 42, None, g.shape_index, 1, 3, 3, (0.1, 0.2, 0.3), 1, "none", init_seq=seq, device=True, stream=st, out=out,
                      workspace=work[k], n=m)

        gather(g0, 4, gathered["prev"])
        gather(g1, 4, gathered[4], 54 + 4 * m)
        gather(g1, 16, gathered[16])
        zero = ds.temporal_clear(DeviceBuffer((m,), np.int32), stream=st)
        hist, hist_n = ds.temporal(gathered["prev"], g0.shape_index, g0.normal, g0.point, gathered[4], g1.shape_index, g1.normal, g1.point, zero, before,
                                   W, H, device=True, stream=st)
        acc, acc_n = DeviceBuffer((3, m), np.float64), DeviceBuffer((m,), np.int32)
        filtered = DeviceBuffer((3, m), np.float64)
        filter_work = DeviceBuffer((ds.denoise_workspace_bytes(W, H, passes=4),), np.uint8)

        def accumulate():
            ds.temporal(gathered[4], g1.shape_index, g1.normal, g1.point, hist, g0.shape_index, g0.normal, g0.point, hist_n, before, W, H, device=True,
                        stream=st, out=acc, out_count=acc_n)

        def filter_of(colour):
            ds.denoise(colour, g1.shape_index, g1.normal, g1.point, W, H, device=True, stream=st, out=filtered, workspace=filter_work, passes=4)

        def frame_new():
            gather(g1, 4, gathered[4], 54 + 4 * m)
            accumulate()
            filter_of(acc)

        def frame_old():
            gather(g1, 16, gathered[16])
            filter_of(gathered[16])

        accumulate()
        torch.cuda.synchronize()
        lengths = acc_n.numpy()
        frame0, frame1 = HitFrame(g0.keep.numpy(), par, abi.HIT_ALL), HitFrame(g1.keep.numpy(), par, abi.HIT_ALL)
        hit = int((np.asarray(frame1.shape_index) >= 0).sum())
        say(f"C2 at {W}x{H}: {m} records ({hit} hits), the camera turned by {args.step_deg:g} degree(s) since the previous frame; "
            f"{int((lengths >= 2).sum())} pixels found their history, {int((lengths == 1).sum())} started one; {args.repeats} alternating rounds of "
            f"{args.warmup} warm-up + {args.steps} timed calls")
        jobs = {"accumulate": accumulate, "filter": lambda: filter_of(gathered[4]), "gather 4": lambda: gather(g1, 4, gathered[4], 54 + 4 * m),
                "gather 16": lambda: gather(g1, 16, gathered[16]), "frame 4+a+f": frame_new, "frame 16+f": frame_old}
        rounds = {key: [] for key in jobs}
        for _ in range(args.repeats):
            for key, go in jobs.items():
                rounds[key].append(timed(go))
        med = {key: float(np.median(r)) for key, r in rounds.items()}
        spread = {key: 100 * (max(r) - min(r)) / med[key] for key, r in rounds.items()}
        for key in jobs:
            say(f"{key:12s} {med[key] * 1e3:9.1f} us  spread {spread[key]:5.2f}%")
        floor_us, most_us = m * 104 / 8e12 * 1e6, m * (104 + 320) / 8e12 * 1e6
        a = med["accumulate"]
        say(f"traffic floor of one accumulate call: {m} x (76 B read + 28 B written) = {m * 104 / 1e6:.0f} MB, {floor_us:.1f} us at 8 TB/s; with every tap's "
            f"history fetched and nothing shared, {most_us:.1f} us: the call takes {a * 1e3 / floor_us:.1f} x the first and {a * 1e3 / most_us:.1f} x the second")
        say(f"accumulate / filter = {a / med['filter']:.3f}; accumulate / gather 4 = {a / med['gather 4']:.3f}; accumulate / gather 16 = "
            f"{a / med['gather 16']:.3f}")
        say(f"frame (gather 4 + accumulate + filter) / frame (gather 16 + filter) = {med['frame 4+a+f'] / med['frame 16+f']:.3f}")
        if not args.no_host:
            accumulate()
            got = np.ascontiguousarray(acc.numpy()[:, :m].T).reshape(H, W, 3), acc_n.numpy().reshape(H, W)
            colour = lambda b: np.ascontiguousarray(b.numpy()[: 24 * m].view(np.float64).reshape(3, m).T)  # noqa: E731
            guides = lambda f: (np.asarray(f.shape_index)[0], np.asarray(f.normal)[0], np.asarray(f.point)[0])  # noqa: E731
            prev_colour = np.ascontiguousarray(hist.numpy()[:, :m].T)
            t0 = time.perf_counter()
            want = rb.temporal_host(colour(gathered[4]), *guides(frame1), prev_colour, *guides(frame0), hist_n.numpy(), before, W, H)
            host_s = time.perf_counter() - t0
            same = got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            ok = ok and same
            say(f"the numpy mirror on the same frame, once, wall time: {host_s:.2f} s, {host_s * 1e3 / a:.0f} x the query; the device's frame and lengths "
                f"{'equal' if same else 'DIFFER FROM'} it bit for bit")
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
