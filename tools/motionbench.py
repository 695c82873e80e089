#!/usr/bin/env python3
"""Times the motion accumulate query (libptrace_motion.so) on one GPU beside the weighted accumulate query it extends (the parent's
kernel from the parent's library, measured in the same run), and measures what following a moving shape buys a sequence.

    python tools/motionbench.py [--width 1280] [--height 720] [--warmup 10] [--steps 100] [--repeats 5] [--no-quality] [--output FILE]

Workload: tools/weightedbench.py's.  C2 (32 spheres + checkered ground plane) at ``width x height``; two hit frames of the same camera
resident in HBM, a 4-sample gather of the frame, and one weighted accumulation from an empty history as the frame before.  Timed
ALTERNATING over the jobs, ``--repeats`` rounds of ``--warmup`` + ``--steps`` calls each between two events on one stream, no host
synchronisation inside the window:

    weighted              one pt_rays_weighted_accumulate_device call (the parent's kernel)
    motion, no tables     one pt_rays_motion_accumulate_device call with n_shapes = 0
    motion, static (a)    the same with a table of all the world's shapes whose `moved` is 0 everywhere
    motion, all moved (b) every shape moved by a small translation (1e-3 along each axis: the taps still pass)
    motion, half (c)      the shapes of even index moved by it

Before anything is timed contracts C and D of include/ptrace_motion.h are checked on the whole frame: with the static table the three
outputs are the weighted query's bit for bit, and with table (b) they are the weighted query's on records moved on the host.

What binds the kernel is not determined here: that needs counters, collected in a run of their own.

The quality experiment (``--no-quality`` skips it): the demo world at 48x36, eight frames, 4 samples per pixel, 1 degree per frame,
the sphere translated by 0.1 along y per frame; RMS error of the accumulated E against a 1024-sample gather of the LAST world, for
``MotionAccumulator`` and for ``WeightedAccumulator`` on the same gathers, on the sphere's pixels, on the ground within two radii of
the sphere's foot (the shadow moved: the history there is stale whichever way it is fetched) and on the whole frame.  Needs torch
only to read the events."""
import argparse
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def quality(say):
    from pytracer_amd import hostmodel as hm, rays as rb, scenes
    from pytracer_amd.tracer import GpuImageTracer

    W, H, K, N, step, dy = 48, 36, 4, 8, 1.0, 0.1
    base, camera = scenes.demo_world()

    def world_at(f):
        world = copy.copy(base)
        world.shapes = list(base.shapes)
        sphere = copy.copy(base.shapes[2])
        sphere.transformation = hm.translation(hm.Vec(0.0, dy * f, 0.0)) * sphere.transformation
        world.shapes[2] = sphere
        return world

    tracer = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=0)
    try:
        black = hm.Color(0.0, 0.0, 0.0)
        follow, plain = None, None
        for f in range(N):
            world = world_at(f)
            tracer.camera = scenes.turned_camera(camera, step * f)
            frame = tracer.fire_all_hits(world)
            wq = tracer.world_queries(world)
            if follow is None:
                follow, plain = rb.MotionAccumulator(wq), rb.WeightedAccumulator(wq)
            index = np.asarray(frame.shape_index)[0]
            g = np.asarray(wq.hemisphere_radiance(frame, K, 42, None, 1, 10, 3, black, 1, "none", init_seq=54 + f * W * H * K).radiance)[0]
            taken = np.where(index >= 0, K, 0).astype(np.int32)
            e_follow, _ = follow.update(g, frame, tracer.camera, samples=taken, world=world, queries=wq)
            plain.queries = wq
            e_plain, _ = plain.update(g, frame, tracer.camera, samples=taken)
        reference = np.asarray(wq.hemisphere_radiance(frame, 1024, 42, None, 1, 10, 3, black, 1, "none", init_seq=10 ** 9).radiance)[0]
        point = np.asarray(frame.point)[0]
        foot_y = dy * (N - 1)
        regions = (("the sphere's pixels", index == 2),
                   ("the ground within two radii of the foot", (index == 1) & (np.hypot(point[..., 0], point[..., 1] - foot_y) <= 2.0)),
                   ("the whole frame", index >= 0))
        rms = lambda a, where: float(np.sqrt(np.mean((a[where] - reference[where]) ** 2)))  # noqa: E731
        say(f"QUALITY: demo world {W}x{H}, {N} frames of {K} samples, {step:g} degree(s) per frame, the sphere {dy:g} along y per frame; RMS error "
            f"of the accumulated E against a 1024-sample gather of the last world; one frame alone: {rms(g, index >= 0):.5f}")
        for name, where in regions:
            a, b = rms(e_follow, where), rms(e_plain, where)
            longer = int((np.asarray(follow.count)[where] >= 2).sum()), int((np.asarray(plain.count)[where] >= 2).sum())
            say(f"    {name:42s} {int(where.sum()):5d} px   MotionAccumulator {a:.5f}   WeightedAccumulator {b:.5f}   ratio {a / b:.3f}   "
                f"histories >= 2: {longer[0]} / {longer[1]}   mean length {np.asarray(follow.count)[where].mean():.2f} / "
                f"{np.asarray(plain.count)[where].mean():.2f}")
    finally:
        tracer.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true", help="skip the quality experiment")
    ap.add_argument("--output", type=str, default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch

    from pytracer_amd import _motion_lib, abi, flatten, hostmodel as hm, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    W, H, K = args.width, args.height, 4
    m = W * H
    world = scenes.synthetic_world(32, with_plane=True)
    flat = flatten.flatten_world(world)
    S = len(world.shapes)
    camera = scenes.synthetic_camera(W, H)
    par = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    ok = True
    say(f"library: {_motion_lib.lib_path()}")
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

        def frame_in_hbm():
            hits = DeviceBuffer((abi.hits_bytes(par, abi.HIT_ALL),), np.uint8)
            ds.render_hits_into(flatten.flatten_camera(camera), par, abi.HIT_ALL, hits, stream=st)
            return rb.DeviceGuides.of_hit_buffer(hits, par, abi.HIT_ALL)

        g0, g1 = frame_in_hbm(), frame_in_hbm()
        gathered = DeviceBuffer((rb.gather_bytes(m, 0),), np.uint8)
        ds.gather(g1.point, g1.normal, K, 42, None, g1.shape_index, 1, 3, 3, (0.1, 0.2, 0.3), 1, "none", device=True, stream=st, out=gathered, n=m)
        f3 = lambda: DeviceBuffer((3, m), np.float64)  # noqa: E731
        i1 = lambda: DeviceBuffer((m,), np.int32)  # noqa: E731
        hist_c, hist_m, hist_n, scratch_c, scratch_m = f3(), f3(), i1(), f3(), f3()
        zero = ds.weighted_clear(i1(), stream=st)
        fours = torch.full((m,), K, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        # the history: the same gather accumulated from nothing, as the frame before (lengths of 1 and weights of 4 at every hit)
        ds.weighted(gathered, fours, g0.shape_index, g0.normal, g0.point, scratch_c, scratch_m, g1.shape_index, g1.normal, g1.point, zero, camera, W, H,
                    device=True, stream=st, out=hist_c, out_moments=hist_m, out_count=hist_n)
        outs = {key: (f3(), f3(), i1()) for key in ("weighted", "none", "static", "all", "half", "host")}

        def weighted(out, normal=None, point=None):
            ds.weighted(gathered, fours, g1.shape_index, g1.normal if normal is None else normal, g1.point if point is None else point, hist_c, hist_m,
                        g0.shape_index, g0.normal, g0.point, hist_n, camera, W, H, device=True, stream=st, out=out[0], out_moments=out[1],
                        out_count=out[2])

        def motion(out, tables):
            ds.motion(gathered, fours, g1.shape_index, g1.normal, g1.point, hist_c, hist_m, g0.shape_index, g0.normal, g0.point, hist_n, camera,
                      tables[0], tables[1], W, H, device=True, stream=st, out=out[0], out_moments=out[1], out_count=out[2])

        small = M_record(hm.translation(hm.Vec(-1e-3, -1e-3, -1e-3)))
        rows = np.array([small] * S)
        host_tables = {"static": (np.zeros(S, np.int32), rows), "all": (np.ones(S, np.int32), rows),
                       "half": ((np.arange(S) % 2 == 0).astype(np.int32), rows)}
        tables = {key: ds.motion_table(*t) for key, t in host_tables.items()}
        tables["none"] = (None, None)
        torch.cuda.synchronize()
        # contracts C and D on the whole frame
        weighted(outs["weighted"])
        for key in ("none", "static", "all", "half"):
            motion(outs[key], tables[key])
        raw = g1.keep.numpy()
        base = int(g1.keep.data_ptr())
        plane = lambda addr, dtype, n: raw[int(addr) - base: int(addr) - base + n].view(dtype)  # noqa: E731
        shape = plane(g1.shape_index, np.int32, 4 * m).copy()
        normal, point = (plane(a, np.float64, 24 * m).reshape(3, m).T.copy() for a in (g1.normal, g1.point))
        nm, pm = rb.move_records_host(shape, normal, point, *host_tables["all"])
        nm_dev, pm_dev = (torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (nm, pm))
        torch.cuda.synchronize()
        weighted(outs["host"], nm_dev, pm_dev)
        torch.cuda.synchronize()
        same = lambda a, b: all(x.numpy().tobytes() == y.numpy().tobytes() for x, y in zip(outs[a], outs[b]))  # noqa: E731
        c_ok, d_ok = same("none", "weighted") and same("static", "weighted"), same("all", "host")
        reaches = not same("all", "weighted")
        ok = ok and c_ok and d_ok
        lengths = {key: outs[key][2].numpy() for key in outs}
        moved_px = {key: int(((host_tables[key][0][np.clip(shape, 0, S - 1)] != 0) & (shape >= 0)).sum()) for key in host_tables}
        say(f"C2 at {W}x{H}: {m} records ({int((shape >= 0).sum())} hits, {S} shapes), a {K}-sample gather in HBM; histories of 2 after the "
            f"accumulation: weighted {int((lengths['weighted'] == 2).sum())}, all moved {int((lengths['all'] == 2).sum())}, half "
            f"{int((lengths['half'] == 2).sum())}; pixels whose shape moved: all {moved_px['all']}, half {moved_px['half']}; {args.repeats} alternating "
            f"rounds of {args.warmup} warm-up + {args.steps} timed calls")
        say(f"contract C (no tables and an all-static table against the weighted query, whole frame): {'bit for bit' if c_ok else 'DIFFERS'}; "
            f"contract D (every shape moved against the weighted query on records moved on the host): {'bit for bit' if d_ok else 'DIFFERS'}; "
            f"the small translation {'reaches' if reaches else 'DOES NOT reach'} the bits")
        jobs = {"weighted": lambda: timed(lambda: weighted(outs["weighted"])),
                "motion, no tables": lambda: timed(lambda: motion(outs["none"], tables["none"])),
                "motion, static (a)": lambda: timed(lambda: motion(outs["static"], tables["static"])),
                "motion, all moved (b)": lambda: timed(lambda: motion(outs["all"], tables["all"])),
                "motion, half (c)": lambda: timed(lambda: motion(outs["half"], tables["half"]))}
        rounds = {key: [] for key in jobs}
        for _ in range(args.repeats):
            for key, run in jobs.items():
                rounds[key].append(run())
        med = {key: float(np.median(r)) for key, r in rounds.items()}
        spread = {key: 100 * (max(r) - min(r)) / med[key] for key, r in rounds.items()}
        for key in jobs:
            say(f"{key:24s} {med[key] * 1e3:9.1f} us  spread {spread[key]:5.2f}%  rounds {' '.join(f'{x * 1e3:.1f}' for x in rounds[key])}")
        say(f"(a) motion with an all-static table / weighted = {med['motion, static (a)'] / med['weighted']:.3f}; without tables "
            f"{med['motion, no tables'] / med['weighted']:.3f}")
        say(f"(b) every shape moved / (a) = {med['motion, all moved (b)'] / med['motion, static (a)']:.3f}")
        say(f"(c) half the shapes moved / (a) = {med['motion, half (c)'] / med['motion, static (a)']:.3f}")
    if not args.no_quality:
        quality(say)
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


def M_record(transformation):
    """A row of the motion table from a ``Transformation`` that takes this frame's points to the previous frame's."""
    m, inv = transformation.m, transformation.invm
    return [m[i][j] for i in range(3) for j in range(4)] + [inv[j][i] for i in range(3) for j in range(3)] + [0.0, 0.0, 0.0]


if __name__ == "__main__":
    sys.exit(main())
