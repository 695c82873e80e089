#!/usr/bin/env python3
"""Times the three kernels of the gradient accumulate query (libptrace_gradient.so) on one GPU beside the motion accumulate query they
extend (the parent's kernel from the parent's library, measured in the same run), times the frame they make, and measures what
following the light buys a sequence in which a shadow moves.

    python tools/gradientbench.py [--width 1280] [--height 720] [--warmup 10] [--steps 100] [--repeats 5] [--no-quality] [--no-sweep] [--output FILE]

Workload: tools/motionbench.py's.  C2 (32 spheres + checkered ground plane) at ``width x height``; two hit frames of the same camera
resident in HBM, a 4-sample gather of the frame, and one accumulation from an empty history as the frame before.  Timed ALTERNATING
over the jobs, ``--repeats`` rounds of ``--warmup`` + ``--steps`` calls each between two events on one stream, no host synchronisation
inside the window:

    motion                      one pt_rays_motion_accumulate_device call, no tables (the parent's kernel)
    gradient, keep NULL         one pt_rays_gradient_accumulate_device call without a keep plane
    gradient, keep plane        the same with the plane the keep kernel made (half of the probes' old colours changed)
    probes                      one pt_rays_gradient_probes_device call, stratum 3
    keep                        one pt_rays_gradient_keep_device call, stratum 3, radius 1
    frame, motion               gather 4 + motion accumulate + variance estimate
    frame, gradient             gather 4 + probes + the probes' gather + keep + gradient accumulate + variance estimate
                                (the variance-guided filter behind both frames is the same launches and is not timed here)

Before anything is timed contract E of include/ptrace_gradient.h is checked on the whole frame (keep NULL and keep 1.0 against the
motion query, bit for bit), and contract G through the real gather (the probes gathered in the same scene: keep 1.0 in every bit).

What binds each kernel is not determined here: that needs counters, collected in a run of their own.

The quality experiment (``--no-quality`` skips it) is tools/motionbench.py's, unchanged: the demo world at 48x36, eight frames, 4
samples per pixel, 1 degree per frame, the sphere translated by 0.1 along y per frame; RMS error of the accumulated E against a
1024-sample gather of the LAST world, for ``GradientAccumulator`` and for ``MotionAccumulator`` on the same gathers, on the sphere's
pixels, on the ground within two radii of the sphere's foot and on the whole frame; also behind the variance-guided filter.  The sweep
(``--no-sweep`` skips it) runs it over gain 1..32, stratum 2..4 and radius 0..2.  Needs torch only to read the events."""
import argparse
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAINS, STRATA, RADII = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0), (2, 3, 4), (0, 1, 2)


def quality(say, sweep):
    from pytracer_amd import _gradient_lib, abi, flatten, hostmodel as hm, rays as rb, scenes
    from pytracer_amd.device import DeviceScene

    W, H, K, N, step, dy = 48, 36, 4, 8, 1.0, 0.1
    base, camera = scenes.demo_world()
    par = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    black = hm.Color(0.0, 0.0, 0.0)

    def world_at(f):
        world = copy.copy(base)
        world.shapes = list(base.shapes)
        sphere = copy.copy(base.shapes[2])
        sphere.transformation = hm.translation(hm.Vec(0.0, dy * f, 0.0)) * sphere.transformation
        world.shapes[2] = sphere
        return world

    frames = []
    try:
        for f in range(N):  # every frame keeps its scene: the next one gathers its probes there
            world, cam = world_at(f), scenes.turned_camera(camera, step * f)
            ds = DeviceScene(flatten.flatten_world(world))
            wq = rb.WorldQueries(ds)
            frame = ds.render_hits(flatten.flatten_camera(cam), par, abi.HIT_ALL)
            seq = 54 + f * W * H * K
            g = np.asarray(wq.hemisphere_radiance(frame, K, 42, None, 1, 10, 3, black, 1, "none", init_seq=seq).radiance)[0]
            frames.append((world, cam, ds, wq, frame, g, seq))
        world, cam, ds, wq, frame, g, _ = frames[-1]
        index, point = np.asarray(frame.shape_index)[0], np.asarray(frame.point)[0]
        reference = np.asarray(wq.hemisphere_radiance(frame, 1024, 42, None, 1, 10, 3, black, 1, "none", init_seq=10 ** 9).radiance)[0]
        foot_y = dy * (N - 1)
        regions = (("the sphere's pixels", index == 2),
                   ("the ground within two radii of the foot", (index == 1) & (np.hypot(point[..., 0], point[..., 1] - foot_y) <= 2.0)),
                   ("the whole frame", index >= 0))
        rms = lambda a, where: float(np.sqrt(np.mean((a[where] - reference[where]) ** 2)))  # noqa: E731

        def run(make):
            acc = make(frames[0][3])
            for world_f, cam_f, _, wq_f, frame_f, g_f, seq_f in frames:
                kw = dict(probe=dict(samples=K, init_state=42, init_seq=seq_f, max_depth=10, russian_roulette_limit=3, background=black, depth=1)) \
                    if isinstance(acc, rb.GradientAccumulator) else {}
                e, variance = acc.update(g_f, frame_f, cam_f, samples=np.where(np.asarray(frame_f.shape_index)[0] >= 0, K, 0).astype(np.int32),
                                         world=world_f, queries=wq_f, **kw)
            filtered, _ = wq.variance_filtered(e, frame, variance=variance)
            return e, np.asarray(filtered), np.asarray(acc.count), getattr(acc, "keep", None)

        e_m, f_m, n_m, _ = run(lambda q: rb.MotionAccumulator(q))
        e_g, f_g, n_g, keep = run(lambda q: rb.GradientAccumulator(q))
        d = _gradient_lib.KEEP_DEFAULTS
        say(f"QUALITY: demo world {W}x{H}, {N} frames of {K} samples, {step:g} degree(s) per frame, the sphere {dy:g} along y per frame; RMS error "
            f"of the accumulated E against a 1024-sample gather of the last world; one frame alone: {rms(g, index >= 0):.5f}; defaults stratum "
            f"{d['stratum']}, radius {d['radius']}, gain {d['gain']:g}; keep < 1 at {int((np.asarray(keep) < 1).sum())} of {int((index >= 0).sum())} hit pixels")
        for name, where in regions:
            a, b = rms(e_g, where), rms(e_m, where)
            fa, fb = rms(f_g, where), rms(f_m, where)
            say(f"    {name:42s} {int(where.sum()):5d} px   GradientAccumulator {a:.5f}   MotionAccumulator {b:.5f}   ratio {a / b:.3f}   "
                f"behind the filter {fa:.5f} / {fb:.5f}   ratio {fa / fb:.3f}   mean length {n_g[where].mean():.2f} / {n_m[where].mean():.2f}")
        if sweep:
            foot, whole = regions[1][1], regions[2][1]
            say(f"SWEEP (RMS on the foot region / the whole frame; MotionAccumulator {rms(e_m, foot):.5f} / {rms(e_m, whole):.5f}):")
            best = None
            for s in STRATA:
                for radius in RADII:
                    row = []
                    for gain in GAINS:
                        e, _, _, _ = run(lambda q: rb.GradientAccumulator(q, stratum=s, radius=radius, gain=gain))
                        a, b = rms(e, foot), rms(e, whole)
                        row.append(f"{a:.5f}/{b:.5f}")
                        if b <= rms(e_m, whole) and (best is None or a < best[0]):
                            best = (a, b, s, radius, gain)
                    say(f"    stratum {s} radius {radius}  gain " + "  ".join(f"{g_:g}: {r}" for g_, r in zip(GAINS, row)))
            if best is None:
                say("    no setting lowers the foot region's error without raising the whole frame's above MotionAccumulator's")
            else:
                say(f"    best on the foot region without raising the whole frame's error: stratum {best[2]}, radius {best[3]}, gain {best[4]:g} "
                    f"({best[0]:.5f} / {best[1]:.5f})")
    finally:
        for item in frames:
            item[2].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true", help="skip the quality experiment")
    ap.add_argument("--no-sweep", action="store_true", help="skip the sweep over gain, stratum and radius")
    ap.add_argument("--output", type=str, default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch

    from pytracer_amd import _gradient_lib, abi, flatten, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    W, H, K, s, radius = args.width, args.height, 4, 3, 1
    m, ns = W * H, _gradient_lib.strata(args.width, args.height, 3)
    world = scenes.synthetic_world(32, with_plane=True)
    flat = flatten.flatten_world(world)
    camera = scenes.synthetic_camera(W, H)
    par = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    ok = True
    say(f"library: {_gradient_lib.lib_path()}")
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
        workspace = DeviceBuffer((ds.gather_workspace_bytes(m, K, 1, 3, 1),), np.uint8)

        def gather():
            ds.gather(g1.point, g1.normal, K, 42, None, g1.shape_index, 1, 3, 3, (0.1, 0.2, 0.3), 1, "none", device=True, stream=st, out=gathered,
                      workspace=workspace, n=m)

        gather()
        f3 = lambda: DeviceBuffer((3, m), np.float64)  # noqa: E731
        i1 = lambda: DeviceBuffer((m,), np.int32)  # noqa: E731
        hist_c, hist_m, hist_n, scratch_c, scratch_m = f3(), f3(), i1(), f3(), f3()
        zero = ds.motion_clear(i1(), stream=st)
        fours = torch.full((m,), K, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ds.motion(gathered, fours, g0.shape_index, g0.normal, g0.point, scratch_c, scratch_m, g1.shape_index, g1.normal, g1.point, zero, camera, None,
                  None, W, H, device=True, stream=st, out=hist_c, out_moments=hist_m, out_count=hist_n)
        outs = {key: (f3(), f3(), i1()) for key in ("motion", "null", "ones", "plane")}
        variance = DeviceBuffer((m,), np.float64)
        probes = (DeviceBuffer((ns,), np.int32), DeviceBuffer((3, ns), np.float64), DeviceBuffer((3, ns), np.float64), DeviceBuffer((ns,), np.uint64))
        old = DeviceBuffer((max(rb.gather_bytes(ns, 0), 8),), np.uint8)
        old_ws = DeviceBuffer((ds.gather_workspace_bytes(ns, K, 1, 3, 1),), np.uint8)
        keep = DeviceBuffer((m,), np.float64)
        ones = torch.ones((m,), dtype=torch.float64, device="cuda")

        def motion(out):
            ds.motion(gathered, fours, g1.shape_index, g1.normal, g1.point, hist_c, hist_m, g0.shape_index, g0.normal, g0.point, hist_n, camera, None,
                      None, W, H, device=True, stream=st, out=out[0], out_moments=out[1], out_count=out[2])

        def accumulate(out, plane):
            ds.gradient_accumulate(gathered, fours, g1.shape_index, g1.normal, g1.point, hist_c, hist_m, g0.shape_index, g0.normal, g0.point, hist_n,
                                   camera, None, None, plane, W, H, device=True, stream=st, out=out[0], out_moments=out[1], out_count=out[2])

        def make_probes():
            ds.gradient_probes(g1.shape_index, g1.normal, g1.point, None, None, W, H, stratum=s, phase=1, samples=K, init_seq=54, device=True,
                               stream=st, out=probes)

        def probe_gather():
            ds.gather(probes[1], probes[2], K, 42, probes[3], probes[0], 1, 3, 3, (0.1, 0.2, 0.3), 1, "none", device=True, stream=st, out=old,
                      workspace=old_ws, n=ns)

        def make_keep(source=None):
            ds.gradient_keep(gathered, g1.shape_index, probes[0], old if source is None else source, W, H, stratum=s, radius=radius, gain=8.0,
                             device=True, stream=st, out=keep)

        def estimate(out):
            ds.variance_estimate(out[1], out[2], g1.shape_index, g1.normal, g1.point, W, H, device=True, stream=st, out=variance)

        # contracts E and G on the whole frame
        motion(outs["motion"])
        accumulate(outs["null"], None)
        accumulate(outs["ones"], ones)
        make_probes()
        probe_gather()
        make_keep()
        torch.cuda.synchronize()
        same = lambda a, b: all(x.numpy().tobytes() == y.numpy().tobytes() for x, y in zip(outs[a], outs[b]))  # noqa: E731
        e_ok = same("null", "motion") and same("ones", "motion")
        g_ok = keep.numpy().tobytes() == np.ones(m).tobytes()
        index = probes[0].numpy()
        # a keep plane that does something: half of the probes' old colours changed by a quarter
        changed = np.array(old.numpy()[: 24 * ns].view(np.float64).reshape(3, ns))
        changed[:, ::2] *= 0.75
        changed_dev = torch.from_numpy(changed).cuda()
        torch.cuda.synchronize()
        make_keep(changed_dev)
        torch.cuda.synchronize()
        below = int((keep.numpy() < 1.0).sum())
        accumulate(outs["plane"], keep)
        torch.cuda.synchronize()
        ok = ok and e_ok and g_ok and below > 0 and not same("plane", "motion")
        say(f"C2 at {W}x{H}: {m} records, {ns} probes of stratum {s} ({int((index >= 0).sum())} on hits), a {K}-sample gather in HBM; "
            f"{args.repeats} alternating rounds of {args.warmup} warm-up + {args.steps} timed calls")
        say(f"contract E (keep NULL and keep 1.0 against the motion query, whole frame): {'bit for bit' if e_ok else 'DIFFERS'}; contract G (the probes "
            f"gathered in the same scene): keep {'1.0 in every bit' if g_ok else 'DIFFERS FROM 1.0'}; with half the probes changed by a quarter "
            f"keep < 1 at {below} pixels")

        def frame_motion():
            gather()
            motion(outs["motion"])
            estimate(outs["motion"])

        def frame_gradient():
            gather()
            make_probes()
            probe_gather()
            make_keep()
            accumulate(outs["plane"], keep)
            estimate(outs["plane"])

        jobs = {"motion": lambda: timed(lambda: motion(outs["motion"])),
                "gradient, keep NULL": lambda: timed(lambda: accumulate(outs["null"], None)),
                "gradient, keep plane": lambda: timed(lambda: accumulate(outs["plane"], keep)),
                "probes": lambda: timed(make_probes),
                "keep": lambda: timed(lambda: make_keep(changed_dev)),
                "frame, motion": lambda: timed(frame_motion),
                "frame, gradient": lambda: timed(frame_gradient)}
        rounds = {key: [] for key in jobs}
        for _ in range(args.repeats):
            for key, run in jobs.items():
                rounds[key].append(run())
        med = {key: float(np.median(r)) for key, r in rounds.items()}
        spread = {key: 100 * (max(r) - min(r)) / med[key] for key, r in rounds.items()}
        for key in jobs:
            say(f"{key:24s} {med[key] * 1e3:9.1f} us  spread {spread[key]:5.2f}%  rounds {' '.join(f'{x * 1e3:.1f}' for x in rounds[key])}")
        say(f"gradient accumulate with keep NULL / motion = {med['gradient, keep NULL'] / med['motion']:.3f}; with a keep plane "
            f"{med['gradient, keep plane'] / med['motion']:.3f}")
        say(f"frame with the gradient chain / frame with the motion query = {med['frame, gradient'] / med['frame, motion']:.3f} "
            f"(probes + keep alone: {(med['probes'] + med['keep']) * 1e3:.1f} us)")
    if not args.no_quality:
        quality(say, not args.no_sweep)
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
