#!/usr/bin/env python3
"""Times the variance queries (libptrace_variance.so) on one GPU: the variance-guided filter beside the denoise query it extends
(measured in the same run), per tile and for the direct variant; the estimate with every pixel short of history and with none; the
moments kernel; and a whole frame beside the frame it replaces.

    python tools/variancebench.py [--width 1280] [--height 720] [--passes 4] [--warmup 10] [--steps 100] [--repeats 5] [--no-host]
                                  [--output FILE]

Workload: C2 (32 spheres + checkered ground plane) at ``width x height``.  Two hit frames of the same camera are resident in HBM
(``render_hits_into``; the accumulators read the previous frame's guides where the caller left them), a 4-sample gather of the frame is
resident in HBM (``gather(device=True)``), its moments, one accumulation of each from an empty history (every hit has the length 1)
and the variance estimated from them.  Timed ALTERNATING over the jobs, ``--repeats`` rounds of ``--warmup`` + ``--steps`` calls each
between two events on one stream, no host synchronisation inside the window:

    moments               one pt_rays_variance_moments_device call
    estimate all short    one pt_rays_variance_estimate_device call, min_history 4 on lengths of 1: every hit walks the 7x7 window
    estimate none short   the same with min_history 1: no window
    denoise               one denoise-query call, ``passes`` passes, default parameters (the geometry-only filter)
    variance filter ...   one pt_rays_variance_filter_device call, ``passes`` passes, default parameters: lds 16x16 / 32x8 / 64x4, direct
    frame 4+a+f           gather 4, accumulate, denoise: a TemporalGatherShader frame's device work
    frame 4+2a+e+vf       gather 4, moments, two accumulations, estimate, variance filter: a VarianceGuidedGatherShader frame's, with
                          every history long enough for the temporal estimate (the steady state); ", short": with none (the first frames)

The traffic floor of one filter pass: 84 B read (shape, colour, point, unit normal, variance) + 32 B written per pixel, plus the
prefilter's 12 B read + 8 B written and the 8 B of g.  What binds the kernels is not determined here: that needs counters, collected in
a run of their own.

The device's outputs must equal the mirrors of ``pytracer_amd.rays`` bit for bit (on the whole frame, unless ``--no-host``).  Needs torch
only to read the events."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("lds 16x16", dict(PTRACE_VR_VARIANT="lds", PTRACE_VR_TILE="16x16")), ("lds 32x8", dict(PTRACE_VR_VARIANT="lds", PTRACE_VR_TILE="32x8")),
            ("lds 64x4", dict(PTRACE_VR_VARIANT="lds", PTRACE_VR_TILE="64x4")), ("direct", dict(PTRACE_VR_VARIANT="direct")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy mirrors (and with them the bit comparison)")
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

    W, H, P, K = args.width, args.height, args.passes, 4
    m = W * H
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    camera = scenes.synthetic_camera(W, H)
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

        def frame_in_hbm():
            hits = DeviceBuffer((abi.hits_bytes(par, abi.HIT_ALL),), np.uint8)
            ds.render_hits_into(flatten.flatten_camera(camera), par, abi.HIT_ALL, hits, stream=st)
            return rb.DeviceGuides.of_hit_buffer(hits, par, abi.HIT_ALL)

        g0, g1 = frame_in_hbm(), frame_in_hbm()
        gathered = DeviceBuffer((rb.gather_bytes(m, 0),), np.uint8)
        gather_work = DeviceBuffer((ds.gather_workspace_bytes(m, K, 1, 3, 1),), np.uint8)

        def gather():
            ds.gather(g1.point, g1.normal, K, 42, None, g1.shape_index, 1, 3, 3, (0.1, 0.2, 0.3), 1, "none", device=True, stream=st, out=gathered,
                      workspace=gather_work, n=m)

        gather()
        f3 = lambda: DeviceBuffer((3, m), np.float64)  # noqa: E731
        f1 = lambda: DeviceBuffer((m,), np.float64)  # noqa: E731
        i1 = lambda: DeviceBuffer((m,), np.int32)  # noqa: E731
        mom, hist_c, hist_m, hist_n, hist_n2 = f3(), f3(), f3(), i1(), i1()
        acc_c, acc_m, acc_n, acc_n2 = f3(), f3(), i1(), i1()
        var, out_c, out_v, filtered = f1(), f3(), f1(), f3()
        zero = ds.temporal_clear(i1(), stream=st)

        def moments():
            ds.variance_moments(gathered, g1.shape_index, W, H, device=True, stream=st, out=mom)

        moments()
        # the history: the same gather accumulated from nothing, as the frame before (lengths of 1 at every hit)
        ds.temporal(gathered, g0.shape_index, g0.normal, g0.point, acc_c, g1.shape_index, g1.normal, g1.point, zero, camera, W, H, device=True, stream=st,
                    out=hist_c, out_count=hist_n)
        ds.temporal(mom, g0.shape_index, g0.normal, g0.point, acc_m, g1.shape_index, g1.normal, g1.point, zero, camera, W, H, device=True, stream=st,
                    out=hist_m, out_count=hist_n2)

        def accumulate(colour, hist, out, out_n):
            ds.temporal(colour, g1.shape_index, g1.normal, g1.point, hist, g0.shape_index, g0.normal, g0.point, hist_n, camera, W, H, device=True,
                        stream=st, out=out, out_count=out_n)

        def estimate(counts=acc_n, moments_of=acc_m, **kw):
            ds.variance_estimate(moments_of, counts, g1.shape_index, g1.normal, g1.point, W, H, device=True, stream=st, out=var, **kw)

        dn_work = DeviceBuffer((ds.denoise_workspace_bytes(W, H, passes=max(P, 2)),), np.uint8)
        vr_work = DeviceBuffer((ds.variance_workspace_bytes(W, H, passes=max(P, 2)),), np.uint8)

        def denoise(colour=acc_c):
            ds.denoise(colour, g1.shape_index, g1.normal, g1.point, W, H, device=True, stream=st, out=filtered, workspace=dn_work, passes=P)

        def variance_filter():
            ds.variance_filter(acc_c, var, g1.shape_index, g1.normal, g1.point, W, H, device=True, stream=st, out=out_c, out_variance=out_v,
                               workspace=vr_work, passes=P)

        def with_env(env, go):
            def run():
                os.environ.update(env)
                try:
                    return timed(go)
                finally:
                    for k in env:
                        del os.environ[k]
            return run

        def frame_old():
            gather()
            accumulate(gathered, hist_c, acc_c, acc_n)
            denoise()

        def frame_new(min_history=2):  # (the lengths here are 2: min_history 2 is the steady state, 4 a sequence's first frames)
            gather()
            moments()
            accumulate(gathered, hist_c, acc_c, acc_n)
            accumulate(mom, hist_m, acc_m, acc_n2)
            estimate(min_history=min_history)
            variance_filter()

        frame_new()
        torch.cuda.synchronize()
        frame = HitFrame(g1.keep.numpy(), par, abi.HIT_ALL)
        shape, normal, point = np.asarray(frame.shape_index)[0], np.asarray(frame.normal)[0], np.asarray(frame.point)[0]
        hit = int((shape >= 0).sum())
        lengths = acc_n.numpy()
        say(f"C2 at {W}x{H}: {m} records ({hit} hits), a {K}-sample gather in HBM, {P} passes; history lengths after the accumulation: "
            f"{int((lengths == 2).sum())} of 2, {int((lengths == 1).sum())} of 1; {args.repeats} alternating rounds of {args.warmup} warm-up + "
            f"{args.steps} timed calls")
        jobs = {"moments": lambda: timed(moments),
                "estimate all short": lambda: timed(lambda: estimate(hist_n, hist_m, min_history=4)),
                "estimate none short": lambda: timed(lambda: estimate(hist_n, hist_m, min_history=1)),
                "gather 4": lambda: timed(gather),
                "accumulate": lambda: timed(lambda: accumulate(gathered, hist_c, acc_c, acc_n)),
                "denoise": lambda: timed(denoise)}
        for name, env in VARIANTS:
            jobs[f"variance filter {name}"] = with_env(env, variance_filter)
        jobs["frame 4+a+f"] = lambda: timed(frame_old)
        jobs["frame 4+2a+e+vf"] = lambda: timed(frame_new)
        jobs["frame 4+2a+e+vf, short"] = lambda: timed(lambda: frame_new(4))
        rounds = {key: [] for key in jobs}
        for _ in range(args.repeats):
            for key, run in jobs.items():
                rounds[key].append(run())
        med = {key: float(np.median(r)) for key, r in rounds.items()}
        spread = {key: 100 * (max(r) - min(r)) / med[key] for key, r in rounds.items()}
        for key in jobs:
            say(f"{key:26s} {med[key] * 1e3:9.1f} us  spread {spread[key]:5.2f}%")
        floor_us = m * (116 + 28) / 8e12 * 1e6
        vf, dn = med["variance filter lds 16x16"], med["denoise"]
        say(f"traffic floor per variance-filter pass: {m} x (84 B + 32 B, and 12 B + 8 B + 8 B for g) = {m * 144 / 1e6:.0f} MB, {floor_us:.1f} us at "
            f"8 TB/s; {P} passes take {vf * 1e3 / (P * floor_us):.1f} x that")
        say(f"variance filter (lds 16x16) / denoise = {vf / dn:.3f}; lds 16x16 / direct = {vf / med['variance filter direct']:.3f}; fastest: "
            f"{min((med['variance filter ' + n], n) for n, _ in VARIANTS)[1]}")
        say(f"estimate all short / none short = {med['estimate all short'] / med['estimate none short']:.2f}")
        say(f"frame (gather 4 + 2 accumulations + moments + estimate + variance filter) / frame (gather 4 + accumulate + denoise) = "
            f"{med['frame 4+2a+e+vf'] / med['frame 4+a+f']:.3f}")
        say(f"the same in a sequence's first frames (every pixel walks the window) = {med['frame 4+2a+e+vf, short'] / med['frame 4+a+f']:.3f}")
        if not args.no_host:
            frame_new(4)
            planes3 = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(H, W, 3)  # noqa: E731
            colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T).reshape(H, W, 3)
            t0 = time.perf_counter()
            same = planes3(mom).tobytes() == rb.luminance_moments_host(colour, shape, W, H).tobytes()
            want_v = rb.variance_estimate_host(planes3(acc_m), acc_n.numpy(), shape, normal, point, W, H)
            same = same and var.numpy().reshape(H, W).tobytes() == want_v.tobytes()
            want = rb.variance_filter_host(planes3(acc_c), want_v, shape, normal, point, W, H, passes=P)
            same = same and planes3(out_c).tobytes() == want[0].tobytes() and out_v.numpy().reshape(H, W).tobytes() == want[1].tobytes()
            host_s = time.perf_counter() - t0
            ok = ok and same
            say(f"the numpy mirrors on the same frame, once, wall time: {host_s:.2f} s; the device's moments, variance and filtered frame "
                f"{'equal' if same else 'DIFFER FROM'} them bit for bit")
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
