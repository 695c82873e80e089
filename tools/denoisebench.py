#!/usr/bin/env python3
"""Times the denoise query (libptrace_denoise.so) on one GPU: per pass and whole, the LDS variant beside the direct one and beside
its other tiles, beside the gather it follows and beside its numpy mirror.

    python tools/denoisebench.py [--width 1280] [--height 720] [--samples 16] [--passes 4] [--warmup 10] [--steps 100] [--repeats 5]
                                 [--no-host] [--output FILE]

Workload: C2 (32 spheres + checkered ground plane) at ``width x height``, its hit frame resident in HBM (``render_hits_into``), a
``samples``-sample gather of that frame resident in HBM (``gather(device=True)``), then the filter on the gather's radiance planes
guided by the frame's own planes, where they are.  Timed ALTERNATING over the launch alternatives, ``--repeats`` rounds of ``--warmup``
+ ``--steps`` calls each between two events on one stream, no host synchronisation inside the window.

A call with ``p`` passes is the unit-normal pre-pass plus the passes 0 .. p - 1, so the time of the pass with the step ``2^(p-1)`` is
reported as ``T(p) - T(p - 1)`` (and ``T(1)`` holds the pre-pass).  The traffic floor beside each: 76 B read + 24 B written per pixel
and pass.  What binds the kernel is not determined here: that needs counters, collected in a run of their own.

The device's output must equal ``rays.denoise_host`` bit for bit (on the whole frame, unless ``--no-host``); the mirror's wall time
is the host alternative the query replaces.  Needs torch only to read the events."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("lds 16x16", dict(PTRACE_DN_VARIANT="lds", PTRACE_DN_TILE="16x16")), ("lds 32x8", dict(PTRACE_DN_VARIANT="lds", PTRACE_DN_TILE="32x8")),
            ("lds 64x4", dict(PTRACE_DN_VARIANT="lds", PTRACE_DN_TILE="64x4")), ("direct", dict(PTRACE_DN_VARIANT="direct")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--passes", type=int, default=4)
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

    W, H, K, P = args.width, args.height, args.samples, args.passes
    m = W * H
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    cam = flatten.flatten_camera(scenes.synthetic_camera(W, H))
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

        hits = DeviceBuffer((abi.hits_bytes(par, abi.HIT_ALL),), np.uint8)
        ds.render_hits_into(cam, par, abi.HIT_ALL, hits, stream=st)
        frame = HitFrame(hits.numpy(), par, abi.HIT_ALL)
        base = hits.data_ptr()
        off = lambda channel, first=0: base + abi.hits_plane_offset(par, abi.HIT_ALL, channel, first)  # noqa: E731
        shape_p, point_p, normal_p = base, off(abi.HIT_POINT), off(abi.HIT_NORMAL)
        gathered = DeviceBuffer((rb.gather_bytes(m, 0),), np.uint8)
        gather_work = DeviceBuffer((ds.gather_workspace_bytes(m, K, 1, 3, 1),), np.uint8)

        def gather():
            ds.gather(point_p, normal_p, K, 42, None, shape_p, 1, 3, 3, (0.1, 0.2, 0.3), 1, "none", device=True, stream=st, out=gathered,
                      workspace=gather_work, n=m)

        gather()
        colour_p = gathered.data_ptr()  # (the three radiance planes come first)
        out = DeviceBuffer((3, m), np.float64)
        work = DeviceBuffer((ds.denoise_workspace_bytes(W, H, passes=max(P, 2)),), np.uint8)
        torch.cuda.synchronize()
        hit = int((np.asarray(frame.shape_index) >= 0).sum())
        say(f"C2 at {W}x{H}: {m} records ({hit} hits), a {K}-sample gather in HBM, {P} passes; {args.repeats} alternating rounds of "
            f"{args.warmup} warm-up + {args.steps} timed calls")

        def filter_with(env, passes):
            def go():
                ds.denoise(colour_p, shape_p, normal_p, point_p, W, H, device=True, stream=st, out=out, workspace=work, passes=passes)

            def run():
                os.environ.update(env)
                try:
                    return timed(go)
                finally:
                    for k in env:
                        del os.environ[k]
            return run

        jobs = {(name, p): filter_with(env, p) for name, env in VARIANTS for p in range(1, P + 1)}
        jobs[("gather", K)] = lambda: timed(gather)
        rounds = {key: [] for key in jobs}
        for _ in range(args.repeats):
            for key, run in jobs.items():
                rounds[key].append(run())
        med = {key: float(np.median(r)) for key, r in rounds.items()}
        spread = {key: 100 * (max(r) - min(r)) / med[key] for key, r in rounds.items()}
        floor_us = m * 100 / 8e12 * 1e6
        say(f"traffic floor per pass: {m} x (76 B read + 24 B written) = {m * 100 / 1e6:.0f} MB, {floor_us:.1f} us at 8 TB/s")
        for name, _ in VARIANTS:
            say(f"{name:10s} whole ({P} passes + pre-pass) {med[(name, P)] * 1e3:8.1f} us  spread {spread[(name, P)]:5.2f}%")
            prev = 0.0
            for p in range(1, P + 1):
                t = med[(name, p)]
                say(f"    step {2 ** (p - 1):3d}: T({p}) - T({p - 1}) = {(t - prev) * 1e3:8.1f} us ({(t - prev) * 1e3 / floor_us:5.1f} x the floor)"
                    + ("   (with the pre-pass: 48 B per record more)" if p == 1 else ""))
                prev = t
        best = min((med[(name, P)], name) for name, _ in VARIANTS)
        say(f"fastest whole: {best[1]}; lds 16x16 / direct = {med[('lds 16x16', P)] / med[('direct', P)]:.3f}")
        g = med[("gather", K)]
        say(f"the {K}-sample gather it follows: {g:.3f} ms (spread {spread[('gather', K)]:.2f}%); the default filter (lds 16x16) costs {med[('lds 16x16', P)] / g:.3f} of it")
        if not args.no_host:
            ds.denoise(colour_p, shape_p, normal_p, point_p, W, H, device=True, stream=st, out=out, workspace=work, passes=P)
            got = np.ascontiguousarray(out.numpy()[:, :m].T).reshape(H, W, 3)
            noisy = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T)
            t0 = time.perf_counter()
            want = rb.denoise_host(noisy, np.asarray(frame.shape_index)[0], np.asarray(frame.normal)[0], np.asarray(frame.point)[0], W, H, passes=P)
            host_s = time.perf_counter() - t0
            same = got.tobytes() == want.tobytes()
            ok = ok and same
            say(f"the numpy mirror on the same frame, once, wall time: {host_s:.2f} s, {host_s * 1e3 / med[('lds 16x16', P)]:.0f} x the query; the device's frame "
                f"{'equals' if same else 'DIFFERS FROM'} it bit for bit")
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
