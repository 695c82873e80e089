#!/usr/bin/env python3
"""Times the weighted accumulate query (libptrace_weighted.so) on one GPU beside the three launches it replaces (measured in the same
run), the frame it shortens, and measures what weighting frames by their samples buys an adaptive sequence.

    python tools/weightedbench.py [--width 1280] [--height 720] [--passes 4] [--warmup 10] [--steps 100] [--repeats 5] [--no-quality]
                                  [--output FILE]

Workload: tools/variancebench.py's.  C2 (32 spheres + checkered ground plane) at ``width x height``; two hit frames of the same camera
resident in HBM, a 4-sample gather of the frame, and one accumulation from an empty history as the frame before (every hit has the
length 1 and, on the weighted path, the weight 4).  Timed ALTERNATING over the jobs, ``--repeats`` rounds of ``--warmup`` + ``--steps``
calls each between two events on one stream, no host synchronisation inside the window:

    moments               one pt_rays_variance_moments_device call
    accumulate            one pt_rays_temporal_accumulate_device call (the colour's; the moments' is the same launch on other planes)
    moments + 2 acc       the three launches the weighted query replaces
    weighted              one pt_rays_weighted_accumulate_device call, samples = a plane of 4
    weighted, no plane    the same with samples = NULL
    frame 4+2a+e+vf       gather 4, moments, two accumulations, estimate, variance filter: a VarianceGuidedGatherShader frame's device work
    frame 4+w+e+vf        gather 4, weighted, estimate, variance filter: the same frame on the weighted query

Before anything is timed contract A of include/ptrace_weighted.h is checked on the whole frame: unweighted, the weighted query's
colour, moments and lengths are the three launches' bit for bit.

The taps' traffic: per hit pixel up to 4 x (8 B of shape and count + 96 B of normal, point, colour and moments) read, 52 B written,
plus the pixel's own 80 B; neighbouring lanes share their taps' lines.  What binds the kernel is not determined here: that needs
counters, collected in a run of their own.

The quality experiment (``--no-quality`` skips it) is tools/adaptivebench.py's protocol, unchanged: the demo world at 48x36, eight
frames, 1 degree per frame, ``min_samples`` 1, ``max_samples`` 32, ``gain_for_budget`` at the uniform sequence's rays; RMS error of the
accumulated E against a 1024-sample gather on the whole frame and within two radii of the sphere's foot -- uniform 4,
``VarianceAccumulator`` under adaptive counts (the parent's path), and ``WeightedAccumulator`` in both weight modes, with
``min_samples`` 1 and 0, each with and without the filter.  Needs torch only to read the events."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def quality(say):
    from pytracer_amd import hostmodel as hm, rays as rb, scenes
    from pytracer_amd.tracer import GpuImageTracer

    W, H, K, N, step = 48, 36, 4, 8, 1.0
    world, camera = scenes.demo_world()
    tracer = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=0)
    try:
        wq = tracer.world_queries(world)
        black = hm.Color(0.0, 0.0, 0.0)
        frames = []
        for f in range(N):
            tracer.camera = scenes.turned_camera(camera, step * f)
            frames.append((tracer.fire_all_hits(world), tracer.camera))
        last = frames[-1][0]
        shape, point = np.asarray(last.shape_index)[0], np.asarray(last.point)[0]
        hit, shadow = shape >= 0, (shape == 1) & (np.hypot(point[..., 0], point[..., 1]) <= 2.0)
        reference = np.asarray(wq.hemisphere_radiance(last, 1024, 42, None, 1, 10, 3, black, 1, "none", init_seq=10 ** 9).radiance)[0]
        rms = lambda a, where: float(np.sqrt(np.mean((a[where] - reference[where]) ** 2)))  # noqa: E731

        def sequence(make, counts_of):
            """``make()`` -> the accumulator; ``counts_of(frame, e, variance)`` -> counts [H, W] or None (uniform K)"""
            acc, seq, totals, e, variance = make(), 54, [], None, None
            weighted = isinstance(acc, rb.WeightedAccumulator)
            for f, (frame, cam) in enumerate(frames):
                counts = counts_of(frame, e, variance) if f else None
                index = np.asarray(frame.shape_index)[0]
                if counts is None:
                    g = wq.hemisphere_radiance(frame, K, 42, None, 1, 10, 3, black, 1, "none", init_seq=seq)
                    seq += W * H * K
                    taken = np.where(index >= 0, K, 0).astype(np.int32)
                else:
                    g = wq.hemisphere_radiance_ragged(frame, counts[None], None, 42, None, 1, 10, 3, black, 1, "taken", init_seq=seq)
                    seq += int(np.maximum(counts, 0).sum())
                    taken = np.asarray(g.taken, dtype=np.int32).reshape(H, W)
                totals.append(int(taken.sum()))
                e, variance = acc.update(np.asarray(g.radiance)[0], frame, cam, samples=taken) if weighted else acc.update(np.asarray(g.radiance)[0], frame, cam)
            return e, variance, totals

        def row(label, e, variance, totals):
            filtered, _ = wq.variance_filtered(e, last, variance=variance)
            say(f"    {label:58s} {rms(e, hit):.5f} / {rms(e, shadow):.5f}   filtered {rms(filtered, hit):.5f} / {rms(filtered, shadow):.5f}   rays per frame "
                f"{' '.join(map(str, totals))}")
            return rms(e, hit)

        say(f"QUALITY: demo world {W}x{H}, {N} frames, {step:g} degree(s) per frame, {int(hit.sum())} hit pixels at the last camera ({int(shadow.sum())} in the "
            f"shadow region); RMS error of the accumulated E against a 1024-sample gather, whole frame / shadow region")
        uniform = lambda frame, e, variance: None  # noqa: E731
        base = row(f"uniform {K} per pixel, VarianceAccumulator", *sequence(lambda: rb.VarianceAccumulator(wq), uniform))
        row(f"uniform {K} per pixel, WeightedAccumulator", *sequence(lambda: rb.WeightedAccumulator(wq), uniform))
        results = {}
        for floor in (0.05, 0.2, 1.0):
            for least in (1, 0):
                par = dict(min_samples=least, max_samples=32, tolerance=0.05, luminance_floor=floor)

                def counts_of(frame, e, variance, par=par):
                    index = np.asarray(frame.shape_index)[0]
                    budget = K * int((index >= 0).sum())
                    gain = rb.gain_for_budget(variance, e, index, budget, **par)
                    return wq.sample_counts(e, frame, variance, gain=gain, **par)

                if least == 1:
                    results[("parent", floor, least)] = row(f"adaptive floor {floor:g} min {least}, VarianceAccumulator (the parent)",
                                                            *sequence(lambda: rb.VarianceAccumulator(wq), counts_of))
                for blend in (False, True):
                    for cap in (128.0, float("inf")):
                        results[("blend" if blend else "max", floor, least, cap)] = row(
                            f"adaptive floor {floor:g} min {least}, weighted {'blend' if blend else 'max'} max_weight {cap:g}",
                            *sequence(lambda: rb.WeightedAccumulator(wq, blend_weight=blend, max_weight=cap), counts_of))
        parent = min(v for k, v in results.items() if k[0] == "parent")
        for mode in ("max", "blend"):
            best = min((v, k) for k, v in results.items() if k[0] == mode)
            say(f"    best weighted ({mode}): {best[0]:.5f} at floor {best[1][1]:g}, min_samples {best[1][2]}, max_weight {best[1][3]:g}: / parent's best "
                f"{parent:.5f} = {best[0] / parent:.3f}; / uniform {base:.5f} = {best[0] / base:.3f}")
    finally:
        tracer.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true", help="skip the quality experiment")
    ap.add_argument("--output", type=str, default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch

    from pytracer_amd import abi, flatten, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer

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
        whist_c, whist_m, whist_n, wacc_c, wacc_m, wacc_n = f3(), f3(), i1(), f3(), f3(), i1()
        var, out_c, out_v = f1(), f3(), f1()
        zero = ds.temporal_clear(i1(), stream=st)
        fours = torch.full((m,), K, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def moments():
            ds.variance_moments(gathered, g1.shape_index, W, H, device=True, stream=st, out=mom)

        moments()
        # the history: the same gather accumulated from nothing, as the frame before (lengths of 1 at every hit)
        ds.temporal(gathered, g0.shape_index, g0.normal, g0.point, acc_c, g1.shape_index, g1.normal, g1.point, zero, camera, W, H, device=True, stream=st,
                    out=hist_c, out_count=hist_n)
        ds.temporal(mom, g0.shape_index, g0.normal, g0.point, acc_m, g1.shape_index, g1.normal, g1.point, zero, camera, W, H, device=True, stream=st,
                    out=hist_m, out_count=hist_n2)

        def weighted(samples, hist=(None, None, None), out=(wacc_c, wacc_m, wacc_n), **kw):
            hc, hm_, hn = hist if hist[0] is not None else (whist_c, whist_m, whist_n)
            ds.weighted(gathered, samples, g1.shape_index, g1.normal, g1.point, hc, hm_, g0.shape_index, g0.normal, g0.point, hn, camera, W, H,
                        device=True, stream=st, out=out[0], out_moments=out[1], out_count=out[2], **kw)

        ds.weighted(gathered, fours, g0.shape_index, g0.normal, g0.point, wacc_c, wacc_m, g1.shape_index, g1.normal, g1.point, zero, camera, W, H,
                    device=True, stream=st, out=whist_c, out_moments=whist_m, out_count=whist_n)

        def accumulate(colour, hist, out, out_n):
            ds.temporal(colour, g1.shape_index, g1.normal, g1.point, hist, g0.shape_index, g0.normal, g0.point, hist_n, camera, W, H, device=True,
                        stream=st, out=out, out_count=out_n)

        def three():
            moments()
            accumulate(gathered, hist_c, acc_c, acc_n)
            accumulate(mom, hist_m, acc_m, acc_n2)

        vr_work = DeviceBuffer((ds.variance_workspace_bytes(W, H, passes=max(P, 2)),), np.uint8)

        def rest(colour, moments_of, counts):
            ds.variance_estimate(moments_of, counts, g1.shape_index, g1.normal, g1.point, W, H, device=True, stream=st, out=var, min_history=2)
            ds.variance_filter(colour, var, g1.shape_index, g1.normal, g1.point, W, H, device=True, stream=st, out=out_c, out_variance=out_v,
                               workspace=vr_work, passes=P)

        def frame_old():
            gather()
            three()
            rest(acc_c, acc_m, acc_n)

        def frame_new():
            gather()
            weighted(fours)
            rest(wacc_c, wacc_m, wacc_n)

        # contract A on the whole frame: the history of the old path, whose moments' third plane is 0 where the contract wants the length --
        # so compare on a history made for it: S = 1.0 at every hit (the lengths are 1)
        three()
        contract_m = f3()
        ds.weighted(gathered, None, g0.shape_index, g0.normal, g0.point, wacc_c, wacc_m, g1.shape_index, g1.normal, g1.point, zero, camera, W, H,
                    device=True, stream=st, out=out_c, out_moments=contract_m, out_count=wacc_n, max_weight=31.0)
        torch.cuda.synchronize()
        same_start = out_c.numpy().tobytes() == hist_c.numpy().tobytes() and contract_m.numpy()[:2].tobytes() == hist_m.numpy()[:2].tobytes()
        a_c, a_m, a_n = f3(), f3(), i1()
        weighted(None, hist=(hist_c, contract_m, hist_n), out=(a_c, a_m, a_n), max_weight=31.0)
        torch.cuda.synchronize()
        same = (same_start and a_c.numpy().tobytes() == acc_c.numpy().tobytes() and a_m.numpy()[:2].tobytes() == acc_m.numpy()[:2].tobytes()
                and a_n.numpy().tobytes() == acc_n.numpy().tobytes() and np.array_equal(a_m.numpy()[2], a_n.numpy().astype(np.float64)))
        ok = ok and same
        lengths = acc_n.numpy()
        say(f"C2 at {W}x{H}: {m} records ({int((lengths >= 1).sum())} hits), a {K}-sample gather in HBM, {P} filter passes; history lengths after the "
            f"accumulation: {int((lengths == 2).sum())} of 2, {int((lengths == 1).sum())} of 1; {args.repeats} alternating rounds of {args.warmup} warm-up + "
            f"{args.steps} timed calls; contract A (unweighted, the weighted query against moments + 2 accumulations, whole frame): "
            f"{'bit for bit' if same else 'DIFFERS'}")
        jobs = {"moments": lambda: timed(moments),
                "accumulate": lambda: timed(lambda: accumulate(gathered, hist_c, acc_c, acc_n)),
                "moments + 2 acc": lambda: timed(three),
                "weighted": lambda: timed(lambda: weighted(fours)),
                "weighted, no plane": lambda: timed(lambda: weighted(None)),
                "gather 4": lambda: timed(gather),
                "frame 4+2a+e+vf": lambda: timed(frame_old),
                "frame 4+w+e+vf": lambda: timed(frame_new)}
        rounds = {key: [] for key in jobs}
        for _ in range(args.repeats):
            for key, run in jobs.items():
                rounds[key].append(run())
        med = {key: float(np.median(r)) for key, r in rounds.items()}
        spread = {key: 100 * (max(r) - min(r)) / med[key] for key, r in rounds.items()}
        for key in jobs:
            say(f"{key:22s} {med[key] * 1e3:9.1f} us  spread {spread[key]:5.2f}%")
        say(f"weighted / (moments + 2 accumulations) = {med['weighted'] / med['moments + 2 acc']:.3f} "
            f"({med['weighted'] * 1e3:.1f} us against {med['moments + 2 acc'] * 1e3:.1f} us; the parts alone: {med['moments'] * 1e3:.1f} + 2 x "
            f"{med['accumulate'] * 1e3:.1f} us)")
        say(f"frame (gather 4 + weighted + estimate + variance filter) / frame (gather 4 + moments + 2 accumulations + estimate + variance filter) = "
            f"{med['frame 4+w+e+vf'] / med['frame 4+2a+e+vf']:.3f} ({med['frame 4+w+e+vf']:.3f} ms against {med['frame 4+2a+e+vf']:.3f} ms)")
        hits_n = int((lengths >= 1).sum())
        say(f"the taps' traffic at most: {hits_n} hits x (4 x 104 B read + 80 B own) + {m} x 52 B written = {(hits_n * 496 + m * 52) / 1e6:.0f} MB "
            f"before any line is shared between lanes; {(hits_n * 496 + m * 52) / 8e12 * 1e6:.1f} us at 8 TB/s")
    if not args.no_quality:
        quality(say)
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
