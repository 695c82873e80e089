#!/usr/bin/env python3
"""Times the adaptive queries (libptrace_adaptive.so) on one GPU and measures what adaptive sampling buys: the ragged gather beside
the uniform gather it generalises (measured in the same run), its launches apart, the counts and the offsets query alone, a skewed
count plane beside a flat one of the same total, and the quality experiment.

    python tools/adaptivebench.py [--width 1280] [--height 720] [--warmup 5] [--steps 30] [--repeats 5] [--no-quality] [--output FILE]

Workload: C2 (32 spheres + checkered ground plane) at ``width x height``; one hit frame resident in HBM (``render_hits_into``); gathers
at ``max_depth`` 3 from the frame's first hits (``Ray.depth`` 1), one ray per node.  Timed ALTERNATING over the jobs, ``--repeats`` rounds of
``--warmup`` + ``--steps`` calls each between two events on one stream, no host synchronisation inside the window:

    uniform 16 / uniform 4     one uniform gather call (libptrace_gather.so, the parent's), samples = 16 / 4
    ragged 16 / ragged 4       the offsets query and one ragged gather call, every count 16 / 4 (both gathers skip the records
                               without a hit by their shape index; offsets[i] = 16 i, so both draw the same streams)
    ragged 16 walk / mean      the ragged gather's launches apart (PTRACE_ADAPTIVE_PART; `walk` includes the owner variant's expand launch)
    ... search / ... owner     the same with the record look-up named (PTRACE_ADAPTIVE_LOOKUP); without a name: the library's default
    offsets                    the offsets query alone (three launches)
    counts                     the counts query alone (one launch)
    ragged skewed              the total of 4 per record: 90 % of the records at 1, every tenth sharing the rest (31 each)

The quality experiment (``--no-quality`` skips it): the demo world at 48x36, eight frames, the camera turning 1 degree per frame, RMS
error of the accumulated E at the last camera against a 1024-sample gather there, over the hit pixels and over the ground plane within
two radii of the sphere's foot -- ``VarianceGuidedGatherShader`` 's sequence at 4 samples per pixel against ``AdaptiveGatherShader`` 's
with ``gain_for_budget`` set to the same total per frame, ``min_samples`` 1, ``max_samples`` 32, over a small sweep of ``tolerance`` and
``luminance_floor``.  Needs torch only to read the events."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BG = (0.1, 0.2, 0.3)


def quality(say):
    """-> the sweep's rows.  Both sequences filter nothing: E is the accumulated estimate, as in profiles/variance_kernel.txt's (c)."""
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

        def sequence(counts_of):
            """``counts_of(frame, e, variance)`` -> counts [H, W] or None (uniform K) -> (E, variance, totals per frame)"""
            acc, seq, totals, e, variance = rb.VarianceAccumulator(wq), 54, [], None, None
            for f, (frame, cam) in enumerate(frames):
                counts = counts_of(frame, e, variance) if f else None
                if counts is None:
                    g = wq.hemisphere_radiance(frame, K, 42, None, 1, 10, 3, black, 1, "none", init_seq=seq)
                    seq += W * H * K
                    totals.append(K * int((np.asarray(frame.shape_index) >= 0).sum()))
                else:
                    g = wq.hemisphere_radiance_ragged(frame, counts[None], None, 42, None, 1, 10, 3, black, 1, "taken", init_seq=seq)
                    seq += int(np.maximum(counts, 0).sum())
                    totals.append(int(np.asarray(g.taken).sum()))
                e, variance = acc.update(np.asarray(g.radiance)[0], frame, cam)
            return e, variance, totals

        e_u, v_u, totals_u = sequence(lambda frame, e, variance: None)
        say(f"QUALITY: demo world {W}x{H}, {N} frames, {step:g} degree(s) per frame, {int(hit.sum())} hit pixels at the last camera ({int(shadow.sum())} in the "
            f"shadow region); RMS error of the accumulated E against a 1024-sample gather, whole frame / shadow region")
        say(f"    uniform {K} per pixel                          {rms(e_u, hit):.5f} / {rms(e_u, shadow):.5f}   rays per frame {' '.join(map(str, totals_u))}")
        guided, _ = wq.variance_filtered(e_u, last, variance=v_u)
        say(f"    uniform {K} per pixel, variance-guided filter   {rms(guided, hit):.5f} / {rms(guided, shadow):.5f}")
        rows = []
        # (under a budget the tolerance cancels against the gain that is fitted to the budget: two values show it; the floor does not)
        for tolerance in (0.05, 0.1):
            for floor in (0.01, 0.05, 0.2, 0.5, 1.0):
                par = dict(min_samples=1, max_samples=32, tolerance=tolerance, luminance_floor=floor)

                def counts_of(frame, e, variance, par=par):
                    index = np.asarray(frame.shape_index)[0]
                    budget = K * int((index >= 0).sum())
                    gain = rb.gain_for_budget(variance, e, index, budget, **par)
                    return wq.sample_counts(e, frame, variance, gain=gain, **par)

                e_a, v_a, totals_a = sequence(counts_of)
                filtered, _ = wq.variance_filtered(e_a, last, variance=v_a)
                rows.append((tolerance, floor, rms(e_a, hit), rms(e_a, shadow), rms(filtered, hit), rms(filtered, shadow), totals_a))
                say(f"    adaptive tolerance {tolerance:<5g} luminance_floor {floor:<5g}   {rows[-1][2]:.5f} / {rows[-1][3]:.5f}   filtered "
                    f"{rows[-1][4]:.5f} / {rows[-1][5]:.5f}   rays per frame {' '.join(map(str, totals_a))}")
        best = min(rows, key=lambda r: r[2])
        say(f"    best of the sweep on the whole frame: tolerance {best[0]:g}, luminance_floor {best[1]:g}: adaptive / uniform = "
            f"{best[2] / rms(e_u, hit):.3f} whole frame, {best[3] / rms(e_u, shadow):.3f} shadow region (the accumulation weights frames equally whatever they cost)")
        # without a budget, gain 1: what a tolerance spends on this scene (the default is the one nearest the uniform sequence's cost)
        for tolerance in (0.02, 0.05, 0.1, 0.2):
            par = dict(min_samples=1, max_samples=32, tolerance=tolerance, luminance_floor=best[1])
            e_a, v_a, totals_a = sequence(lambda frame, e, variance, par=par: wq.sample_counts(e, frame, variance, **par))
            say(f"    gain 1, tolerance {tolerance:<5g} luminance_floor {best[1]:<5g}        {rms(e_a, hit):.5f} / {rms(e_a, shadow):.5f}   rays per frame "
                f"{' '.join(map(str, totals_a))}")
        return rows
    finally:
        tracer.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true", help="skip the quality experiment")
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

        hits = DeviceBuffer((abi.hits_bytes(par, abi.HIT_ALL),), np.uint8)
        ds.render_hits_into(flatten.flatten_camera(camera), par, abi.HIT_ALL, hits, stream=st)
        g = rb.DeviceGuides.of_hit_buffer(hits, par, abi.HIT_ALL)
        torch.cuda.synchronize()
        shape = np.asarray(HitFrame(hits.numpy(), par, abi.HIT_ALL).shape_index)[0].reshape(-1)
        hit = shape >= 0
        n_hit = int(hit.sum())
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

        def plane(value):
            return np.full(m, value, dtype=np.int32)

        skew = plane(1)
        heavy = np.arange(9, m, 10)  # every tenth record
        rest = 4 * m - (m - heavy.size)
        skew[heavy] = rest // heavy.size
        skew[heavy[: rest % heavy.size]] += 1
        assert int(skew.sum()) == 4 * m
        planes = {"16": to_dev(plane(16)), "4": to_dev(plane(4)), "skewed": to_dev(skew)}
        totals = {"16": 16 * m, "4": 4 * m, "skewed": 4 * m}
        torch.cuda.synchronize()
        offsets = DeviceBuffer((m + 1,), np.int64)
        off_work = DeviceBuffer((8 * ((m + 255) // 256),), np.uint8)
        out_u = DeviceBuffer((rb.gather_bytes(m, 0),), np.uint8)
        out_r = DeviceBuffer((rb.adaptive_bytes(m, 0),), np.uint8)
        work_u = {K: DeviceBuffer((ds.gather_workspace_bytes(m, K, 1, 3, 1),), np.uint8) for K in (16, 4)}
        os.environ["PTRACE_ADAPTIVE_LOOKUP"] = "owner"  # (the larger of the two workspaces: it holds the owner plane too)
        work_r = DeviceBuffer((ds.adaptive_workspace_bytes(m, totals["16"], 1, 3, 1),), np.uint8)
        del os.environ["PTRACE_ADAPTIVE_LOOKUP"]

        def uniform(K):
            ds.gather(g.point, g.normal, K, 42, None, g.shape_index, 1, 3, 3, BG, 1, "none", device=True, stream=st, out=out_u, workspace=work_u[K], n=m)

        def scan(name):
            ds.sample_offsets(planes[name], device=True, stream=st, out=offsets, workspace=off_work, n=m)

        def ragged(name, with_scan=True):
            if with_scan:
                scan(name)
            ds.gather_ragged(g.point, g.normal, planes[name], offsets, totals[name], 42, None, g.shape_index, 1, 3, 3, BG, 1, "none", device=True,
                             stream=st, out=out_r, workspace=work_r, n=m)

        def with_env(env, go):
            def run():
                os.environ.update(env)
                try:
                    return timed(go)
                finally:
                    for k in env:
                        del os.environ[k]
            return run

        def part(which, lookup):
            return with_env(dict(PTRACE_ADAPTIVE_PART=which, PTRACE_ADAPTIVE_LOOKUP=lookup), lambda: ragged("16", with_scan=False))

        variance, colour, counts_out = DeviceBuffer((m,), np.float64), DeviceBuffer((3, m), np.float64), DeviceBuffer((m,), np.int32)
        ds.variance_moments(out_u, g.shape_index, W, H, device=True, stream=st, out=colour)  # (any finite planes: the launch is what is timed)

        def counts():
            ds.sample_counts(colour, colour, g.shape_index, device=True, stream=st, out=counts_out, m=m)

        # the ragged gather with every count 16 is the uniform gather at 16 on the frame's own streams: checked before anything is timed
        uniform(16)
        same = True
        for lookup in ("search", "owner"):
            os.environ["PTRACE_ADAPTIVE_LOOKUP"] = lookup
            ragged("16")
            torch.cuda.synchronize()
            del os.environ["PTRACE_ADAPTIVE_LOOKUP"]
            same = same and out_u.numpy()[: 24 * m].tobytes() == out_r.numpy()[: 24 * m].tobytes()
        ok = ok and same
        say(f"C2 at {W}x{H}: {m} records ({n_hit} hits), max_depth 3 from depth 1; {args.repeats} alternating rounds of {args.warmup} warm-up + "
            f"{args.steps} timed calls; the radiance of ragged 16 {'equals' if same else 'DIFFERS FROM'} uniform 16's bit for bit on the whole frame, for both look-ups")
        search, owner = dict(PTRACE_ADAPTIVE_LOOKUP="search"), dict(PTRACE_ADAPTIVE_LOOKUP="owner")
        jobs = {"uniform 16": lambda: timed(lambda: uniform(16)),
                "ragged 16": lambda: timed(lambda: ragged("16")),
                "ragged 16 search": with_env(search, lambda: ragged("16")),
                "ragged 16 search walk": part("walk", "search"),
                "ragged 16 owner": with_env(owner, lambda: ragged("16")),
                "ragged 16 owner walk": part("walk", "owner"),
                "ragged 16 mean": part("mean", "search"),
                "offsets": lambda: timed(lambda: scan("16")),
                "counts": lambda: timed(counts),
                "uniform 4": lambda: timed(lambda: uniform(4)),
                "ragged 4": lambda: timed(lambda: ragged("4")),
                "ragged 4 search": with_env(search, lambda: ragged("4")),
                "ragged 4 owner": with_env(owner, lambda: ragged("4")),
                "ragged skewed": lambda: timed(lambda: ragged("skewed")),
                "ragged skewed search": with_env(search, lambda: ragged("skewed")),
                "ragged skewed owner": with_env(owner, lambda: ragged("skewed"))}
        rounds = {key: [] for key in jobs}
        for _ in range(args.repeats):
            for key, run in jobs.items():
                rounds[key].append(run())
        med = {key: float(np.median(r)) for key, r in rounds.items()}
        spread = {key: 100 * (max(r) - min(r)) / med[key] for key, r in rounds.items()}
        for key in jobs:
            say(f"{key:22s} {med[key] * 1e3:10.1f} us  spread {spread[key]:5.2f}%")
        say(f"ragged 16 (the default look-up, offsets included) / uniform 16 = {med['ragged 16'] / med['uniform 16']:.3f}; search: "
            f"{med['ragged 16 search'] / med['uniform 16']:.3f}, owner plane: {med['ragged 16 owner'] / med['uniform 16']:.3f}")
        say(f"of the ragged 16's time: the walk {med['ragged 16 search walk'] * 1e3:.1f} us with the search in it, {med['ragged 16 owner walk'] * 1e3:.1f} us "
            f"behind the expand launch (included); the mean {med['ragged 16 mean'] * 1e3:.1f} us; the scan {med['offsets'] * 1e3:.1f} us")
        say(f"ragged 4 / uniform 4 = {med['ragged 4'] / med['uniform 4']:.3f}; skewed (90 % at 1, every tenth hit at {int(skew.max())}) / ragged 4 = "
            f"{med['ragged skewed'] / med['ragged 4']:.3f}; skewed / uniform 4 = {med['ragged skewed'] / med['uniform 4']:.3f}: the same rays, what divergence "
            f"within a wave and rows of unequal length cost")
    if not args.no_quality:
        quality(say)
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
