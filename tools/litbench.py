#!/usr/bin/env python3
"""Times the shade query (libptrace_lit.so) on one GPU beside the same work without the blend, and beside the host composition it
replaces.

    python tools/litbench.py [--width 1280] [--height 720] [--grid 16] [--samples 64] [--warmup 10] [--steps 100] [--repeats 5] [--no-host]

Workload: C2 (32 spheres + checkered ground plane) at ``width x height``, its hit frame resident in HBM (``render_hits_into``), a
``grid^3`` ``ProbeGrid`` over the bounds of the scene's spheres, coefficients from ONE ``sh_project`` at ``samples`` samples per probe.
Timed ALTERNATING, ``--repeats`` rounds of ``--warmup`` + ``--steps`` launches each between two events on one stream, no host
synchronisation inside the window:

* ``pt_rays_lit_shade_device`` on the frame's planes where they are: slot, pigments, eight corners, 216 gathered coefficients,
  evaluation, ``emitted + brdf_color * E``;
* the yardstick, the parent commit's unchanged libraries on the same records: ``pt_rays_surface_device`` (both colours) plus
  ``pt_rays_sh_eval_device`` (hemisphere) towards the frame's normals with an index plane that names the NEAREST probe of every
  record -- the same work without the blend, an eighth of the coefficient reads (and without the final ``emitted + colour * E``).

In C2's frame every record is a hit, so both sides do their work for every record.  In a frame with misses the two would differ a
little more: the yardstick's surface query still runs for a miss and its evaluation writes zeros for the index -1, where the shade
query reads a miss's shape index and nothing else.

Then, once, in wall time, the host composition the query replaces: ``ProbeGrid.blend`` + ``hemisphere_mean`` + ``materials``.
The shade query's output must equal ``rays.lit_shade_host`` on a sample of the records bit for bit.
Needs torch only to put the batches into device memory and to read the events."""
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
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host composition (it makes a [27, m] block)")
    args = ap.parse_args()
    import torch

    from pytracer_amd import abi, flatten, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer
    from pytracer_amd.hits import HitFrame

    W, H, G, K, BG = args.width, args.height, args.grid, args.samples, (0.1, 0.2, 0.3)
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    cam = flatten.flatten_camera(scenes.synthetic_camera(W, H))
    par = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0)
    # the bounds of the spheres that are part of the scene (the sky sphere around them is not)
    mat = np.asarray(flat.m).reshape(3, 4, -1)
    small = [s for s in range(flat.n_shapes) if flat.kind[s] == abi.SHAPE_SPHERE and abs(mat[0, 0, s]) < 50.0]
    lo = np.min([mat[:, 3, s] - np.abs(mat[:, :3, s]).sum(axis=1) for s in small], axis=0)
    hi = np.max([mat[:, 3, s] + np.abs(mat[:, :3, s]).sum(axis=1) for s in small], axis=0)
    grid = rb.ProbeGrid(lo, (hi - lo) / max(G - 1, 1), (G, G, G))
    n, m = grid.n, W * H
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

        wq = rb.WorldQueries(ds)
        probes = wq.radiance_probes(grid.points(), K, 45, 54, None, None, 1, 3, 3, BG, 1, "none")
        co_dev = torch.from_numpy(np.ascontiguousarray(probes.block)).cuda()
        hits = DeviceBuffer((abi.hits_bytes(par, abi.HIT_ALL),), np.uint8)
        ds.render_hits_into(cam, par, abi.HIT_ALL, hits, stream=st)
        frame = HitFrame(hits.numpy(), par, abi.HIT_ALL)
        base = hits.data_ptr()
        off = lambda channel, first=0: base + abi.hits_plane_offset(par, abi.HIT_ALL, channel, first)  # noqa: E731
        shape_p, point_p, normal_p, uv_p, dir_p = base, off(abi.HIT_POINT), off(abi.HIT_NORMAL), off(abi.HIT_UV), off(abi.HIT_RAY, 3)
        # the yardstick's index plane: the corner with the largest weight; -1 where nothing was hit (zeros)
        pts = np.asarray(frame.point).reshape(-1, 3)
        hit = np.asarray(frame.hit).reshape(-1)
        index, weight = grid.corners(np.where(hit[:, None], pts, grid.origin[None, :]))
        nearest = np.where(hit, index[np.arange(m), weight.argmax(axis=1)], -1).astype(np.int32)
        idx_dev = torch.from_numpy(nearest).cuda()
        lit_out = DeviceBuffer((3, m), np.float64)
        surf_out = DeviceBuffer((rb.surface_bytes(m, rb.SURF_ALL),), np.uint8)
        eval_out = DeviceBuffer((3, m), np.float64)
        ds.slot_table()
        torch.cuda.synchronize()

        def lit():
            ds.lit_shade(grid, co_dev, shape_p, point_p, normal_p, uv_p, dir_p, BG, device=True, stream=st, out=lit_out, n=m)

        def yardstick():
            ds.surface(shape_p, uv_p, "all", device=True, stream=st, out=surf_out, n=m)
            ds.sh_eval(co_dev, normal_p, idx_dev, rb.SH_HEMISPHERE, n=n, device=True, stream=st, out=eval_out, m=m)

        rounds = {"lit_shade": [], "surface+sh_eval": []}
        for _ in range(args.repeats):
            rounds["lit_shade"].append(timed(lit))
            rounds["surface+sh_eval"].append(timed(yardstick))
        print(f"C2 at {W}x{H}: {m} records ({int(hit.sum())} hits), {G}x{G}x{G} probes over [{lo.round(2).tolist()}, {hi.round(2).tolist()}] "
              f"({n * 216 / 2 ** 10:.0f} KiB of coefficients); {args.repeats} alternating rounds of {args.warmup} warm-up + {args.steps} timed launches")
        med = {}
        for name, r in rounds.items():
            med[name] = float(np.median(r))
            print(f"{name:16s} median {med[name] * 1e3:9.1f} us  spread {100 * (max(r) - min(r)) / med[name]:5.2f}%  rounds {' '.join(f'{x * 1e3:.1f}' for x in r)}")
        record_bytes = 4 + 4 + 8 * 11 + 24  # shape index, slot entry, point + normal + uv + dir, the output
        print(f"lit_shade / (surface + sh_eval) = {med['lit_shade'] / med['surface+sh_eval']:.3f} x; {record_bytes} B of record traffic per hit record "
              f"({m * record_bytes / med['lit_shade'] / 1e6:.0f} GB/s if every record were a hit), {8 * 27 * 8} B of gathered coefficients per hit record "
              f"({int(hit.sum()) * 8 * 27 * 8 / med['lit_shade'] / 1e6:.0f} GB/s through the caches)")
        # the same bits as the mirror, on a sample of the records
        got = lit_out.numpy()[:, :m].T
        rows = np.random.default_rng(1).choice(m, size=min(m, 20000), replace=False)
        sub = {k: np.asarray(getattr(frame, k)).reshape(m, -1)[rows] for k in ("point", "normal", "uv", "ray_dir")}
        from types import SimpleNamespace

        mats = wq.materials(SimpleNamespace(shape_index=np.asarray(frame.shape_index).reshape(-1)[rows], uv=sub["uv"]))
        want = rb.lit_shade_host(grid, probes, mats, sub["point"], sub["normal"], sub["ray_dir"], BG)
        same = np.ascontiguousarray(got[rows]).tobytes() == np.ascontiguousarray(want).tobytes()
        ok = ok and same
        print(f"the shade query's output {'equals' if same else 'DIFFERS FROM'} rays.lit_shade_host on {rows.size} of the records bit for bit")
        if not args.no_host:
            probes.evaluator = ds.sh_eval
            t0 = time.perf_counter()
            blended = grid.blend(probes, pts)
            t1 = time.perf_counter()
            mean = blended.hemisphere_mean(np.asarray(frame.normal).reshape(-1, 3))
            t2 = time.perf_counter()
            colours = wq.materials(frame)
            host = np.asarray(colours.emitted).reshape(-1, 3) + np.asarray(colours.brdf_color).reshape(-1, 3) * mean
            t3 = time.perf_counter()
            print(f"the host composition, once, wall time: ProbeGrid.blend {t1 - t0:.2f} s (a [27, {m}] block of {27 * m * 8 / 1e6:.0f} MB), hemisphere_mean "
                  f"{t2 - t1:.2f} s (that block up, {24 * m / 1e6:.0f} MB down), materials + the sum {t3 - t2:.2f} s: {t3 - t0:.2f} s, "
                  f"{(t3 - t0) * 1e3 / med['lit_shade']:.0f} x the shade query")
            diffuse = hit & (np.asarray(colours.brdf_kind).reshape(-1) == abi.BRDF_DIFFUSE)
            print(f"(on the {int(diffuse.sum())} diffuse records the two agree to {np.abs(host[diffuse] - got[diffuse]).max():.3g}: the frame's normals "
                  "are normalised once more in the query)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
