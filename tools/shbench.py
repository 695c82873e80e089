#!/usr/bin/env python3
"""Times the probe query (libptrace_sh.so) on one GPU beside what a caller would run without it.

    python tools/shbench.py [--grid 16] [--samples 1024] [--warmup 10] [--steps 100] [--repeats 5] [--eval 1000000]

Workload: C2 (32 spheres + checkered ground plane) at max_depth 3, num_of_rays 1, a ``grid^3`` ``ProbeGrid`` over the bounds of
the scene's spheres at ``samples`` samples per probe.  Timed ALTERNATING, ``--repeats`` rounds of ``--warmup`` + ``--steps`` launches
each on a stream of its own between two events, no host synchronisation inside the window:

* ``pt_rays_sh_project_device``: the walk and the projection (two kernels; ``rocprofv3 --kernel-trace --stats`` on this script
  splits them);
* ``pt_rays_radiance_device`` on the SAME ``n K`` rays and generators, prepared in HBM beforehand (the directions by
  ``pt_rays_sh_directions_device``, the generators two draws in): what a caller runs today, before the host's projection and the
  two transfers.  Its output, projected on the host in sample order, must equal the probe query's bit for bit.

Then ``pt_rays_sh_eval_device`` for ``--eval`` records, and the transfer volumes of the host-side alternative.
Needs torch only to put the batches into device memory and to read the events."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--eval", type=int, default=1000000)
    args = ap.parse_args()
    import torch

    from pytracer_amd import abi, flatten, rays as rb, scenes
    from pytracer_amd.device import DeviceScene
    from pytracer_amd.devmem import DeviceBuffer

    N, D, LIMIT, DEPTH, BG, S0, Q0 = 1, 3, 3, 1, (0.1, 0.2, 0.3), 45, 54
    K, G = args.samples, args.grid
    flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    # the bounds of the spheres that are part of the scene (the sky sphere around them is not)
    m = np.asarray(flat.m).reshape(3, 4, -1)
    small = [s for s in range(flat.n_shapes) if flat.kind[s] == abi.SHAPE_SPHERE and abs(m[0, 0, s]) < 50.0]
    lo = np.min([m[:, 3, s] - np.abs(m[:, :3, s]).sum(axis=1) for s in small], axis=0)
    hi = np.max([m[:, 3, s] + np.abs(m[:, :3, s]).sum(axis=1) for s in small], axis=0)
    grid = rb.ProbeGrid(lo, (hi - lo) / max(G - 1, 1), (G, G, G))
    pts = grid.points()
    n, total = grid.n, grid.n * K
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

        pts_dev = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
        ws = DeviceBuffer((ds.sh_workspace_bytes(n, K, N, D, DEPTH),), np.uint8)
        out = DeviceBuffer((rb.sh_bytes(n, rb.SH_ALL),), np.uint8)
        # today's route, its host work left out: the n K rays and generators prepared in HBM (not timed)
        dirs_dev = ds.sh_directions(n, K, S0, Q0, None, device=True, stream=st)
        stream.synchronize()
        d = torch.from_numpy(dirs_dev.numpy()).cuda()  # [3, n K]
        rays_dev = torch.empty((8, total), dtype=torch.float64, device="cuda")
        rays_dev[0:3] = pts_dev.repeat_interleave(K, dim=1)
        rays_dev[3:6] = d
        rays_dev[6] = 1.0e-5
        rays_dev[7] = math.inf
        gen_dev = torch.from_numpy(rb.pcg_streams(S0, Q0 + np.arange(total, dtype=np.uint64), skip=2).view(np.int64)).cuda()
        rws = DeviceBuffer((ds.radiance_workspace_bytes(total, N, D, DEPTH),), np.uint8)
        rout = DeviceBuffer((rb.radiance_bytes(total, rb.RAD_COUNT),), np.uint8)
        torch.cuda.synchronize()
        probe = lambda: ds.sh_project(pts_dev, K, S0, Q0, None, None, N, D, LIMIT, BG, DEPTH, "all", device=True, stream=st, out=out,  # noqa: E731
                                      workspace=ws)
        route = lambda: ds.radiance(rays_dev, gen_dev, N, D, LIMIT, BG, DEPTH, "count", device=True, stream=st, out=rout, workspace=rws,  # noqa: E731
                                    n=total)
        rounds = {"probes": [], "path_radiance": []}
        for _ in range(args.repeats):
            rounds["probes"].append(timed(probe))
            rounds["path_radiance"].append(timed(route))
        res = rb.ProbeSet(out.numpy(), n, "all")
        rad = rb.RayRadiance(rout.numpy(), total, "count")
        traced = int(res.n_rays.sum())
        print(f"C2: {G}x{G}x{G} probes over [{lo.round(2).tolist()}, {hi.round(2).tolist()}] x {K} samples = {total} rays, num_of_rays={N}, "
              f"max_depth={D}, limit={LIMIT}, depth={DEPTH}; {args.repeats} alternating rounds of {args.warmup} warm-up + {args.steps} timed launches")
        med = {}
        for name, r in rounds.items():
            med[name] = float(np.median(r))
            print(f"{name:16s} median {med[name]:9.3f} ms  spread {100 * (max(r) - min(r)) / med[name]:5.2f}%  rounds {' '.join(f'{x:.3f}' for x in r)}")
        print(f"{traced} rays traced, {traced / med['probes'] / 1e3:.1f} Mray/s; radiance_probes / path_radiance = {med['probes'] / med['path_radiance']:.3f} x; "
              f"workspace {ws.nbytes / 2 ** 20:.1f} MiB")
        # the same bits: the route's radiance projected on the host in sample order
        dirs = np.ascontiguousarray(dirs_dev.numpy().T).reshape(n, K, 3)
        y = rb.sh_basis(dirs)
        per_sample = np.asarray(rad.radiance).reshape(n, K, 3)
        acc = np.zeros((n, 9, 3))
        for k in range(K):
            acc = acc + y[:, k, :, None] * per_sample[:, k, None, :]
        acc = acc * ((4.0 * math.pi) * (1.0 / K))
        same = acc.tobytes() == np.ascontiguousarray(res.coefficients).tobytes() and \
            np.array_equal(np.asarray(rad.n_rays).reshape(n, K).sum(axis=1, dtype=np.uint64), res.n_rays)
        ok = ok and same
        print(f"the probe query's output {'equals' if same else 'DIFFERS FROM'} the host's ordered projection of path_radiance's bit for bit")
        print(f"the host-side alternative moves {total * 88 / 2 ** 20:.1f} MiB each way ({total} x 88 B: 64 B of ray and 16 B of generator "
              f"down, 24 B of radiance and 8 B of count up, rounded to the larger) against {n * 216 / 2 ** 10:.1f} KiB ({n} x 216 B) of coefficients")
        # the evaluation
        M = args.eval
        rng = np.random.default_rng(1)
        nrm = rng.standard_normal((3, M))
        nrm /= np.linalg.norm(nrm, axis=0, keepdims=True)
        nrm_dev = torch.from_numpy(nrm).cuda()
        idx_dev = torch.from_numpy(rng.integers(0, n, M).astype(np.int32)).cuda()
        eout = DeviceBuffer((3, M), np.float64)
        torch.cuda.synchronize()
        ev = [timed(lambda: ds.sh_eval(out, nrm_dev, idx_dev, rb.SH_HEMISPHERE, n=n, device=True, stream=st, out=eout)) for _ in range(args.repeats)]
        e_med = float(np.median(ev))
        print(f"sh_eval (hemisphere) {M} records against {n} probes: median {e_med * 1e3:.1f} us  spread {100 * (max(ev) - min(ev)) / e_med:.2f}%  "
              f"({M / e_med / 1e6:.2f} G records/s, {M * (4 + 24 + 24 + 216) / e_med / 1e6:.0f} GB/s of records and gathered coefficients)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
