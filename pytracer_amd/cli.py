"""Command-line driver with the flags of pytracer's ``render`` command.

    python -m pytracer_amd render [options] SCENE

Mirrors ``python -m pytracer render`` (main.py:76-214): same options, same defaults, same outputs
(a PFM file and a tone-mapped PNG), with the per-pixel loop running on the MI355X.  The scene-file
language is parsed by pytracer's own parser when pytracer is importable (the parser is out of scope
for this path and stays the reference's); ``SCENE`` may also name a built-in scene —
``builtin:demo`` (the scene of examples/demo.txt), ``builtin:c2`` ... ``builtin:c5`` —
so the driver also runs where pytracer is not installed.
"""
from __future__ import annotations

import sys
from math import isqrt
from time import perf_counter
from typing import Dict, Iterable

import click

from . import hostmodel as hm
from . import scenes
from .tracer import GpuImageTracer

RENDERERS = ["onoff", "flat", "pathtracing", "pointlight"]


class UsageError(Exception):
    """A command-line value the driver cannot use; reported on stderr, exit status 2."""


def parse_float_overrides(switches: Iterable[str]) -> Dict[str, float]:
    """Every ``-d NAME:VALUE`` switch becomes one entry of the scene parser's variable table (the contract of
    main.py:48-70 and scene_file.py:640-675: float variables that override the scene file's own ``float`` lines).
    A switch without exactly one colon, with an empty name, or whose value is not a float is refused."""
    table: Dict[str, float] = {}
    for switch in switches:
        name, colon, text = switch.partition(":")
        if not colon or not name or ":" in text:
            raise UsageError(f"-d expects NAME:VALUE, got {switch!r}")
        try:
            table[name] = float(text)
        except ValueError:
            raise UsageError(f"-d {name}: {text!r} is not a floating-point number") from None
    return table


BUILTIN_SCENES = {  # name -> (spheres, ground plane, "wide" recipe) of SURVEY.md 8(d)
    "c2": (32, True, False), "c3": (32, False, False), "c4": (256, False, True), "c5": (10000, False, True)}


def _load_scene(name: str, variables: Dict[str, float], width: int, height: int):
    """-> (world, camera, classes): ``classes`` supplies the renderer / PCG types matching the world.

    ``builtin:NAME`` builds one of this repository's scene recipes from parameter-holder classes; anything
    else is a scene file in pytracer's language and goes through pytracer's own parser (out of scope for this
    path: it stays the reference's, scene_file.py:640-697), whose objects the flattener reads directly."""
    if name.startswith("builtin:"):
        which = name[len("builtin:"):]
        if which == "demo":
            return (*scenes.demo_world(clock=variables.get("clock", 150.0)), hm)
        if which in BUILTIN_SCENES:
            n, plane, wide = BUILTIN_SCENES[which]
            return scenes.synthetic_world(n, with_plane=plane, wide=wide), scenes.synthetic_camera(width, height), hm
        raise UsageError(f"no built-in scene {which!r} (have: demo, {', '.join(sorted(BUILTIN_SCENES))})")
    try:
        from pytracer import render as ref_render
        from pytracer.pcg import PCG as RefPCG
        from pytracer.scene_file import GrammarError, InputStream, parse_scene
    except ImportError:
        raise UsageError(f"{name}: reading a scene file needs pytracer's parser, and pytracer is not importable "
                         "here; the built-in scenes (builtin:demo, builtin:c2, ...) need nothing") from None
    try:
        with open(name, "rt") as f:
            scene = parse_scene(input_file=InputStream(stream=f, file_name=name), variables=variables)
    except OSError as e:
        raise UsageError(f"{name}: {e.strerror}") from None
    except GrammarError as e:
        at = e.location
        raise UsageError(f"{at.file_name}, line {at.line_num}, column {at.col_num}: {e.message}") from None

    class Ref:  # the reference's own classes, so the flattener sees exactly what main.py would build
        OnOffRenderer, FlatRenderer = ref_render.OnOffRenderer, ref_render.FlatRenderer
        PathTracer, PointLightRenderer = ref_render.PathTracer, ref_render.PointLightRenderer
        PCG = RefPCG

    return scene.world, scene.camera, Ref


class RenderJob:
    """Everything `render` needs before a GPU is touched: scene objects and the renderer parameter holder."""

    def __init__(self, world, camera, renderer, samples_per_side):
        self.world, self.camera, self.renderer, self.samples_per_side = world, camera, renderer, samples_per_side


def plan_render(width, height, algorithm, num_of_rays, max_depth, init_state, init_seq, samples_per_pixel,
                declare_float, input_scene_name) -> RenderJob:
    """Options -> scene + renderer (main.py:144-191 in effect): the sample count must be a perfect square; the
    four algorithms map onto the four renderer classes, only the path tracer takes the ray/depth/seed options."""
    side = isqrt(samples_per_pixel) if samples_per_pixel >= 0 else -1
    if side * side != samples_per_pixel:
        raise UsageError(f"--samples-per-pixel {samples_per_pixel}: must be a perfect square (1, 4, 9, 16, ...)")
    world, camera, K = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    # the seeds are uint64_t at the boundary (include/ptrace.h): any int is taken mod 2^64 here, where every generator class
    # agrees (pytracer's own PCG raises from its first draw for some negative states, pcg.py:39,58)
    init_state, init_seq = int(init_state) & (2**64 - 1), int(init_seq) & (2**64 - 1)
    make = {
        "onoff": lambda: K.OnOffRenderer(world=world),
        "flat": lambda: K.FlatRenderer(world=world),
        "pathtracing": lambda: K.PathTracer(world=world, pcg=K.PCG(init_state=init_state, init_seq=init_seq),
                                            num_of_rays=num_of_rays, max_depth=max_depth),
        "pointlight": lambda: K.PointLightRenderer(world=world),
    }
    return RenderJob(world, camera, make[algorithm](), side)


@click.group()
def cli():
    pass


@click.command("render")
@click.option("--width", type=int, default=640, help="Width of the image to render")
@click.option("--height", type=int, default=480, help="Height of the image to render")
@click.option("--algorithm", type=click.Choice(RENDERERS), default="pathtracing")
@click.option("--pfm-output", type=str, default="output.pfm", help="Name of the PFM file to create")
@click.option("--png-output", type=str, default="output.png", help="Name of the PNG file to create")
@click.option("--num-of-rays", type=int, default=10,
              help="Number of rays departing from each surface point (only with --algorithm=pathtracing).")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth (only with --algorithm=pathtracing).")
@click.option("--init-state", type=int, default=45, help="Initial seed for the random number generator.")
@click.option("--init-seq", type=int, default=54, help="Identifier of the random sequence.")
@click.option("--samples-per-pixel", type=int, default=1, help="Samples per pixel (a perfect square, e.g. 16).")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.option("--pcg-mode", type=click.Choice(["auto", "seq", "pixel", "sample"]), default="auto",
              help="Random streams.  auto (default): onoff / flat / pointlight draw their jitter from the reference's own "
                   "sequential stream PCG(42, 54) -- the frame `python -m pytracer render` writes with the same flags, bit "
                   "for bit -- and pathtracing uses one generator per sample (its scattering stream is serial in the "
                   "reference and cannot be reproduced in parallel; per-sample and per-pixel generators are both pinned by "
                   "reference-held frames and coincide at the default --samples-per-pixel 1).  seq: the reference's stream "
                   "(refused for pathtracing).  pixel: one generator per pixel, consumed in program order (slower with "
                   "--samples-per-pixel > 1: a pixel's samples then depend on each other).  sample: one per sample.")
@click.option("--host-postprocess", is_flag=True, default=False,
              help="Copy the fp64 frame to the host first and post-process there (the round-2 behaviour; same bytes).")
@click.argument("input_scene_name", type=str)
def render(width, height, algorithm, pfm_output, png_output, num_of_rays, max_depth, init_state, init_seq,
           samples_per_pixel, declare_float, device, pcg_mode, host_postprocess, input_scene_name):
    try:
        if pcg_mode == "seq" and algorithm == "pathtracing":
            raise UsageError("--pcg-mode seq with --algorithm pathtracing: the reference's scattering stream is one generator "
                             "consumed in the order the paths of all pixels end in (render.py:118,128) -- serial by "
                             "construction; use sample (what auto, the default, picks for pathtracing) or pixel")
        job = plan_render(width, height, algorithm, num_of_rays, max_depth, init_state, init_seq, samples_per_pixel,
                          declare_float, input_scene_name)
    except UsageError as e:
        click.echo(f"pytracer_amd render: {e}", err=True)
        sys.exit(2)
    from . import _lib, prefer_device_kernargs

    prefer_device_kernargs()  # (this process is ours: kernel arguments in device memory, before its first HIP call)
    _lib.standalone()  # (... and it never imports torch: the frame's HBM and streams come from the C-ABI, pt_device_alloc)
    click.echo(f"{width}x{height} px, {algorithm}, {job.samples_per_side ** 2} sample(s) per pixel, "
               f"{len(job.world.shapes)} shape(s), GPU {device}")
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=job.camera, samples_per_side=job.samples_per_side, device=device,
                            pcg_mode=pcg_mode, resident=not host_postprocess)
    started = perf_counter()
    tracer.fire_all_rays(job.renderer, callback=lambda col, row: click.echo(f"  row {row + 1} of {height}\r", nl=False))
    wall = perf_counter() - started
    st = tracer.last_stats
    click.echo(f"frame done: {wall:.3f} s wall, {st.kernel_ms:.3f} ms in kernels, {st.n_rays} rays")
    # what main.py:203-213 leaves behind: the PFM of the raw frame, then a PNG of the tone-mapped one.  The frame stays
    # in HBM (fp64, like the reference's HdrImage): the PFM floats and the tone-mapped bytes are all that crosses the link
    frame = image if host_postprocess else tracer.device_image
    with open(pfm_output, "wb") as f:
        frame.write_pfm(f)
    frame.normalize_image(factor=1.0)
    frame.clamp_image()
    with open(png_output, "wb") as f:
        frame.write_ldr_image(f, "PNG")
    click.echo(f"wrote {pfm_output} and {png_output}")
    tracer.close()


HIT_CHANNEL_NAMES = ["t", "point", "normal", "uv", "ray", "all"]


@click.command("hits")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--channels", type=str, default="all",
              help="Comma-separated planes to write besides shape_index: " + ", ".join(HIT_CHANNEL_NAMES))
@click.option("--output", type=str, default="frame.npz", help="Name of the .npz file to create")
@click.option("--samples-per-pixel", type=int, default=0,
              help="Samples per pixel (a perfect square; 0: one ray through the pixel centre, no jitter).")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.option("--pcg-mode", type=click.Choice(["auto", "seq", "pixel", "sample"]), default="auto",
              help="Jitter streams (auto = seq: the reference's own stream PCG(42, 54)).")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def hits(width, height, channels, output, samples_per_pixel, declare_float, device, pcg_mode, input_scene_name):
    """First-hit buffers of a scene: what World.ray_intersection returns for every primary ray, as an .npz of planes
    [samples, H, W(, components)] -- shape_index (int32, -1 = no hit) and the selected channels."""
    from . import abi

    try:
        side = isqrt(samples_per_pixel) if samples_per_pixel >= 0 else -1
        if side * side != samples_per_pixel:
            raise UsageError(f"--samples-per-pixel {samples_per_pixel}: must be a perfect square (0, 1, 4, 9, ...)")
        try:
            bits = abi.hit_channels(channels)
        except ValueError as e:
            raise UsageError(f"--channels: {e}") from None
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd hits: {e}", err=True)
        sys.exit(2)
    import numpy as np

    from . import _lib, prefer_device_kernargs

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `render`)
    tracer = GpuImageTracer(image=hm.HdrImage(width, height), camera=camera, samples_per_side=side, device=device,
                            pcg_mode=pcg_mode)
    frame = tracer.fire_all_hits(world, bits)
    st = tracer.last_stats
    np.savez(output, **frame.planes())
    click.echo(f"{width}x{height} px, {frame.nsamp} sample(s) per pixel, {len(world.shapes)} shape(s): "
               f"{st.kernel_ms:.3f} ms in kernels, {st.n_rays} rays; wrote {output} ({', '.join(frame.planes())})")
    tracer.close()


@click.command("rays")
@click.option("--input", "input_name", type=str, required=True, help="A .npy file of [n, 8] rays: origin xyz, direction xyz, tmin, tmax")
@click.option("--output", type=str, default="hits.npz", help="Name of the .npz file to create")
@click.option("--any-hit", is_flag=True, default=False,
              help="Only ask whether anything lies in (tmin, tmax): writes `blocked` (int32, 1 / 0) instead of hit records.")
@click.option("--channels", type=str, default="all", help="Comma-separated planes to write besides shape_index: t, point, normal, uv, all")
@click.option("--width", type=int, default=640, help="Width the scene's camera is built for (built-in scenes)")
@click.option("--height", type=int, default=480, help="Height the scene's camera is built for")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to trace on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def rays(input_name, output, any_hit, channels, width, height, declare_float, device, input_scene_name):
    """World.ray_intersection (or, with --any-hit, the test World.is_point_visible makes) for a file of rays: an .npz of
    shape_index (int32, -1 = no hit) and the selected planes [n(, components)]."""
    import numpy as np

    from . import flatten
    from . import rays as rb

    try:
        try:
            bits = 0 if any_hit else rb.ray_channels(channels)
        except ValueError as e:
            raise UsageError(f"--channels: {e}") from None
        try:
            batch = np.load(input_name)
        except (OSError, ValueError) as e:
            raise UsageError(f"--input {input_name}: {e}") from None
        if batch.ndim != 2 or batch.shape[1] != 8:
            raise UsageError(f"--input {input_name}: expected [n, 8] rays (origin, direction, tmin, tmax), got {batch.shape}")
        world, _, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd rays: {e}", err=True)
        sys.exit(2)
    from . import _lib
    from .device import DeviceScene

    _lib.standalone()  # (torch-free, like `render`)
    block = rb.ray_planes(batch)
    with DeviceScene(flatten.flatten_world(world), device) as scene:
        if any_hit:
            planes = {"blocked": scene.occluded(block)}
        else:
            planes = scene.trace_rays(block, bits).planes()
    np.savez(output, **planes)
    click.echo(f"{block.shape[1]} ray(s), {len(world.shapes)} shape(s): wrote {output} ({', '.join(planes)})")


@click.command("radiance")
@click.option("--input", "input_name", type=str, required=True,
              help="A .npy file of [n, 8] rays (origin xyz, direction xyz, tmin, tmax), or an .npz holding them as `rays` (or as its only array)")
@click.option("--output", type=str, default="radiance.npz", help="Name of the .npz file to create")
@click.option("--num-of-rays", type=int, default=10, help="Number of rays departing from each surface point")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth")
@click.option("--russian-roulette-limit", type=int, default=3, help="Depth from which on the Russian roulette runs")
@click.option("--init-state", type=int, default=45, help="Initial seed of the generators (positive number)")
@click.option("--init-seq", type=int, default=54, help="Identifier of ray 0's sequence: ray i draws from PCG(init_state, init_seq + i)")
@click.option("--depth", type=int, default=0, help="Ray.depth of the rays of the file")
@click.option("--width", type=int, default=640, help="Width the scene's camera is built for (built-in scenes)")
@click.option("--height", type=int, default=480, help="Height the scene's camera is built for")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to trace on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def radiance(input_name, output, num_of_rays, max_depth, russian_roulette_limit, init_state, init_seq, depth, width, height,
             declare_float, device, input_scene_name):
    """PathTracer(world, BLACK, PCG(init_state, init_seq + i), ...)(ray i) for a file of rays: an .npz of radiance [n, 3], the
    generators behind their draws (pcg_state, pcg_inc) and the rays traced per ray (n_rays)."""
    import numpy as np

    from . import flatten
    from . import rays as rb

    try:
        try:
            batch = np.load(input_name)
        except (OSError, ValueError) as e:
            raise UsageError(f"--input {input_name}: {e}") from None
        if not isinstance(batch, np.ndarray):  # an .npz
            names = list(batch.files)
            if "rays" not in names and len(names) != 1:
                raise UsageError(f"--input {input_name}: an .npz must hold the rays as `rays` or as its only array, not {names}")
            batch = batch["rays" if "rays" in names else names[0]]
        if batch.ndim != 2 or batch.shape[1] != 8:
            raise UsageError(f"--input {input_name}: expected [n, 8] rays (origin, direction, tmin, tmax), got {batch.shape}")
        if num_of_rays < 1 or max_depth < 0 or depth < 0:
            raise UsageError("--num-of-rays must be at least 1, --max-depth and --depth not negative")
        if max_depth - depth > 64:
            raise UsageError(f"--max-depth {max_depth} with --depth {depth}: a radiance query walks at most 64 levels; "
                             "`render --algorithm pathtracing` takes deeper paths")
        world, _, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd radiance: {e}", err=True)
        sys.exit(2)
    from . import _lib
    from .device import DeviceScene

    _lib.standalone()  # (torch-free, like `render`)
    block = rb.ray_planes(batch)
    n = block.shape[1]
    pcg = rb.pcg_streams(init_state, [init_seq + i for i in range(n)])
    with DeviceScene(flatten.flatten_world(world), device) as scene:
        res = scene.radiance(block, pcg, num_of_rays, max_depth, russian_roulette_limit, (0.0, 0.0, 0.0), depth, "all")
    planes = res.planes()
    np.savez(output, **planes)
    click.echo(f"{n} ray(s), {len(world.shapes)} shape(s), {int(res.n_rays.sum())} rays traced: wrote {output} ({', '.join(planes)})")


@click.command("gather")
@click.option("--input", "input_name", type=str, default=None,
              help="An .npz holding `points` and `normals`, both [n, 3] (optionally `seqs`, [n]: the stream number of every record's "
                   "sample 0).  Without it: the first hits of the scene's frame of --width x --height pixels")
@click.option("--output", type=str, default="gather.npz", help="Name of the .npz file to create")
@click.option("--samples", type=int, default=16, help="Hemisphere samples per record")
@click.option("--num-of-rays", type=int, default=1, help="Number of rays departing from each surface point below the hemisphere's rays")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth")
@click.option("--russian-roulette-limit", type=int, default=3, help="Depth from which on the Russian roulette runs")
@click.option("--init-state", type=int, default=45, help="Initial seed of the generators (positive number)")
@click.option("--init-seq", type=int, default=54,
              help="Identifier of record 0's first sequence: sample k of record i draws from PCG(init_state, init_seq + i * samples + k)")
@click.option("--depth", type=int, default=0, help="Ray.depth of the hemisphere's rays")
@click.option("--width", type=int, default=640, help="Width of the frame (and what the scene's camera is built for)")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to trace on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def gather(input_name, output, samples, num_of_rays, max_depth, russian_roulette_limit, init_state, init_seq, depth, width, height,
           declare_float, device, input_scene_name):
    """The mean radiance arriving over the hemisphere of surface points (irradiance probes, light-map texels): per record
    `samples` cosine-weighted rays, each followed by PathTracer(world, BLACK, its own generator, ...), averaged on the device in
    sample order.  Writes an .npz of radiance [n, 3] and n_rays [n] -- for a frame [1, H, W(, 3)] beside its shape_index."""
    import numpy as np

    from . import abi
    from . import rays as rb

    try:
        points = normals = seqs = None
        if input_name is not None:
            try:
                batch = np.load(input_name)
            except (OSError, ValueError) as e:
                raise UsageError(f"--input {input_name}: {e}") from None
            names = [] if isinstance(batch, np.ndarray) else list(batch.files)
            if "points" not in names or "normals" not in names:
                raise UsageError(f"--input {input_name}: expected an .npz holding `points` and `normals`, not {names or 'one array'}")
            points, normals = np.asarray(batch["points"], dtype=np.float64), np.asarray(batch["normals"], dtype=np.float64)
            if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
                raise UsageError(f"--input {input_name}: points and normals must both be [n, 3], got {points.shape} and {normals.shape}")
            if "seqs" in names:
                seqs = np.asarray(batch["seqs"])
                if seqs.shape != (points.shape[0],) or seqs.dtype.kind not in "iu":
                    raise UsageError(f"--input {input_name}: seqs must be [n] integers, got {seqs.dtype} {seqs.shape}")
        elif width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        if samples < 1 or num_of_rays < 1 or max_depth < 0 or depth < 0:
            raise UsageError("--samples and --num-of-rays must be at least 1, --max-depth and --depth not negative")
        if max_depth - depth > 64:
            raise UsageError(f"--max-depth {max_depth} with --depth {depth}: a gather query walks at most 64 levels")
        n = points.shape[0] if points is not None else width * height
        if n * samples > rb.MAX_RAYS:
            raise UsageError(f"{n} records x {samples} samples: a gather takes at most 2^31 - 1 hemisphere rays (split the batch)")
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd gather: {e}", err=True)
        sys.exit(2)
    from . import _lib, flatten
    from .device import DeviceScene

    _lib.standalone()  # (torch-free, like `render`)
    kw = dict(num_of_rays=num_of_rays, max_depth=max_depth, russian_roulette_limit=russian_roulette_limit, background=(0.0, 0.0, 0.0),
              depth=depth, channels="all", init_seq=init_seq)
    if points is not None:
        with DeviceScene(flatten.flatten_world(world), device) as scene:
            res = rb.WorldQueries(scene).hemisphere_radiance(points, samples, init_state, seqs, normals=normals, **kw)
        planes = res.planes()
    else:
        tracer = GpuImageTracer(image=hm.HdrImage(width, height), camera=camera, samples_per_side=0, device=device)
        frame = tracer.fire_all_hits(world, abi.HIT_POINT | abi.HIT_NORMAL)
        res = tracer.world_queries(world).hemisphere_radiance(frame, samples, init_state, None, **kw)
        planes = dict(res.planes(), shape_index=np.asarray(frame.shape_index))
        tracer.close()
    np.savez(output, **planes)
    click.echo(f"{res.n} record(s) x {samples} sample(s), {len(world.shapes)} shape(s), {int(res.n_rays.sum())} rays traced: "
               f"wrote {output} ({', '.join(planes)})")


def parse_size(text: str):
    """``WxH`` -> (W, H), both at least 1."""
    w, x, h = text.lower().partition("x")
    try:
        size = (int(w), int(h)) if x else None
    except ValueError:
        size = None
    if size is None or size[0] < 1 or size[1] < 1:
        raise UsageError(f"--size expects WxH with W and H at least 1, got {text!r}")
    return size


BAKE_WINDOW_SAMPLES = 1 << 24  # hemisphere rays per window of a bake: 512 MiB of sample planes in the workspace


@click.command("bake")
@click.option("--shape", type=int, required=True, help="Index in World.shapes of the shape whose map is baked (a DiffuseBRDF shape)")
@click.option("--size", type=str, default="256x256", help="Texels of the map over the shape's (u, v) square: WxH")
@click.option("--samples", type=int, default=64, help="Samples per texel")
@click.option("--side", type=int, default=1, help="1: the side the shape's local normal points to (a sphere's outside); -1: the other")
@click.option("--no-jitter", is_flag=True, default=False, help="Every sample at its texel's centre")
@click.option("--output", "-o", type=str, default="map.pfm", help="Name of the PFM file to create")
@click.option("--num-of-rays", type=int, default=1, help="Number of rays departing from each surface point below the hemisphere's rays")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth")
@click.option("--russian-roulette-limit", type=int, default=3, help="Depth from which on the Russian roulette runs")
@click.option("--init-state", type=int, default=45, help="Initial seed of the generators (positive number)")
@click.option("--init-seq", type=int, default=54,
              help="Identifier of texel 0's first sequence: sample k of texel t draws from PCG(init_state, init_seq + t * samples + k)")
@click.option("--depth", type=int, default=1, help="Ray.depth of the hemisphere's rays (1: the children of a camera ray's hit)")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to bake on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def bake(shape, size, samples, side, no_jitter, output, num_of_rays, max_depth, russian_roulette_limit, init_state, init_seq, depth,
         declare_float, device, input_scene_name):
    """The outgoing-radiance map of one diffuse shape: per texel of its (u, v) grid, emitted + brdf colour x the mean radiance
    arriving over the hemisphere of `samples` points of the texel.  Writes a PFM -- the ImagePigment of scenes.baked_world, with
    which FlatRenderer renders the shape's converged indirect light."""
    from . import rays as rb

    try:
        width, height = parse_size(size)
        if side not in (1, -1):
            raise UsageError(f"--side {side}: must be 1 or -1")
        if samples < 1 or num_of_rays < 1 or max_depth < 0 or depth < 0:
            raise UsageError("--samples and --num-of-rays must be at least 1, --max-depth and --depth not negative")
        if max_depth - depth > 64:
            raise UsageError(f"--max-depth {max_depth} with --depth {depth}: a bake walks at most 64 levels")
        if width * samples > rb.MAX_RAYS:
            raise UsageError(f"{width} texels x {samples} samples in one row: a bake window takes at most 2^31 - 1 hemisphere rays")
        world, _, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), 640, 480)
        if not 0 <= shape < len(world.shapes):
            raise UsageError(f"--shape {shape}: the scene has {len(world.shapes)} shape(s)")
        if type(world.shapes[shape].material.brdf).__name__ != "DiffuseBRDF":
            raise UsageError(f"--shape {shape}: a {type(world.shapes[shape].material.brdf).__name__} shape -- what a mirror sends out "
                             "depends on where it is seen from, a map cannot hold it")
    except UsageError as e:
        click.echo(f"pytracer_amd bake: {e}", err=True)
        sys.exit(2)
    from types import SimpleNamespace

    import numpy as np

    from . import _lib, flatten
    from .device import DeviceScene

    _lib.standalone()  # (torch-free, like `render`)
    rows_per = max(1, BAKE_WINDOW_SAMPLES // (width * samples))
    out = np.empty((height, width, 3), dtype=np.float64)
    traced = 0
    started = perf_counter()
    with DeviceScene(flatten.flatten_world(world), device) as scene:
        wq = rb.WorldQueries(scene)
        centres = rb.texel_centres(width, height)
        mat = wq.materials(SimpleNamespace(shape_index=np.full((height, width), shape, np.int32), uv=centres))
        for row0 in range(0, height, rows_per):  # (the texel index is global: the windows are the whole map, bit for bit)
            h = min(rows_per, height - row0)
            part = wq.light_map(shape, width, height, samples, side, not no_jitter, (0, row0, width, h), depth, init_state, init_seq,
                                num_of_rays, max_depth, russian_roulette_limit)
            out[row0: row0 + h] = np.asarray(mat.emitted)[row0: row0 + h] + np.asarray(mat.brdf_color)[row0: row0 + h] * part.radiance
            traced += int(part.n_rays.sum())
    wall = perf_counter() - started
    image = hm.HdrImage(width, height)
    image.set_array(out)
    with open(output, "wb") as f:
        image.write_pfm(f)
    click.echo(f"shape {shape}: {width}x{height} texels x {samples} sample(s), {len(world.shapes)} shape(s), {traced} rays traced, "
               f"{wall:.3f} s: wrote {output}")


def parse_grid(text: str):
    """``ox,oy,oz,step,nx,ny,nz`` -> (origin, step, dims) of a :class:`pytracer_amd.rays.ProbeGrid`."""
    parts = text.split(",")
    try:
        if len(parts) != 7:
            raise ValueError
        origin, step = tuple(float(x) for x in parts[:3]), float(parts[3])
        dims = tuple(int(x) for x in parts[4:])
    except ValueError:
        raise UsageError(f"--grid expects ox,oy,oz,step,nx,ny,nz (four numbers, three counts), got {text!r}") from None
    if not step > 0.0 or min(dims) < 1:
        raise UsageError(f"--grid {text}: the step must be positive and nx, ny, nz at least 1")
    return origin, step, dims


@click.command("probes")
@click.option("--grid", type=str, default=None, help="Probes on a lattice: ox,oy,oz,step,nx,ny,nz (probe (ix, iy, iz) has index (iz * ny + iy) * nx + ix)")
@click.option("--input", "input_name", type=str, default=None,
              help="Probes at the [n, 3] points of a .npy file, or of an .npz holding them as `points` (or as its only array)")
@click.option("--output", type=str, default="probes.npz", help="Name of the .npz file to create")
@click.option("--samples", type=int, default=256, help="Samples (rays uniform on the sphere) per probe")
@click.option("--num-of-rays", type=int, default=1, help="Number of rays departing from each surface point below the probes' rays")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth")
@click.option("--russian-roulette-limit", type=int, default=3, help="Depth from which on the Russian roulette runs")
@click.option("--init-state", type=int, default=45, help="Initial seed of the generators (positive number)")
@click.option("--init-seq", type=int, default=54,
              help="Identifier of probe 0's first sequence: sample k of probe i draws from PCG(init_state, init_seq + i * samples + k)")
@click.option("--depth", type=int, default=1, help="Ray.depth of the probes' rays (1: the children of a camera ray's hit)")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to trace on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def probes(grid, input_name, output, samples, num_of_rays, max_depth, russian_roulette_limit, init_state, init_seq, depth, declare_float,
           device, input_scene_name):
    """Radiance probes at free points of the scene: per point the 27 order-2 spherical-harmonic coefficients of the radiance
    arriving there (`samples` rays uniform on the sphere, each followed by PathTracer(world, BLACK, its own generator, ...),
    projected on the device in sample order).  Writes an .npz of coefficients [n, 9, 3], n_rays [n] and points [n, 3]."""
    import numpy as np

    from . import rays as rb

    try:
        if (grid is None) == (input_name is None):
            raise UsageError("the probes' points come from --grid or from --input: give one of them")
        if samples < 1 or num_of_rays < 1 or max_depth < 0 or depth < 0:
            raise UsageError("--samples and --num-of-rays must be at least 1, --max-depth and --depth not negative")
        if max_depth - depth > 64:
            raise UsageError(f"--max-depth {max_depth} with --depth {depth}: a probe walks at most 64 levels")
        if grid is not None:
            lattice = rb.ProbeGrid(*parse_grid(grid))
            n = lattice.n  # (counted before the points are made: a lattice can be asked for that no memory holds)
        else:
            try:
                batch = np.load(input_name)
            except (OSError, ValueError) as e:
                raise UsageError(f"--input {input_name}: {e}") from None
            if not isinstance(batch, np.ndarray):  # an .npz
                names = list(batch.files)
                if "points" not in names and len(names) != 1:
                    raise UsageError(f"--input {input_name}: an .npz must hold the points as `points` or as its only array, not {names}")
                batch = batch["points" if "points" in names else names[0]]
            if batch.ndim != 2 or batch.shape[1] != 3 or batch.dtype.kind not in "fiu":
                raise UsageError(f"--input {input_name}: expected [n, 3] points, got {batch.dtype} {batch.shape}")
            points = np.asarray(batch, dtype=np.float64)
            n = points.shape[0]
        if n * samples > rb.MAX_RAYS:
            raise UsageError(f"{n} probes x {samples} samples: a call takes at most 2^31 - 1 rays (split the points)")
        if grid is not None:
            points = lattice.points()
        world, _, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), 640, 480)
    except UsageError as e:
        click.echo(f"pytracer_amd probes: {e}", err=True)
        sys.exit(2)
    from . import _lib, flatten
    from .device import DeviceScene

    _lib.standalone()  # (torch-free, like `render`)
    with DeviceScene(flatten.flatten_world(world), device) as scene:
        res = rb.WorldQueries(scene).radiance_probes(points, samples, init_state, init_seq, None, None, num_of_rays, max_depth,
                                                     russian_roulette_limit, (0.0, 0.0, 0.0), depth, "all")
    planes = dict(res.planes(), points=points)
    np.savez(output, **planes)
    click.echo(f"{n} probe(s) x {samples} sample(s), {len(world.shapes)} shape(s), {int(res.n_rays.sum())} rays traced: "
               f"wrote {output} ({', '.join(planes)})")


def load_probes(name: str, n: int):
    """The ``coefficients`` of the .npz the ``probes`` command wrote, as the ``[27, n]`` block of a lattice of ``n`` probes."""
    import numpy as np

    try:
        batch = np.load(name)
        if isinstance(batch, np.ndarray):
            raise UsageError(f"--probes {name}: an array, not the .npz the probes command writes")
        with batch:
            if "coefficients" not in batch.files:
                raise UsageError(f"--probes {name}: no `coefficients` in it ({', '.join(batch.files)}): not written by the probes command?")
            c = np.asarray(batch["coefficients"])
    except (OSError, ValueError) as e:
        raise UsageError(f"--probes {name}: {e}") from None
    if c.ndim != 3 or c.shape[1:] != (9, 3) or c.dtype.kind != "f":
        raise UsageError(f"--probes {name}: expected coefficients [n, 9, 3], got {c.dtype} {c.shape}")
    if c.shape[0] != n:
        raise UsageError(f"--probes {name} holds {c.shape[0]} probes, the lattice of --grid has {n}")
    return np.ascontiguousarray(np.asarray(c, dtype=np.float64).transpose(1, 2, 0)).reshape(27, n)


@click.command("lit")
@click.option("--probes", "probes_name", type=str, required=True, help="The .npz the probes command wrote for the lattice of --grid")
@click.option("--grid", type=str, required=True, help="The probes' lattice: ox,oy,oz,step,nx,ny,nz (as given to the probes command)")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--output", type=str, default="frame.pfm", help="Name of the .pfm file to create")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def lit(probes_name, grid, width, height, output, declare_float, device, input_scene_name):
    """A frame of the scene lit by a lattice of radiance probes: per pixel emitted + brdf_color * E, with E the eight probes
    around the hit point blended and evaluated on the device (the hemisphere mean around the normal of a diffuse surface, the
    radiance from the mirror direction of a specular one); black where nothing is hit.  Writes a PFM."""
    from . import rays as rb

    try:
        if width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        lattice = rb.ProbeGrid(*parse_grid(grid))
        block = load_probes(probes_name, lattice.n)
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd lit: {e}", err=True)
        sys.exit(2)
    from . import _lib, prefer_device_kernargs
    from .shaders import ProbeLitShader

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `probes`)
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=camera, samples_per_side=0, device=device)
    probe_set = rb.ProbeSet(block.reshape(-1).view("uint8"), lattice.n, 0, evaluator=tracer.world_queries(world).scene.sh_eval)
    started = perf_counter()
    tracer.fire_all_rays(ProbeLitShader(world, lattice, probe_set, tracer))
    wall = perf_counter() - started
    with open(output, "wb") as f:
        image.write_pfm(f)
    click.echo(f"{width}x{height} px, {len(world.shapes)} shape(s), a lattice of {'x'.join(str(d) for d in lattice.dims)} probes, "
               f"{wall:.3f} s: wrote {output}")
    tracer.close()


@click.command("denoise")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--samples", type=int, default=4, help="Hemisphere rays per pixel of the gather that is filtered")
@click.option("--passes", type=int, default=4, help="Filter passes, 1 to 10: pass i has the step 2^i")
@click.option("--sigma-point", type=float, default=0.1, help="Distance from the centre's tangent plane, per step, at which a tap's weight halves (inf: off)")
@click.option("--normal-power-log2", type=int, default=5, help="e in 0..10: a tap is weighted by cos^(2^e) of the angle between the normals")
@click.option("--sigma-colour", type=float, default=float("inf"), help="Colour distance at which a tap's weight halves (default inf: off)")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth of the gather's walks")
@click.option("--init-state", type=int, default=45, help="Initial seed for the random number generator.")
@click.option("--init-seq", type=int, default=54, help="Identifier of the first random sequence.")
@click.option("--pfm-output", type=str, default="frame.pfm", help="Name of the PFM file to create")
@click.option("--png-output", type=str, default=None, help="Name of a PNG file of the tone-mapped frame (default: none)")
@click.option("--noisy-output", type=str, default=None, help="Name of a PFM file for the same frame without the filter (default: none)")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def denoise(width, height, samples, passes, sigma_point, normal_power_log2, sigma_colour, max_depth, init_state, init_seq, pfm_output, png_output,
            noisy_output, declare_float, device, input_scene_name):
    """A frame of the scene lit by one bounce of few rays and an edge-avoiding filter: per pixel emitted + brdf_color * E, with E
    the mean radiance over the hit's hemisphere from --samples rays, filtered over the frame under the guidance of the hit
    records (shape, point, normal) on the device; black where nothing is hit.  Writes a PFM."""
    import math

    try:
        if width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        if samples < 1:
            raise UsageError("--samples must be at least 1")
        if not 1 <= passes <= 10:
            raise UsageError("--passes must be 1 to 10")
        if not 0 <= normal_power_log2 <= 10:
            raise UsageError("--normal-power-log2 must be 0 to 10")
        if not sigma_point > 0.0 or not sigma_colour > 0.0 or math.isnan(sigma_point) or math.isnan(sigma_colour):
            raise UsageError("--sigma-point and --sigma-colour must be positive (or inf)")
        if max_depth < 0:
            raise UsageError("--max-depth must not be negative")
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd denoise: {e}", err=True)
        sys.exit(2)
    from . import _lib, prefer_device_kernargs
    from .shaders import DenoisedGatherShader

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `lit`)
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=camera, samples_per_side=0, device=device)
    shader = DenoisedGatherShader(world, tracer, samples, init_state=init_state, init_seq=init_seq, max_depth=max_depth, passes=passes,
                                  sigma_point=sigma_point, normal_power_log2=normal_power_log2, sigma_colour=sigma_colour)
    wrote = []
    started = perf_counter()
    if noisy_output:
        shader.filtered = False
        tracer.fire_all_rays(shader)
        with open(noisy_output, "wb") as f:
            image.write_pfm(f)
        wrote.append(noisy_output)
        shader.filtered = True
    tracer.fire_all_rays(shader)
    wall = perf_counter() - started
    with open(pfm_output, "wb") as f:
        image.write_pfm(f)
    wrote.append(pfm_output)
    if png_output:
        image.normalize_image(factor=1.0)
        image.clamp_image()
        with open(png_output, "wb") as f:
            image.write_ldr_image(f, "PNG")
        wrote.append(png_output)
    click.echo(f"{width}x{height} px, {len(world.shapes)} shape(s), {samples} ray(s) per pixel, {passes} filter pass(es), "
               f"{wall:.3f} s: wrote {' and '.join(wrote)}")
    tracer.close()


@click.command("temporal")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--frames", type=int, default=8, help="Frames to render; the last one is written")
@click.option("--step-deg", type=float, default=1.0, help="The camera turns by this many degrees about z from one frame to the next")
@click.option("--samples", type=int, default=4, help="Hemisphere rays per pixel and frame")
@click.option("--max-history", type=int, default=32, help="Frames after which the running mean becomes an exponential average, 1 to 2^20")
@click.option("--normal-min", type=float, default=0.9, help="Least cosine between this frame's normal and a history tap's, -1 to 1")
@click.option("--point-tolerance", type=float, default=0.05, help="Largest distance of a history tap from the pixel's tangent plane (inf: off)")
@click.option("--passes", type=int, default=4, help="Filter passes behind the accumulation, 1 to 10; 0: no filter")
@click.option("--sigma-point", type=float, default=0.1, help="The filter's: distance from the tangent plane, per step, at which a tap's weight halves")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth of the gather's walks")
@click.option("--init-state", type=int, default=45, help="Initial seed for the random number generator.")
@click.option("--init-seq", type=int, default=54, help="Identifier of the first random sequence.")
@click.option("--pfm-output", type=str, default="frame.pfm", help="Name of the PFM file to create")
@click.option("--no-history-output", type=str, default=None, help="Name of a PFM file for the same last frame without accumulation (default: none)")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def temporal(width, height, frames, step_deg, samples, max_history, normal_min, point_tolerance, passes, sigma_point, max_depth, init_state,
             init_seq, pfm_output, no_history_output, declare_float, device, input_scene_name):
    """The last of --frames frames of a camera that turns about z, each lit by one bounce of few rays whose mean is accumulated
    over the frames: last frame's accumulated mean is reprojected onto this frame's hit points through last frame's camera,
    checked against the hit records (shape, normal, point) and blended in on the device; then the edge-avoiding filter, then
    emitted + brdf_color * E.  Writes a PFM."""
    import math

    try:
        if width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        if frames < 1:
            raise UsageError("--frames must be at least 1")
        if not math.isfinite(step_deg):
            raise UsageError("--step-deg must be finite")
        if samples < 1:
            raise UsageError("--samples must be at least 1")
        if not 1 <= max_history <= 2 ** 20:
            raise UsageError("--max-history must be 1 to 2^20")
        if not -1.0 <= normal_min <= 1.0:
            raise UsageError("--normal-min must be -1 to 1")
        if not point_tolerance > 0.0:
            raise UsageError("--point-tolerance must be positive (or inf)")
        if not 0 <= passes <= 10:
            raise UsageError("--passes must be 0 to 10")
        if not sigma_point > 0.0:
            raise UsageError("--sigma-point must be positive (or inf)")
        if max_depth < 0:
            raise UsageError("--max-depth must not be negative")
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd temporal: {e}", err=True)
        sys.exit(2)
    from . import _lib, prefer_device_kernargs
    from .shaders import TemporalGatherShader

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `denoise`)
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=camera, samples_per_side=0, device=device)
    shader = TemporalGatherShader(world, tracer, samples, init_state=init_state, init_seq=init_seq, max_depth=max_depth, filtered=passes > 0,
                                  passes=max(passes, 1), sigma_point=sigma_point, max_history=max_history, normal_min=normal_min,
                                  point_tolerance=point_tolerance)
    wrote = []
    started = perf_counter()
    for f in range(frames):
        tracer.camera = scenes.turned_camera(camera, step_deg * f)
        if f == frames - 1 and no_history_output:
            shader.accumulate = False
            tracer.fire_all_rays(shader)
            with open(no_history_output, "wb") as out:
                image.write_pfm(out)
            wrote.append(no_history_output)
            shader.accumulate = True
        tracer.fire_all_rays(shader)
    wall = perf_counter() - started
    with open(pfm_output, "wb") as out:
        image.write_pfm(out)
    wrote.append(pfm_output)
    count = shader.accumulator.count
    click.echo(f"{width}x{height} px, {len(world.shapes)} shape(s), {frames} frame(s) of {samples} ray(s) per pixel, {step_deg:g} degree(s) per frame, "
               f"longest history {int(count.max())}, {wall:.3f} s: wrote {' and '.join(wrote)}")
    tracer.close()


@click.command("variance")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--frames", type=int, default=8, help="Frames to render; the last one is written")
@click.option("--step-deg", type=float, default=1.0, help="The camera turns by this many degrees about z from one frame to the next")
@click.option("--samples", type=int, default=4, help="Hemisphere rays per pixel and frame")
@click.option("--max-history", type=int, default=32, help="Frames after which the running mean becomes an exponential average, 1 to 2^20")
@click.option("--min-history", type=int, default=4, help="History length below which the variance is estimated over a 7x7 window, 1 to 2^20")
@click.option("--normal-min", type=float, default=0.9, help="Least cosine between this frame's normal and a history or window tap's, -1 to 1")
@click.option("--point-tolerance", type=float, default=0.05, help="Largest distance of such a tap from the pixel's tangent plane (inf: off)")
@click.option("--passes", type=int, default=4, help="Filter passes behind the accumulation, 1 to 10; 0: no filter")
@click.option("--sigma-point", type=float, default=0.1, help="The filter's: distance from the tangent plane, per step, at which a tap's weight halves")
@click.option("--sigma-luminance", type=float, default=1.0,
              help="The filter's: luminance difference, in standard deviations of the pixel, at which a tap's weight halves (inf: off)")
@click.option("--epsilon", type=float, default=1e-10, help="The filter's: what is added to the scaled variance, positive and finite")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth of the gather's walks")
@click.option("--init-state", type=int, default=45, help="Initial seed for the random number generator.")
@click.option("--init-seq", type=int, default=54, help="Identifier of the first random sequence.")
@click.option("--pfm-output", type=str, default="frame.pfm", help="Name of the PFM file to create")
@click.option("--variance-output", type=str, default=None, help="Name of a PFM file (grey) of the last frame's variance before the filter (default: none)")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def variance(width, height, frames, step_deg, samples, max_history, min_history, normal_min, point_tolerance, passes, sigma_point, sigma_luminance,
             epsilon, max_depth, init_state, init_seq, pfm_output, variance_output, declare_float, device, input_scene_name):
    """The last of --frames frames of a camera that turns about z, each lit by one bounce of few rays whose mean AND whose luminance
    moments are accumulated over the frames; from the moments a variance per pixel, and then an edge-avoiding filter whose
    luminance weight is scaled by that variance, so that it blurs a pixel as hard as the pixel is still noisy; then emitted +
    brdf_color * E.  Writes a PFM."""
    import math

    try:
        if width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        if frames < 1:
            raise UsageError("--frames must be at least 1")
        if not math.isfinite(step_deg):
            raise UsageError("--step-deg must be finite")
        if samples < 1:
            raise UsageError("--samples must be at least 1")
        if not 1 <= max_history <= 2 ** 20:
            raise UsageError("--max-history must be 1 to 2^20")
        if not 1 <= min_history <= 2 ** 20:
            raise UsageError("--min-history must be 1 to 2^20")
        if not -1.0 <= normal_min <= 1.0:
            raise UsageError("--normal-min must be -1 to 1")
        if not point_tolerance > 0.0:
            raise UsageError("--point-tolerance must be positive (or inf)")
        if not 0 <= passes <= 10:
            raise UsageError("--passes must be 0 to 10")
        if not sigma_point > 0.0:
            raise UsageError("--sigma-point must be positive (or inf)")
        if not sigma_luminance > 0.0:
            raise UsageError("--sigma-luminance must be positive (or inf)")
        if not (epsilon > 0.0 and math.isfinite(epsilon)):
            raise UsageError("--epsilon must be positive and finite")
        if max_depth < 0:
            raise UsageError("--max-depth must not be negative")
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd variance: {e}", err=True)
        sys.exit(2)
    import numpy as np

    from . import _lib, prefer_device_kernargs
    from .shaders import VarianceGuidedGatherShader

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `temporal`)
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=camera, samples_per_side=0, device=device)
    shader = VarianceGuidedGatherShader(world, tracer, samples, init_state=init_state, init_seq=init_seq, max_depth=max_depth, filtered=passes > 0,
                                        passes=max(passes, 1), sigma_point=sigma_point, sigma_luminance=sigma_luminance, epsilon=epsilon,
                                        max_history=max_history, min_history=min_history, normal_min=normal_min, point_tolerance=point_tolerance)
    wrote = []
    started = perf_counter()
    for f in range(frames):
        tracer.camera = scenes.turned_camera(camera, step_deg * f)
        tracer.fire_all_rays(shader)
    wall = perf_counter() - started
    with open(pfm_output, "wb") as out:
        image.write_pfm(out)
    wrote.append(pfm_output)
    last = np.asarray(shader.last_variance, dtype=np.float64)
    if variance_output:
        grey = hm.HdrImage(width, height)
        grey.set_array(np.repeat(last.reshape(height, width, 1), 3, axis=-1))
        with open(variance_output, "wb") as out:
            grey.write_pfm(out)
        wrote.append(variance_output)
    count = shader.accumulator.count
    click.echo(f"{width}x{height} px, {len(world.shapes)} shape(s), {frames} frame(s) of {samples} ray(s) per pixel, {step_deg:g} degree(s) per frame, "
               f"longest history {int(count.max())}, mean variance {float(last.mean()):.3e}, {wall:.3f} s: wrote {' and '.join(wrote)}")
    tracer.close()


@click.command("adaptive")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--frames", type=int, default=8, help="Frames to render; the last one is written")
@click.option("--step-deg", type=float, default=1.0, help="The camera turns by this many degrees about z from one frame to the next")
@click.option("--samples", type=int, default=4, help="Hemisphere rays per pixel of the first frame, which is sampled uniformly")
@click.option("--min-samples", type=int, default=1, help="Least rays a hit pixel gets in a later frame, 1 to --max-samples")
@click.option("--max-samples", type=int, default=32, help="Most rays a pixel gets in a later frame, up to 2^20")
@click.option("--tolerance", type=float, default=0.05, help="Relative standard error of a pixel's luminance the counts aim at, positive")
@click.option("--luminance-floor", type=float, default=1.0, help="Least luminance the tolerance is relative to, positive and finite")
@click.option("--gain", type=float, default=1.0, help="Scales every count, positive and finite")
@click.option("--budget", type=int, default=None, help="Most rays a later frame may take; beyond it the frame is cut off in pixel order (default: none)")
@click.option("--max-history", type=int, default=32, help="Frames after which the running mean becomes an exponential average, 1 to 2^20")
@click.option("--min-history", type=int, default=4, help="History length below which the variance is estimated over a 7x7 window, 1 to 2^20")
@click.option("--passes", type=int, default=4, help="Filter passes behind the accumulation, 1 to 10; 0: no filter")
@click.option("--sigma-luminance", type=float, default=1.0,
              help="The filter's: luminance difference, in standard deviations of the pixel, at which a tap's weight halves (inf: off)")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth of the gather's walks")
@click.option("--init-state", type=int, default=45, help="Initial seed for the random number generator.")
@click.option("--init-seq", type=int, default=54, help="Identifier of the first random sequence.")
@click.option("--pfm-output", type=str, default="frame.pfm", help="Name of the PFM file to create")
@click.option("--counts-output", type=str, default=None, help="Name of a PFM file (grey) of the last frame's sample counts (default: none)")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def adaptive(width, height, frames, step_deg, samples, min_samples, max_samples, tolerance, luminance_floor, gain, budget, max_history, min_history,
             passes, sigma_luminance, max_depth, init_state, init_seq, pfm_output, counts_output, declare_float, device, input_scene_name):
    """The `variance` command with rays that go where the noise is: the first of --frames frames is lit by --samples rays per pixel,
    every later one by as many rays per pixel as the accumulated estimate's variance asks for (--tolerance, --gain, clamped into
    --min-samples .. --max-samples), gathered in one ragged batch; then the accumulation, the variance-guided filter and emitted +
    brdf_color * E.  Writes a PFM."""
    import math

    try:
        if width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        if frames < 1:
            raise UsageError("--frames must be at least 1")
        if not math.isfinite(step_deg):
            raise UsageError("--step-deg must be finite")
        if samples < 1:
            raise UsageError("--samples must be at least 1")
        if not 1 <= min_samples <= max_samples:
            raise UsageError("--min-samples must be 1 to --max-samples")
        if max_samples > 2 ** 20:
            raise UsageError("--max-samples must be at most 2^20")
        if not tolerance > 0.0:
            raise UsageError("--tolerance must be positive (or inf)")
        if not (luminance_floor > 0.0 and math.isfinite(luminance_floor)):
            raise UsageError("--luminance-floor must be positive and finite")
        if not (gain > 0.0 and math.isfinite(gain)):
            raise UsageError("--gain must be positive and finite")
        if budget is not None and not 0 <= budget <= 2 ** 31 - 1:
            raise UsageError("--budget must be 0 to 2^31 - 1")
        if not 1 <= max_history <= 2 ** 20:
            raise UsageError("--max-history must be 1 to 2^20")
        if not 1 <= min_history <= 2 ** 20:
            raise UsageError("--min-history must be 1 to 2^20")
        if not 0 <= passes <= 10:
            raise UsageError("--passes must be 0 to 10")
        if not sigma_luminance > 0.0:
            raise UsageError("--sigma-luminance must be positive (or inf)")
        if max_depth < 0:
            raise UsageError("--max-depth must not be negative")
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd adaptive: {e}", err=True)
        sys.exit(2)
    import numpy as np

    from . import _lib, prefer_device_kernargs
    from .shaders import AdaptiveGatherShader

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `variance`)
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=camera, samples_per_side=0, device=device)
    shader = AdaptiveGatherShader(world, tracer, samples, init_state=init_state, init_seq=init_seq, max_depth=max_depth, filtered=passes > 0,
                                  budget=budget, passes=max(passes, 1), sigma_luminance=sigma_luminance, max_history=max_history,
                                  min_history=min_history, min_samples=min_samples, max_samples=max_samples, tolerance=tolerance,
                                  luminance_floor=luminance_floor, gain=gain)
    wrote, totals = [], []
    started = perf_counter()
    for f in range(frames):
        tracer.camera = scenes.turned_camera(camera, step_deg * f)
        tracer.fire_all_rays(shader)
        totals.append(shader.last_total)
    wall = perf_counter() - started
    with open(pfm_output, "wb") as out:
        image.write_pfm(out)
    wrote.append(pfm_output)
    if counts_output:
        last = np.zeros((height, width)) if shader.last_counts is None else np.asarray(shader.last_counts, dtype=np.float64)
        grey = hm.HdrImage(width, height)
        grey.set_array(np.repeat(last.reshape(height, width, 1), 3, axis=-1))
        with open(counts_output, "wb") as out:
            grey.write_pfm(out)
        wrote.append(counts_output)
    count = shader.accumulator.count
    click.echo(f"{width}x{height} px, {len(world.shapes)} shape(s), {frames} frame(s), {step_deg:g} degree(s) per frame, "
               f"rays per frame {' '.join(str(t) for t in totals)}, longest history {int(count.max())}, {wall:.3f} s: wrote {' and '.join(wrote)}")
    tracer.close()


@click.command("weighted")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--frames", type=int, default=8, help="Frames to render; the last one is written")
@click.option("--step-deg", type=float, default=1.0, help="The camera turns by this many degrees about z from one frame to the next")
@click.option("--samples", type=int, default=4, help="Hemisphere rays per pixel of the first frame, which is sampled uniformly")
@click.option("--min-samples", type=int, default=1, help="Least rays a hit pixel gets in a later frame, 0 to --max-samples")
@click.option("--max-samples", type=int, default=32, help="Most rays a pixel gets in a later frame, up to 2^20")
@click.option("--tolerance", type=float, default=0.05, help="Relative standard error of a pixel's luminance the counts aim at, positive")
@click.option("--luminance-floor", type=float, default=1.0, help="Least luminance the tolerance is relative to, positive and finite")
@click.option("--gain", type=float, default=1.0, help="Scales every count, positive and finite")
@click.option("--budget", type=int, default=None,
              help="Most rays a later frame may take; beyond it the frame is cut off in pixel order and keeps its history (default: none)")
@click.option("--max-history", type=int, default=32, help="The longest history length that is counted, 1 to 2^20")
@click.option("--max-weight", type=float, default=128.0, help="Samples after which the weighted mean becomes an exponential average, 0 to inf")
@click.option("--blend-weight", is_flag=True, help="A history's weight is the blend of its taps' weights, not the largest of them")
@click.option("--min-history", type=int, default=4, help="History length below which the variance is estimated over a 7x7 window, 1 to 2^20")
@click.option("--passes", type=int, default=4, help="Filter passes behind the accumulation, 1 to 10; 0: no filter")
@click.option("--sigma-luminance", type=float, default=1.0,
              help="The filter's: luminance difference, in standard deviations of the pixel, at which a tap's weight halves (inf: off)")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth of the gather's walks")
@click.option("--init-state", type=int, default=45, help="Initial seed for the random number generator.")
@click.option("--init-seq", type=int, default=54, help="Identifier of the first random sequence.")
@click.option("--pfm-output", type=str, default="frame.pfm", help="Name of the PFM file to create")
@click.option("--counts-output", type=str, default=None, help="Name of a PFM file (grey) of the last frame's sample counts (default: none)")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def weighted(width, height, frames, step_deg, samples, min_samples, max_samples, tolerance, luminance_floor, gain, budget, max_history, max_weight,
             blend_weight, min_history, passes, sigma_luminance, max_depth, init_state, init_seq, pfm_output, counts_output, declare_float, device,
             input_scene_name):
    """The `adaptive` command with an accumulation that weights every frame by the rays it took: a pixel's 31-ray frame counts 31 times
    its 1-ray frame, a pixel that got no ray (--min-samples 0, or a --budget that ran out) keeps its history, and the accumulation
    and the variance estimate are two launches.  Writes a PFM."""
    import math

    try:
        if width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        if frames < 1:
            raise UsageError("--frames must be at least 1")
        if not math.isfinite(step_deg):
            raise UsageError("--step-deg must be finite")
        if samples < 1:
            raise UsageError("--samples must be at least 1")
        if not 0 <= min_samples <= max_samples:
            raise UsageError("--min-samples must be 0 to --max-samples")
        if max_samples > 2 ** 20:
            raise UsageError("--max-samples must be at most 2^20")
        if not tolerance > 0.0:
            raise UsageError("--tolerance must be positive (or inf)")
        if not (luminance_floor > 0.0 and math.isfinite(luminance_floor)):
            raise UsageError("--luminance-floor must be positive and finite")
        if not (gain > 0.0 and math.isfinite(gain)):
            raise UsageError("--gain must be positive and finite")
        if budget is not None and not 0 <= budget <= 2 ** 31 - 1:
            raise UsageError("--budget must be 0 to 2^31 - 1")
        if not 1 <= max_history <= 2 ** 20:
            raise UsageError("--max-history must be 1 to 2^20")
        if not max_weight >= 0.0:
            raise UsageError("--max-weight must not be negative (inf: no cap)")
        if not 1 <= min_history <= 2 ** 20:
            raise UsageError("--min-history must be 1 to 2^20")
        if not 0 <= passes <= 10:
            raise UsageError("--passes must be 0 to 10")
        if not sigma_luminance > 0.0:
            raise UsageError("--sigma-luminance must be positive (or inf)")
        if max_depth < 0:
            raise UsageError("--max-depth must not be negative")
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
    except UsageError as e:
        click.echo(f"pytracer_amd weighted: {e}", err=True)
        sys.exit(2)
    import numpy as np

    from . import _lib, prefer_device_kernargs
    from .shaders import WeightedAdaptiveGatherShader

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `adaptive`)
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=camera, samples_per_side=0, device=device)
    shader = WeightedAdaptiveGatherShader(world, tracer, samples, init_state=init_state, init_seq=init_seq, max_depth=max_depth,
                                          filtered=passes > 0, budget=budget, passes=max(passes, 1), sigma_luminance=sigma_luminance,
                                          max_history=max_history, max_weight=max_weight, blend_weight=blend_weight, min_history=min_history,
                                          min_samples=min_samples, max_samples=max_samples, tolerance=tolerance, luminance_floor=luminance_floor,
                                          gain=gain)
    wrote, totals = [], []
    started = perf_counter()
    for f in range(frames):
        tracer.camera = scenes.turned_camera(camera, step_deg * f)
        tracer.fire_all_rays(shader)
        totals.append(shader.last_total)
    wall = perf_counter() - started
    with open(pfm_output, "wb") as out:
        image.write_pfm(out)
    wrote.append(pfm_output)
    if counts_output:
        last = np.zeros((height, width)) if shader.last_counts is None else np.asarray(shader.last_counts, dtype=np.float64)
        grey = hm.HdrImage(width, height)
        grey.set_array(np.repeat(last.reshape(height, width, 1), 3, axis=-1))
        with open(counts_output, "wb") as out:
            grey.write_pfm(out)
        wrote.append(counts_output)
    count, weight = shader.accumulator.count, shader.accumulator.weight
    click.echo(f"{width}x{height} px, {len(world.shapes)} shape(s), {frames} frame(s), {step_deg:g} degree(s) per frame, "
               f"rays per frame {' '.join(str(t) for t in totals)}, longest history {int(count.max())}, largest weight {float(np.max(weight)):g}, "
               f"{wall:.3f} s: wrote {' and '.join(wrote)}")
    tracer.close()


def parse_moves(switches: Iterable[str], n_shapes: int) -> Dict[int, tuple]:
    """``SHAPE:DX:DY:DZ`` switches -> {shape index: (dx, dy, dz)}; a shape named twice moves by the sum."""
    import math

    moves: Dict[int, tuple] = {}
    for text in switches:
        parts = text.split(":")
        try:
            if len(parts) != 4:
                raise ValueError
            shape, step = int(parts[0]), tuple(float(x) for x in parts[1:])
        except ValueError:
            raise UsageError(f"--move={text!r}: expected SHAPE:DX:DY:DZ") from None
        if not 0 <= shape < n_shapes:
            raise UsageError(f"--move={text!r}: the world has shapes 0 to {n_shapes - 1}")
        if not all(math.isfinite(x) for x in step):
            raise UsageError(f"--move={text!r}: the step must be finite")
        old = moves.get(shape, (0.0, 0.0, 0.0))
        moves[shape] = tuple(a + b for a, b in zip(old, step))
    return moves


def moved_world(world, moves: Dict[int, tuple], times: int):
    """A ``World`` with the shapes and lights of ``world``, those in ``moves`` translated by ``times`` of their step."""
    import copy

    out = copy.copy(world)
    out.shapes = list(world.shapes)
    for shape, (dx, dy, dz) in moves.items():
        s = copy.copy(world.shapes[shape])
        s.transformation = hm.translation(hm.Vec(dx * times, dy * times, dz * times)) * s.transformation
        out.shapes[shape] = s
    return out


@click.command("motion")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--frames", type=int, default=8, help="Frames to render; the last one is written")
@click.option("--step-deg", type=float, default=1.0, help="The camera turns by this many degrees about z from one frame to the next")
@click.option("--samples", type=int, default=4, help="Hemisphere rays per pixel and frame")
@click.option("--move", type=str, multiple=True, help="SHAPE:DX:DY:DZ: that shape is translated by that much per frame (repeatable)")
@click.option("--no-follow", is_flag=True, help="Reproject through the camera only (the weighted accumulate query), for comparison")
@click.option("--max-history", type=int, default=32, help="Frames after which the running mean becomes an exponential average, 1 to 2^20")
@click.option("--passes", type=int, default=4, help="Filter passes behind the accumulation, 1 to 10; 0: no filter")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth of the gather's walks")
@click.option("--init-state", type=int, default=45, help="Initial seed for the random number generator.")
@click.option("--init-seq", type=int, default=54, help="Identifier of the first random sequence.")
@click.option("--pfm-output", type=str, default="frame.pfm", help="Name of the PFM file to create")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def motion(width, height, frames, step_deg, samples, move, no_follow, max_history, passes, max_depth, init_state, init_seq, pfm_output,
           declare_float, device, input_scene_name):
    """The last of --frames frames of a camera that turns about z over a world whose --move shapes are translated from frame to
    frame, each lit by one bounce of few rays whose mean is accumulated over the frames by the motion accumulate query: the history
    of a shape that moved is fetched where that surface point was on the previous screen.  Then the variance-guided filter, then
    emitted + brdf_color * E.  Writes a PFM."""
    import math

    try:
        if width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        if frames < 1:
            raise UsageError("--frames must be at least 1")
        if not math.isfinite(step_deg):
            raise UsageError("--step-deg must be finite")
        if samples < 1:
            raise UsageError("--samples must be at least 1")
        if not 1 <= max_history <= 2 ** 20:
            raise UsageError("--max-history must be 1 to 2^20")
        if not 0 <= passes <= 10:
            raise UsageError("--passes must be 0 to 10")
        if max_depth < 0:
            raise UsageError("--max-depth must not be negative")
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
        moves = parse_moves(move, len(world.shapes))
    except UsageError as e:
        click.echo(f"pytracer_amd motion: {e}", err=True)
        sys.exit(2)
    from . import _lib, prefer_device_kernargs
    from .shaders import MovingWorldGatherShader

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `temporal`)
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=camera, samples_per_side=0, device=device)
    shader = MovingWorldGatherShader(world, tracer, samples, init_state=init_state, init_seq=init_seq, max_depth=max_depth, filtered=passes > 0,
                                     passes=max(passes, 1), max_history=max_history)
    shader.follow = not no_follow
    started = perf_counter()
    for f in range(frames):
        tracer.camera = scenes.turned_camera(camera, step_deg * f)
        shader.world = moved_world(world, moves, f)
        tracer.fire_all_rays(shader)
    wall = perf_counter() - started
    with open(pfm_output, "wb") as out:
        image.write_pfm(out)
    count = shader.accumulator.count
    click.echo(f"{width}x{height} px, {len(world.shapes)} shape(s), {len(moves)} moving{'' if shader.follow else ' (not followed)'}, {frames} frame(s) of "
               f"{samples} ray(s) per pixel, {step_deg:g} degree(s) per frame, longest history {int(count.max())}, {wall:.3f} s: wrote {pfm_output}")
    tracer.close()


@click.command("gradient")
@click.option("--width", type=int, default=640, help="Width of the frame")
@click.option("--height", type=int, default=480, help="Height of the frame")
@click.option("--frames", type=int, default=8, help="Frames to render; the last one is written")
@click.option("--step-deg", type=float, default=1.0, help="The camera turns by this many degrees about z from one frame to the next")
@click.option("--samples", type=int, default=4, help="Hemisphere rays per pixel and frame")
@click.option("--move", type=str, multiple=True, help="SHAPE:DX:DY:DZ: that shape is translated by that much per frame (repeatable)")
@click.option("--no-follow-light", is_flag=True, help="Follow the shapes only (the motion accumulate query), for comparison")
@click.option("--stratum", type=int, default=3, help="One probe per block of this many pixels squared, 1 to 16")
@click.option("--radius", type=int, default=1, help="A pixel listens to the probes of (2 radius + 1)^2 blocks, 0 to 4")
@click.option("--gain", type=float, default=8.0, help="How much of the history a relative change of 1 takes away; 0: nothing")
@click.option("--max-history", type=int, default=32, help="Frames after which the running mean becomes an exponential average, 1 to 2^20")
@click.option("--passes", type=int, default=4, help="Filter passes behind the accumulation, 1 to 10; 0: no filter")
@click.option("--max-depth", type=int, default=3, help="Maximum allowed ray depth of the gather's walks")
@click.option("--init-state", type=int, default=45, help="Initial seed for the random number generator.")
@click.option("--init-seq", type=int, default=54, help="Identifier of the first random sequence.")
@click.option("--pfm-output", type=str, default="frame.pfm", help="Name of the PFM file to create")
@click.option("--declare-float", "-d", type=str, multiple=True, help="Declare a variable: --declare-float=VAR:VALUE")
@click.option("--device", type=int, default=0, help="GPU to render on")
@click.argument("input_scene_name", type=str, default="builtin:demo")
def gradient(width, height, frames, step_deg, samples, move, no_follow_light, stratum, radius, gain, max_history, passes, max_depth, init_state,
             init_seq, pfm_output, declare_float, device, input_scene_name):
    """The last of --frames frames of a camera that turns about z over a world whose --move shapes are translated from frame to
    frame, as `motion` renders them, with the gradient accumulate query: one probe per block of the frame is gathered again in the
    PREVIOUS frame's world with this frame's random streams, and where the light changed -- under a shadow that moved -- the history
    counts for less.  Then the variance-guided filter, then emitted + brdf_color * E.  Writes a PFM."""
    import math

    import numpy as np

    try:
        if width < 1 or height < 1:
            raise UsageError("--width and --height must be at least 1")
        if frames < 1:
            raise UsageError("--frames must be at least 1")
        if not math.isfinite(step_deg):
            raise UsageError("--step-deg must be finite")
        if samples < 1:
            raise UsageError("--samples must be at least 1")
        if not 1 <= stratum <= 16:
            raise UsageError("--stratum must be 1 to 16")
        if not 0 <= radius <= 4:
            raise UsageError("--radius must be 0 to 4")
        if not gain >= 0.0:
            raise UsageError("--gain must not be negative")
        if not 1 <= max_history <= 2 ** 20:
            raise UsageError("--max-history must be 1 to 2^20")
        if not 0 <= passes <= 10:
            raise UsageError("--passes must be 0 to 10")
        if max_depth < 0:
            raise UsageError("--max-depth must not be negative")
        world, camera, _ = _load_scene(input_scene_name, parse_float_overrides(declare_float), width, height)
        moves = parse_moves(move, len(world.shapes))
    except UsageError as e:
        click.echo(f"pytracer_amd gradient: {e}", err=True)
        sys.exit(2)
    from . import _lib, prefer_device_kernargs
    from .shaders import GradientGatherShader

    prefer_device_kernargs()
    _lib.standalone()  # (torch-free, like `motion`)
    image = hm.HdrImage(width, height)
    tracer = GpuImageTracer(image=image, camera=camera, samples_per_side=0, device=device)
    shader = GradientGatherShader(world, tracer, samples, init_state=init_state, init_seq=init_seq, max_depth=max_depth, filtered=passes > 0,
                                  passes=max(passes, 1), max_history=max_history, stratum=stratum, radius=radius, gain=gain)
    shader.follow_light = not no_follow_light
    started = perf_counter()
    for f in range(frames):
        tracer.camera = scenes.turned_camera(camera, step_deg * f)
        shader.world = moved_world(world, moves, f)
        tracer.fire_all_rays(shader)
    wall = perf_counter() - started
    with open(pfm_output, "wb") as out:
        image.write_pfm(out)
    count, keep = np.asarray(shader.accumulator.count), getattr(shader.accumulator, "keep", None)
    cut = 0 if keep is None else int((np.asarray(keep) < 1.0).sum())
    click.echo(f"{width}x{height} px, {len(world.shapes)} shape(s), {len(moves)} moving{'' if shader.follow_light else ' (light not followed)'}, "
               f"{frames} frame(s) of {samples} ray(s) per pixel, {step_deg:g} degree(s) per frame, longest history {int(count.max())}, "
               f"mean history {float(count.mean()):.2f}, {cut} pixel(s) kept less than all of theirs, {wall:.3f} s: wrote {pfm_output}")
    tracer.close()


cli.add_command(render)
cli.add_command(lit)
cli.add_command(denoise)
cli.add_command(temporal)
cli.add_command(variance)
cli.add_command(adaptive)
cli.add_command(weighted)
cli.add_command(motion)
cli.add_command(gradient)
cli.add_command(hits)
cli.add_command(rays)
cli.add_command(radiance)
cli.add_command(gather)
cli.add_command(bake)
cli.add_command(probes)
