"""Frames whose pixel and sample indices leave 32 bits, as the eight or sixteen rows of them that hold the crossing.

include/ptrace.h accepts frames of up to 2^40 pixels.  Every kernel forms for itself the global pixel index
``gpix = row * W + col``, the generator index (``gpix`` under PT_PCG_PIXEL, ``gpix * nsamp + k`` under PT_PCG_SAMPLE) and,
under PT_PCG_SEQ, the draw count ``2 * nsamp * gpix``; tests/seed_sweep.py moves the SEEDS across 2^32 / 2^63 / 2^64 and
keeps these indices small on purpose.  Here the seeds are small (45, 54) and the index alone carries the high bits: each
case is a catalogue case of tests/variant_catalog.py (world, camera kind, params, tuning, planned kernels) on a frame so
large that the index crosses 2^31 or 2^32 (2^33 under SEQ) in the middle of ONE block of rows, and that block -- the
share of rank ``row // row_block`` of ``ceil(H / row_block)`` ranks -- is what is rendered: a few hundred thousand pixels.

The frame of a case follows from its width, the factor the index grows by per pixel (1, ``nsamp`` or ``2 * nsamp``) and the
boundary: the crossing pixel is ``ceil(2^bits / factor)``, its row lies about half-way down (``H = 2 * row + 3`` or the
next height off the 8 / 16 grid), so the strip looks along the horizon of the catalogue's cameras, over the spheres' centres,
and the camera's ``aspect_ratio`` is 16 / 9 whatever W / H is.  ``fit`` steps the width up from its nominal value until the
crossing row is neither the first nor the last of its block and the crossing column is well inside the row.

    nominal width    frames                                          what they add
    60001            pix    ~71 600 / ~143 200 rows                  the cheap kernels, every alignment
    4099             narrow ~1.05e6 / ~2.1e6 rows                    the path tracer (33 k pixels per block)
    131              tall   2^25 / 2^26 rows                         rows beyond 2^24: no fp32 holds the row
    262147           wide   ~16 400 / ~32 800 rows                   columns beyond 2^18; OnOff / Flat only
    7683             samp   S = 9 / S = 12 under SAMPLE              ``gpix * nsamp`` at frame sizes in use
    131075           pano   ~16 400 / ~32 800 rows, aspect 8         the path tracer's per-pixel cones beyond column 2^16

Seeding sites (tests/seed_sweep.py's table) and the cases that take each across 2^31 and 2^32 (id + ``-31`` / ``-32``):

    pt_simple.h  pcg_seed_pixel   P simple-flat-ortho, simple-pointlight      Q seq-simple-flat
    pt_simple.h  per sample       S simple-flat-sample (nsamp 4)
    pt_tile.h    pcg_seed_pixel   P tile-onoff, tile-flat-hier (+ pt_cell_kernel), tile-flat-ortho, tall-tile-onoff,
                                    tall-tile-flat-hier (2^31 only: the cell lists), wide-tile-onoff
                                  Q seq-tile-onoff, seq-tile-flat, seq-tile-pointlight, seq-tile-flat-ortho
    pt_tile.h    per sample       S tile-pointlight (nsamp 1), tile-pointlight-ortho (nsamp 4), samp-tile-flat (81 / 144)
    pt_hits.h    both             P, S, Q tests/test_gpu_geometry.py: the hit frames (HIT_FRAMES below)
    pt_path.h    one lane / queue P path-one-lane-pixel (nsamp 4)             S path-one-lane (nsamp 1), path-one-lane-sample (4),
                                                                                queue-handover (nsamp 4: path_start_sample)
    pt_path.h    regions / queue  P regions, regions-plain, tall-regions, pano-regions, queue, queue-handover-pixel
                                  S regions-centre-sample (S = 0), regions-sample (nsamp 4)
    pt_tree.h    tree             P tree; behind a hand-over: queue-handover-pixel
    pt_tree.h    tree, per sample S tree-balls (nsamp 1), tree-sample (nsamp 4); behind a hand-over: queue-handover
    16x16 tiles  (no generator)   tile4-flat-lds, tile4-flat-nolds, tall-tile4-flat, wide-tile4-onoff-f32: the pixel index
                                  and the cone model only (16-row blocks)

What the catalogue leaves out, and why nothing is lost by it:

* The widths are nominal: ``fit`` moves each to the next width at which the crossing lies inside its block (60001, 60003, ...);
  the heights follow from the crossing row (``H ~ 2 * row``), so the wide and the pano frames are ~16 400 / ~32 800 rows high.
* SEQ: every kernel has a 2^32 and a 2^33 strip, the one-lane, the OnOff and the orthogonal kernel a 2^31 strip as well.  An
  ``int`` draw count shows on BOTH sides of a 2^32 crossing (tests/test_frame_geometry.py, condition 4), so the 2^32 strips of
  the Flat and the PointLight kernel cover what their 2^31 strips would.
* The wide frames are OnOff only (8x8 tiles jittered, 16x16 tiles in fp32): a Flat strip of 2 M pixels adds shading, which
  holds no index, to the same seeding site and the same cone model.
* The hit-record frames cross 2^32 only (same argument), and "samp32" is 1031 pixels wide, not 7680: a hit frame holds 15 fp64
  planes per SAMPLE, and 8 rows of 7680 pixels at 144 samples are 1.1 GB to download and to walk in Python; the crossing of
  ``gpix * 144`` does not depend on the width.

A plain helper module: no fixtures, no hooks.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from pytracer_amd import abi, flatten
from pytracer_amd import hostmodel as hm
from tests import variant_catalog as vc

M64 = (1 << 64) - 1
ASPECT = 16.0 / 9.0
# a panorama: at 2^17 columns a pixel is still 1.2e-4 rad wide, more than the slack of ``pixel_cone`` / ``cone_keeps`` (some 5e-5
# rad), so the first pass's per-pixel classification still depends on WHICH pixel's cone it is given
PANORAMA = 8.0
SEEDS = (45, 54)
P, S, Q = abi.PCG_PIXEL, abi.PCG_SAMPLE, abi.PCG_SEQ

PIX, NARROW, TALL, WIDE, SAMP, PANO = 60001, 4099, 131, 262147, 7683, 131075


@dataclass(frozen=True)
class Geo:
    id: str                    # the case is ``id-<bits>``
    base: str                  # the catalogue case it is: world, camera kind, params, tuning, worker / hand-over
    width: int                 # nominal width (``fit`` may step it up)
    mode: int                  # the alignment (the catalogue case's own, or SEQ)
    kernels: Tuple[str, str, str, str]  # what the share plans
    bits: Tuple[int, ...] = (31, 32)
    row_block: int = 8
    params: Dict = field(default_factory=dict)   # changes to the catalogue case's params
    worker: Optional[int] = None                 # where the share lets another kernel work than the catalogue's frame
    handover: Optional[bool] = None
    down: float = 0.5                            # how far down the frame the crossing row lies (0.5: on the horizon)
    aspect: float = ASPECT                       # the camera's ``aspect_ratio``


_TILE = lambda r: ("", "", f"pt_tile_kernel<{r}>", "")  # noqa: E731
_REGIONS = ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", "")
_TREE = ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>")

GEOS = [
    # ---- one lane per pixel ----------------------------------------------------------------------------------------------
    Geo("simple-flat-ortho", "simple-flat-ortho-jitter", PIX, P, ("", "", "pt_simple_kernel<FLAT, noHOIST>", "")),
    Geo("simple-pointlight", "simple-pointlight-hoist", PIX, P, ("", "", "pt_simple_kernel<POINTLIGHT, HOIST>", "")),
    Geo("simple-flat-sample", "simple-flat-hoist-jitter", PIX, S, ("", "", "pt_simple_kernel<FLAT, HOIST>", "")),
    # ---- 8x8 tiles ---------------------------------------------------------------------------------------------------------
    Geo("tile-onoff", "tile-onoff-jitter", PIX, P, _TILE("ONOFF")),
    # (cell lists for the WHOLE frame, 2 GiB at the most: 32 spheres with ``hier_min`` 16, 64 slots per cell, and the strip a
    # little below half-way down, where it also sees the ground plane's far end)
    Geo("tile-flat-hier", "sw-hier_min-16-flat", PIX, P, ("pt_cell_kernel", "", "pt_tile_kernel<FLAT, HIER>", ""), down=0.51),
    Geo("tile-flat-ortho", "tile-flat-ortho-jitter", PIX, P, _TILE("FLAT, ORTHO")),
    # (the gallery's spheres stand lower than the camera: the strip looks a little below the horizon, the dome still ends its rays)
    Geo("tile-pointlight", "tile-pointlight", PIX, S, _TILE("POINTLIGHT"), down=0.5115),
    Geo("tile-pointlight-ortho", "tile-pointlight-ortho", PIX, S, _TILE("POINTLIGHT, ORTHO"), down=0.6),
    Geo("samp-tile-flat", "tile-flat-share-rb8", SAMP, S, _TILE("FLAT"), bits=(31,), params=dict(samples_per_side=9, pcg_mode=S)),
    Geo("samp-tile-flat", "tile-flat-share-rb8", SAMP, S, _TILE("FLAT"), bits=(32,), params=dict(samples_per_side=12, pcg_mode=S)),
    Geo("tall-tile-onoff", "tile-onoff-jitter", TALL, P, _TILE("ONOFF")),
    Geo("tall-tile-flat-hier", "sw-hier_min-16-flat", TALL, P, ("pt_cell_kernel", "", "pt_tile_kernel<FLAT, HIER>", ""), bits=(31,)),
    Geo("wide-tile-onoff", "tile-onoff-jitter", WIDE, P, _TILE("ONOFF")),
    # ---- 16x16 tiles: sixteen-row blocks ----------------------------------------------------------------------------------
    Geo("tile4-flat-lds", "tile4-flat-lds-share-rb16", PIX, P, ("", "", "pt_tile4_kernel<FLAT, LDS>", ""), row_block=16),
    Geo("tile4-flat-nolds", "tile4-flat-nolds", PIX, P, ("", "", "pt_tile4_kernel<FLAT, noLDS>", ""), row_block=16),
    Geo("tall-tile4-flat", "tile4-flat-lds-share-rb16", TALL, P, ("", "", "pt_tile4_kernel<FLAT, LDS>", ""), row_block=16),
    Geo("wide-tile4-onoff-f32", "tile4-onoff-f32", WIDE, P, ("", "", "pt_tile4_kernel<ONOFF, noLDS>", ""), row_block=16),
    # ---- the path tracer, on the narrow frames ----------------------------------------------------------------------------
    Geo("path-one-lane", "path-one-lane", NARROW, S, ("", "", "pt_path_kernel", "")),
    Geo("path-one-lane-sample", "path-one-lane", NARROW, S, ("", "", "pt_path_kernel", ""), params=dict(samples_per_side=2)),
    Geo("path-one-lane-pixel", "sw-cull-0-path", NARROW, P, ("", "", "pt_path_kernel", "")),
    Geo("regions", "regions-lds-scene-lean", NARROW, P, _REGIONS),
    Geo("regions-sample", "regions-lds-scene-lean", NARROW, S, _REGIONS, params=dict(pcg_mode=S)),
    Geo("regions-centre-sample", "regions-lds-scene-lean-centre-sample", NARROW, S, _REGIONS),
    Geo("tall-regions", "regions-lds-scene-lean", TALL, P, _REGIONS),
    Geo("pano-regions", "regions-lds-scene-lean", PANO, P, _REGIONS, aspect=PANORAMA),
    # a "plain" path world: uniform pigments, and ``rr_limit`` beyond ``max_depth`` (no roulette decision a last-bit difference
    # of sin / cos could flip): held to the oracle bit for bit, with its ray count (tests/test_gpu_geometry.py: PLAIN)
    Geo("regions-plain", "regions-lds-scene-lean", NARROW, P, _REGIONS, params=dict(rr_limit=4)),
    Geo("tree", "tree-lean-scene", NARROW, P, _TREE),
    Geo("tree-sample", "tree-lean-scene", NARROW, S, _TREE, params=dict(samples_per_side=2, num_of_rays=4, pcg_mode=S)),
    Geo("tree-balls", "tree-balls", NARROW, S,
        ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_tree_kernel", "pt_path_flagged_kernel<LDS>")),
    Geo("queue", "flagged-lean-lds-queue", NARROW, P, _TREE),
    Geo("queue-handover", "flagged-lean-lds-handover", NARROW, S, _TREE),
    Geo("queue-handover-pixel", "flagged-split-handover", NARROW, P,
        ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_tree_kernel", "pt_path_flagged_kernel<SPLIT>")),
    # ---- the SEQ alignment: 2 * nsamp * gpix draws into the one stream -------------------------------------------------------
    Geo("seq-simple-flat", "simple-flat-hoist-jitter", PIX, Q, ("", "", "pt_simple_kernel<FLAT, HOIST>", ""), bits=(31, 32, 33)),
    Geo("seq-tile-onoff", "tile-onoff-jitter", PIX, Q, _TILE("ONOFF"), bits=(31, 32, 33)),
    Geo("seq-tile-flat", "tile-flat-share-rb8", PIX, Q, _TILE("FLAT"), bits=(32, 33), params=dict(samples_per_side=2)),
    Geo("seq-tile-pointlight", "tile-pointlight", PIX, Q, _TILE("POINTLIGHT"), bits=(32, 33), down=0.5115),
    Geo("seq-tile-flat-ortho", "tile-flat-ortho-jitter", PIX, Q, _TILE("FLAT, ORTHO"), bits=(31, 32, 33)),
]


def nsamp_of(samples_per_side: int) -> int:
    return max(int(samples_per_side), 1) ** 2


def factor(mode: int, samples_per_side: int) -> int:
    """What the index a kernel forms grows by from one pixel to the next: the generator index (PIXEL: ``gpix``; SAMPLE:
    ``gpix * nsamp + k``; without jitter, S = 0, both are ``gpix``) or, under SEQ, the draw count ``2 * nsamp * gpix``."""
    n = nsamp_of(samples_per_side)
    if mode == Q:
        return 2 * n
    return n if mode == S and samples_per_side > 0 else 1


def fit(width: int, per_pixel: int, bits: int, row_block: int, down: float = 0.5) -> Tuple[int, int, int, int]:
    """-> (W, H, row, col): the first odd width from ``width`` on, off the 8 / 16 grid, at which the crossing pixel
    ``ceil(2^bits / per_pixel)`` is neither in the first nor in the last row of its block of ``row_block`` rows and more
    than 8 columns from either end of its row; H puts that row ``down`` of the way down (half-way), off the grid as well."""
    W = width
    while True:
        if W % 2 and W % 8:
            row, col = divmod(-(-(1 << bits) // per_pixel), W)
            if 0 < row % row_block < row_block - 1 and 8 < col < W - 8:
                H = int(row / down) + 3
                while H % 2 == 0 or H % 8 == 0:
                    H += 1
                return W, H, row, col
        W += 1


@dataclass(frozen=True)
class Case:
    id: str
    geo: Geo
    bits: int
    case: vc.Case              # the catalogue case on the large frame, its params selecting the block of rows
    crossing: Tuple[int, int]  # (row, col) of the crossing pixel, global

    @property
    def mode(self) -> int:
        return self.geo.mode


def _make(geo: Geo, bits: int) -> Case:
    base = vc.BY_ID[geo.base]
    kw = dict(base.params, **geo.params)
    kw["pcg_mode"] = geo.mode
    S_ = kw.get("samples_per_side", 0)
    W, H, row, col = fit(geo.width, factor(geo.mode, S_), bits, geo.row_block, geo.down)
    rb = geo.row_block
    kw.update(row_block=rb, n_ranks=-(-H // rb), rank=row // rb)
    if geo.mode == Q:
        kw.update(jitter_state=SEEDS[0], jitter_seq=SEEDS[1], path_state=0x0123456789ABCDEF, path_seq=2**40 + 3)
    else:
        kw.update(path_state=SEEDS[0], path_seq=SEEDS[1], jitter_state=0x0123456789ABCDEF, jitter_seq=2**40 + 3)
    case = dataclasses.replace(base, id=f"{geo.id}-{bits}", size=(W, H), params=kw, kernels=geo.kernels,
                               worker=geo.worker if geo.worker is not None else base.worker,
                               handover=geo.handover if geo.handover is not None else base.handover)
    return Case(case.id, geo, bits, case, (row, col))


CASES: List[Case] = [_make(g, b) for g in GEOS for b in g.bits]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"


# ---- cameras, parameters, rows ---------------------------------------------------------------------------------------------------
def camera_of(kind: str, aspect: float = ASPECT) -> abi.Camera:
    """tests/variant_catalog.py's cameras with ``aspect_ratio`` 16 / 9 instead of W / H (a frame of 131 x 2^26 pixels
    would be a sliver: the strip must show the world)."""
    if kind == "orthogonal":
        return flatten.flatten_camera(hm.OrthogonalCamera(aspect, hm.translation(hm.Vec(-1.0, 0.0, 1.5)) * hm.scaling(hm.Vec(1.0, 5.0, 3.0))))
    return flatten.flatten_camera(hm.PerspectiveCamera(screen_distance=1.0, aspect_ratio=aspect,
                                                       transformation=hm.translation(hm.Vec(-1.0, 0.0, 1.0))))


def camera(c: Case) -> abi.Camera:
    return camera_of(c.case.camera, c.geo.aspect)


def scene(c: Case) -> abi.FlatScene:
    return vc.scene(c.case)


def params(c: Case) -> abi.Params:
    return vc.params(c.case)


def rows(c: Case) -> List[int]:
    return vc.rows(c.case)


def plan(c: Case) -> abi.PlanInfo:
    from pytracer_amd import device

    with vc.tuned(c.case):
        return device.plan(scene(c), camera(c), params(c))


def nsamp(p: abi.Params) -> int:
    return nsamp_of(p.samples_per_side)


def index_of(p: abi.Params, gpix: int, k: int = 0) -> int:
    """The index the kernels form for sample ``k`` of pixel ``gpix``: the number added to ``path_seq`` (PIXEL, SAMPLE) or
    the number of draws the SEQ stream is entered at."""
    n = nsamp(p)
    if p.pcg_mode == Q:
        return 2 * (n * gpix + k)
    return gpix * n + k if p.pcg_mode == S and p.samples_per_side > 0 else gpix


def crossing_gpix(c: Case) -> int:
    return c.crossing[0] * c.case.size[0] + c.crossing[1]


def before_end(c: Case) -> int:
    """The last pixel all of whose indices lie below the boundary: the one before the crossing pixel, or the one before
    that where the boundary falls between two samples of a pixel (SAMPLE with ``nsamp`` no power of two)."""
    p = params(c)
    at = crossing_gpix(c)
    return at - 1 if index_of(p, at - 1, nsamp(p) - 1) < (1 << c.bits) else at - 2


# ---- the oracle on a share, and on what a 32-bit index would make of it ----------------------------------------------------------
def low32(i: int) -> int:
    """The index kept in an ``unsigned`` temporary."""
    return i & 0xFFFFFFFF


def sext32(i: int) -> int:
    """The index kept in an ``int`` temporary and widened afterwards (mod 2^64 where it is added to a seed)."""
    i &= 0xFFFFFFFF
    return i - (1 << 32) if i >> 31 else i


def shifted(p: abi.Params, delta: int) -> abi.Params:
    """``p`` as the oracle must be given it to render its share with every index ``delta`` larger (``delta`` <= 0 here).
    PIXEL / SAMPLE: the index is added to ``path_seq``.  SEQ: ``pto_render`` starts its serial loop at the share's first
    pixel with the generator it is given, so that generator is the frame's advanced on the host to the first pixel's
    draw count (tests/test_pcg_seq.py::test_seq_distances_beyond_32_bits), ``delta`` draws further on."""
    if p.pcg_mode != Q:
        return abi.copy_params(p, path_seq=(p.path_seq + delta) & M64)
    first = abi.rows_for_rank(p.height, p.row_block, p.n_ranks, p.rank)[0] * p.width
    g = hm.PCG(p.jitter_state, p.jitter_seq)
    g.state = hm.pcg_advance(g.state, g.inc, (index_of(p, first) + delta) & M64)
    js, jq = flatten.recover_seeds(g)
    return abi.copy_params(p, jitter_state=js, jitter_seq=jq)


def oracle_params(c: Case) -> abi.Params:
    """The params under which ``oracle.render`` gives the share of ``c`` (its own, but for SEQ: see ``shifted``)."""
    return shifted(params(c), 0)


def narrowed(c: Case, narrow) -> Tuple[int, int]:
    """(delta before, delta at and after the crossing pixel): what ``narrow`` (``low32`` / ``sext32``) adds to the index on
    either side of the crossing.  One number per side: a share is far shorter than 2^31 indices."""
    p, at = params(c), crossing_gpix(c)
    r = rows(c)
    first, last = r[0] * p.width, r[-1] * p.width + p.width - 1
    n = nsamp(p)
    sides = []
    for lo, hi in ((index_of(p, first), index_of(p, before_end(c), n - 1)), (index_of(p, at), index_of(p, last, n - 1))):
        d = narrow(lo) - lo
        assert narrow(hi) - hi == d, f"{c.id}: one side of the crossing spans another boundary"
        sides.append(d)
    return sides[0], sides[1]


# ---- hit-record frames -----------------------------------------------------------------------------------------------------------
# (name, nominal width, samples per side): each under PIXEL, SAMPLE and SEQ, the index crossing 2^32; the world is C2 with its
# plane (32 spheres: tests/test_gpu_hits.py's "c2p")
HIT_FRAMES = [("pix32", PIX, 2), ("tall", TALL, 2), ("samp32", 1031, 12)]
_HITS = ("", "", "pt_hits_kernel", "")
HIT_CASES: List[Case] = [_make(Geo(f"hits-{name}-{tag}", "tile-flat-share-rb8", width, mode, _HITS, params=dict(samples_per_side=sps)), 32)
                         for name, width, sps in HIT_FRAMES for tag, mode in (("pixel", P), ("sample", S), ("seq", Q))]


def window(c: Case, reach: int = 24, ends: int = 4) -> List[Tuple[int, int]]:
    """(local row, col) of the pixels a hit frame is compared at: ``reach`` pixels on either side of the crossing pixel in
    row-major order and the first and last ``ends`` columns of every row of the share."""
    W = c.case.size[0]
    r = rows(c)
    at = crossing_gpix(c)
    px = {divmod(g, W) for g in range(at - reach, at + reach)}
    px |= {(row, col) for row in r for col in list(range(ends)) + list(range(W - ends, W))}
    return sorted((r.index(row), col) for row, col in px)


def oracle_hits(orc, c: Case, pixels):
    """tests/util.py's ``oracle_frame`` for the pixels ``(local row, col)`` of a share alone, each index summed here in
    Python: -> dict of arrays [nsamp, len(pixels), ...] (shape_index, t, point, normal, uv, ray_origin, ray_dir)."""
    import ctypes as C

    import numpy as np

    L = orc.lib()
    p, flat, cam = params(c), scene(c), camera(c)
    n, sps, W, H = nsamp(p), p.samples_per_side, p.width, p.height
    r = rows(c)
    out = dict(shape_index=np.full((n, len(pixels)), -1, dtype=np.int32), t=np.full((n, len(pixels)), np.inf),
               point=np.zeros((n, len(pixels), 3)), normal=np.zeros((n, len(pixels), 3)), uv=np.zeros((n, len(pixels), 2)),
               ray_origin=np.zeros((n, len(pixels), 3)), ray_dir=np.zeros((n, len(pixels), 3)))
    desc = flat.desc()
    ray, rec = np.zeros(8), np.zeros(10)
    pr, po = ray.ctypes.data_as(C.POINTER(C.c_double)), rec.ctypes.data_as(C.POINTER(C.c_double))
    for j, (lrow, col) in enumerate(pixels):
        row = r[lrow]
        gpix = row * W + col
        g = None
        for k in range(n):
            up = vp = 0.5
            if sps > 0:
                if p.pcg_mode == Q:
                    if g is None:
                        g = orc.Pcg(p.jitter_state, p.jitter_seq)
                        g.st[0] = hm.pcg_advance(g.state, g.inc, index_of(p, gpix))
                elif p.pcg_mode == S or g is None:
                    g = orc.Pcg(p.path_state, (p.path_seq + index_of(p, gpix, k)) & M64)
                up = (k % sps + g.random_float()) / sps
                vp = (k // sps + g.random_float()) / sps
            L.pto_tracer_fire_ray(C.byref(cam), W, H, col, row, up, vp, pr)
            out["ray_origin"][k, j], out["ray_dir"][k, j] = ray[0:3], ray[3:6]
            if L.pto_world_intersect(C.byref(desc), pr, po):
                out["shape_index"][k, j] = int(rec[9])
                out["t"][k, j], out["point"][k, j], out["normal"][k, j], out["uv"][k, j] = rec[0], rec[1:4], rec[4:7], rec[7:9]
    return out


# ---- the primary rays of these frames (tests/golden/g16_geometry_rays.npz) ------------------------------------------------------
RAY_OFFSETS = [(0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (0.25, 0.875), (0.999999, 1e-9)]


def ray_points() -> List[Tuple[int, int, int, int]]:
    """(col, row, W, H) at which the oracle's primary rays are compared with the reference's: per frame of the catalogue the
    crossing pixel and the one before it, the first and the last pixel of the share, and the frame's own corners."""
    points = set()
    for c in CASES + HIT_CASES:
        W, H = c.case.size
        row, col = c.crossing
        r = rows(c)
        points |= {(col, row, W, H), (col - 1, row, W, H), (0, r[0], W, H), (W - 1, r[-1], W, H), (0, 0, W, H), (W - 1, H - 1, W, H)}
    return sorted(points, key=lambda t: (t[2], t[3], t[1], t[0]))
