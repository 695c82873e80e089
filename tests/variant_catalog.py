"""Every kernel variant the planner can name, and every tuning switch at a value other than its default, as small frames.

csrc/pt_plan.h promises that every kernel a plan can name renders the same image and that no switch of PT_TUNING_TABLE
changes a result.  This catalogue is what holds it to that promise:

* tests/test_variant_catalog.py (CPU) checks that each case plans exactly the kernels listed here, that the names here are
  every name ``pt_plan_kernel_name`` can return and the switches every ``X(...)`` entry of the table (both read from the
  header), and that each frame gives its kernels real work on the oracle;
* tests/test_gpu_variants.py renders each case on the device and compares it with the oracle.

The cases follow ``pt_make_plan``'s rules (shapes 3 / 4, 64 / 65, 127 / 128, 256 / 257, 1023 / 1024 spheres, the LDS budget
of the frame stacks and of the staged scene, jitter, orthogonal cameras, row shares), not trial and error.  Frames are small
enough for the oracle to finish each in a second or two, with widths and heights off the 8 / 16 grid of the tiles.

A plain helper module: no fixtures, no hooks.
"""
from __future__ import annotations

import contextlib
import os
import re
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

from pytracer_amd import abi, flatten, scenes
from pytracer_amd import hostmodel as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = os.path.join(ROOT, "pytracer_amd", "csrc", "pt_plan.h")

PATH, TREE = abi.KERNEL_PATH, abi.KERNEL_PATH_TREE
ON, FL, PT, PL = abi.RENDERER_ONOFF, abi.RENDERER_FLAT, abi.RENDERER_PATHTRACER, abi.RENDERER_POINTLIGHT

# the path tracer's parameter sets: C3's (one ray per bounce) and the CLI's (main.py:95-102: N = 10, D = 3), with seeds
C3 = dict(renderer=PT, samples_per_side=2, num_of_rays=1, max_depth=3, rr_limit=3, path_state=45, path_seq=54)
CLI = dict(C3, samples_per_side=1, num_of_rays=10)
# the one-queue kernel does all the work and hands nothing over / hands every heavy pixel over after a few rays
Q_ONLY = dict(qchoice=2, q_budget=0, q_tail_budget=0, q_few_lanes=0)
Q_HANDOVER = dict(qchoice=2, q_budget=5)

# switches that act when the scene is uploaded (the grid, the ball hierarchy): set before the DeviceScene is created
UPLOAD_SWITCHES = ("grid", "grid_min", "grid_density", "levels_min")
# switches no case sets, with the reason
EXEMPT_SWITCHES = {
    "trace_unit": "records per-unit timings only in -DPT_DEBUG_TIME builds; the shipped library ignores it",
}


@dataclass(frozen=True)
class Case:
    id: str
    world: Tuple               # ("synthetic", n_spheres, with_plane, wide[, dome]), ("rotated", n_spheres) or
                               # ("gallery", n_shapes[, dome]); dome
                               # False: the sky sphere left out (OnOff: a dome around the camera is hit by every ray)
    size: Tuple[int, int]      # (width, height) of the whole frame
    params: Dict               # abi.make_params keywords (renderer included)
    kernels: Tuple[str, str, str, str]  # the plan's (pre_kernel, first_kernel, main_kernel, alt_kernel)
    camera: str = "perspective"         # or "orthogonal"
    tuning: Dict = field(default_factory=dict)
    worker: Optional[int] = None        # cases with an alternative kernel: the kernel that does the work (KERNEL_PATH / _TREE)
    handover: Optional[bool] = None     # ... and whether pixels are handed from the one-queue kernel to the tree kernel
    changes: Tuple[str, ...] = ()       # switch cases: PlanInfo fields the switch changes (beside the kernel names)
    why_not_in_plan: str = ""           # switch cases whose effect the plan does not report: where it acts
    zero: bool = False                  # the memset frame: black, no ray traced
    slow: bool = False


def _t(**kw):
    return kw


CASES = [
    # ---- one lane per pixel, no culling: worlds of fewer than four shapes ---------------------------------------------------
    Case("simple-onoff-hoist", ("gallery", 3, False), (37, 23), dict(renderer=ON), ("", "", "pt_simple_kernel<ONOFF, HOIST>", "")),
    Case("simple-flat-hoist-jitter", ("gallery", 3), (41, 27), dict(renderer=FL, samples_per_side=2, pcg_mode=abi.PCG_SAMPLE),
         ("", "", "pt_simple_kernel<FLAT, HOIST>", "")),
    Case("simple-pointlight-hoist", ("gallery", 3), (43, 29), dict(renderer=PL, samples_per_side=1),
         ("", "", "pt_simple_kernel<POINTLIGHT, HOIST>", "")),
    Case("simple-onoff-ortho", ("gallery", 3, False), (39, 21), dict(renderer=ON), ("", "", "pt_simple_kernel<ONOFF, noHOIST>", ""),
         camera="orthogonal"),
    Case("simple-flat-ortho-jitter", ("gallery", 3), (35, 19), dict(renderer=FL, samples_per_side=2),
         ("", "", "pt_simple_kernel<FLAT, noHOIST>", ""), camera="orthogonal"),
    Case("simple-pointlight-ortho-f32", ("gallery", 3), (45, 25), dict(renderer=PL, out_format=abi.OUT_F32),
         ("", "", "pt_simple_kernel<POINTLIGHT, noHOIST>", ""), camera="orthogonal"),
    # ---- 8x8 tiles with culled shape lists ----------------------------------------------------------------------------------
    Case("tile-onoff-jitter", ("synthetic", 32, True, False, False), (93, 53), dict(renderer=ON, samples_per_side=2),
         ("", "", "pt_tile_kernel<ONOFF>", "")),
    Case("tile-flat-share-rb8", ("synthetic", 32, True, False), (90, 61), dict(renderer=FL, n_ranks=2, rank=1, row_block=8),
         ("", "", "pt_tile_kernel<FLAT>", "")),  # (a share whose row blocks are not multiples of 16: no 16x16 tiles)
    Case("tile-pointlight", ("gallery", 6), (90, 50), dict(renderer=PL, samples_per_side=1, pcg_mode=abi.PCG_SAMPLE),
         ("", "", "pt_tile_kernel<POINTLIGHT>", "")),
    Case("tile-onoff-hier", ("synthetic", 300, True, True, False), (100, 57), dict(renderer=ON),
         ("pt_cell_kernel", "", "pt_tile_kernel<ONOFF, HIER>", "")),
    Case("tile-flat-hier-jitter-share", ("synthetic", 300, True, True), (99, 59),
         dict(renderer=FL, samples_per_side=2, n_ranks=3, rank=2, row_block=8), ("pt_cell_kernel", "", "pt_tile_kernel<FLAT, HIER>", "")),
    Case("tile-pointlight-hier", ("synthetic", 300, True, True), (97, 55), dict(renderer=PL),
         ("pt_cell_kernel", "", "pt_tile_kernel<POINTLIGHT, HIER>", "")),
    Case("tile-onoff-ortho", ("gallery", 6, False), (71, 45), dict(renderer=ON), ("", "", "pt_tile_kernel<ONOFF, ORTHO>", ""),
         camera="orthogonal"),
    Case("tile-flat-ortho-jitter", ("synthetic", 32, True, False), (83, 49), dict(renderer=FL, samples_per_side=1),
         ("", "", "pt_tile_kernel<FLAT, ORTHO>", ""), camera="orthogonal"),
    Case("tile-pointlight-ortho", ("gallery", 6), (73, 43), dict(renderer=PL, samples_per_side=2, pcg_mode=abi.PCG_SAMPLE),
         ("", "", "pt_tile_kernel<POINTLIGHT, ORTHO>", ""), camera="orthogonal"),
    # ---- 16x16 tiles, four pixels per lane ----------------------------------------------------------------------------------
    Case("tile4-onoff-f32", ("synthetic", 32, True, False, False), (100, 57), dict(renderer=ON, out_format=abi.OUT_F32),
         ("", "", "pt_tile4_kernel<ONOFF, noLDS>", "")),
    Case("tile4-flat-lds-share-rb16", ("synthetic", 32, True, False), (77, 45), dict(renderer=FL, n_ranks=2, rank=0, row_block=16),
         ("", "", "pt_tile4_kernel<FLAT, LDS>", "")),
    Case("tile4-flat-nolds", ("synthetic", 100, True, False), (79, 47), dict(renderer=FL),
         ("", "", "pt_tile4_kernel<FLAT, noLDS>", "")),  # (100 x 384 B of records: more than the 24 KB staged)
    # ---- the path tracer ----------------------------------------------------------------------------------------------------
    Case("path-memset", ("synthetic", 32, False, False), (61, 37), dict(C3, max_depth=-1), ("", "", "memset", ""), zero=True),
    Case("path-one-lane", ("synthetic", 32, True, False), (59, 35), dict(C3, samples_per_side=1, pcg_mode=abi.PCG_SAMPLE),
         ("", "", "pt_path_kernel", ""), tuning=_t(cull=0)),  # (otherwise only worlds without shapes: all background)
    Case("regions-lds-scene-lean", ("synthetic", 32, False, False), (93, 53), dict(C3, pcg_mode=abi.PCG_PIXEL),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", "")),
    Case("regions-lds-scene-lean-centre-sample", ("synthetic", 32, True, False), (87, 51),
         dict(C3, samples_per_side=0, pcg_mode=abi.PCG_SAMPLE, out_format=abi.OUT_F32),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", "")),
    Case("regions-ortho", ("synthetic", 32, False, False), (91, 49), dict(C3, samples_per_side=1),
         ("", "pt_tile_kernel<PATHTRACER, ORTHO>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), camera="orthogonal"),
    # >= 128 spheres (ball hierarchy), every other one rotated (fewer scale+translate records staged), a frame stack of two
    # depths: the 129 records still fit half the LDS behind it
    Case("regions-lds-scene", ("rotated", 128), (101, 57), dict(C3, max_depth=2, samples_per_side=1),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_regions_kernel<LDS, SCENE>", "")),
    Case("regions-lds-nogrid-blocks", ("synthetic", 255, True, True), (103, 59), dict(C3, samples_per_side=1, pcg_mode=abi.PCG_SAMPLE),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_regions_kernel<LDS, NOGRID>", "")),
    Case("regions-lds-grid-hier", ("synthetic", 1100, True, True), (95, 53), dict(C3, samples_per_side=1, max_depth=2),
         ("pt_cell_kernel", "pt_tile_kernel<PATHTRACER, HIER>", "pt_path_regions_kernel<LDS>", "")),
    Case("regions-hbm-deep", ("synthetic", 32, True, False), (63, 35), dict(C3, samples_per_side=1, max_depth=14, rr_limit=1),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<HBM>", "")),  # (14 x 6 x 256 x 8 B: more than the LDS)
    # ---- num_of_rays > 1: the tree kernel, and the one-queue kernel in front of it ------------------------------------------
    Case("tree-lean-scene", ("synthetic", 32, False, False), (93, 53), dict(CLI),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>"),
         worker=TREE, handover=False),
    Case("tree-lean-scene-share-rb5", ("synthetic", 32, True, False), (89, 47), dict(CLI, num_of_rays=4, n_ranks=3, rank=1, row_block=5),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>"),
         worker=TREE, handover=False),
    # a node stack of 100 depths (64 KB): no room left for the scene's records (N = 2 without roulette dies out on its own)
    Case("tree-lean-deep", ("synthetic", 32, True, False), (67, 37), dict(CLI, num_of_rays=2, max_depth=100, rr_limit=0),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN>", "pt_path_flagged_kernel<LEAN, SPLIT>"),
         worker=TREE, handover=False),
    Case("tree-balls", ("synthetic", 128, False, False), (91, 53), dict(CLI, pcg_mode=abi.PCG_SAMPLE),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_tree_kernel", "pt_path_flagged_kernel<LDS>"),
         worker=TREE, handover=False),
    Case("flagged-lean-lds-queue", ("synthetic", 32, True, False), (83, 47), dict(CLI),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>"),
         tuning=Q_ONLY, worker=PATH, handover=False),
    Case("flagged-lean-lds-handover", ("synthetic", 32, True, False), (85, 45), dict(CLI, samples_per_side=2, num_of_rays=3, pcg_mode=abi.PCG_SAMPLE),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>"),
         tuning=Q_HANDOVER, worker=PATH, handover=True),
    Case("flagged-lds-queue", ("synthetic", 128, False, False), (87, 49), dict(CLI, samples_per_side=0),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_tree_kernel", "pt_path_flagged_kernel<LDS>"),
         tuning=Q_ONLY, worker=PATH, handover=False),
    Case("flagged-lds-handover", ("synthetic", 128, False, False), (89, 51), dict(CLI),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_tree_kernel", "pt_path_flagged_kernel<LDS>"),
         tuning=Q_HANDOVER, worker=PATH, handover=True),
    Case("flagged-lean-split-queue", ("synthetic", 32, True, False), (81, 47), dict(CLI, num_of_rays=3, max_depth=5, rr_limit=2),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, SPLIT>"),
         tuning=Q_ONLY, worker=PATH, handover=False),
    Case("flagged-lean-split-handover", ("synthetic", 32, True, False), (79, 45),
         dict(CLI, num_of_rays=3, max_depth=5, rr_limit=2, pcg_mode=abi.PCG_SAMPLE),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, SPLIT>"),
         tuning=Q_HANDOVER, worker=PATH, handover=True),
    Case("flagged-split-queue", ("synthetic", 128, False, False), (85, 49), dict(CLI, num_of_rays=3, max_depth=5, rr_limit=2),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_tree_kernel", "pt_path_flagged_kernel<SPLIT>"),
         tuning=Q_ONLY, worker=PATH, handover=False),
    Case("flagged-split-handover", ("synthetic", 128, False, False), (83, 51), dict(CLI, num_of_rays=3, max_depth=5, rr_limit=2),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_tree_kernel", "pt_path_flagged_kernel<SPLIT>"),
         tuning=Q_HANDOVER, worker=PATH, handover=True),
    # ---- every switch of PT_TUNING_TABLE at a value other than its default (id: sw-<switch>-...) ---------------------------
    Case("sw-cull-0-flat", ("synthetic", 32, True, False), (75, 43), dict(renderer=FL), ("", "", "pt_simple_kernel<FLAT, HOIST>", ""),
         tuning=_t(cull=0)),
    Case("sw-cull-0-path", ("synthetic", 32, True, False), (61, 37), dict(C3), ("", "", "pt_path_kernel", ""), tuning=_t(cull=0)),
    Case("sw-levels_min-no-balls", ("synthetic", 200, False, False), (93, 51), dict(C3, samples_per_side=1, max_depth=2),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_regions_kernel<LDS, NOGRID>", ""),
         tuning=_t(levels_min=100000), changes=("ball_levels",)),
    Case("sw-path_wg_per_cu-1", ("synthetic", 32, False, False), (331, 201), dict(C3, samples_per_side=1),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""),
         tuning=_t(path_wg_per_cu=1), changes=("grid",)),  # (1 092 regions: more waves than one workgroup per CU holds)
    Case("sw-lds_frames-0", ("synthetic", 32, True, False), (71, 41), dict(C3, pcg_mode=abi.PCG_SAMPLE),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<HBM>", ""), tuning=_t(lds_frames=0)),
    Case("sw-tree-0", ("synthetic", 32, False, False), (79, 45), dict(CLI, num_of_rays=4),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, NOGRID>", ""), tuning=_t(tree=0)),  # (frames of 20 doubles: no room for the scene)
    Case("sw-tree_max_pixels-small", ("synthetic", 32, False, False), (77, 43), dict(CLI, num_of_rays=4),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, NOGRID>", ""), tuning=_t(tree_max_pixels=1000)),
    Case("sw-scene_lds-0", ("synthetic", 32, False, False), (81, 47), dict(C3),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, NOGRID>", ""), tuning=_t(scene_lds=0)),
    Case("sw-tile_wg_per_cu-1", ("synthetic", 32, True, False), (331, 247), dict(renderer=FL, samples_per_side=1),
         ("", "", "pt_tile_kernel<FLAT>", ""), tuning=_t(tile_wg_per_cu=1), changes=("grid",)),
    Case("sw-tile4-0", ("synthetic", 32, True, False), (95, 53), dict(renderer=FL), ("", "", "pt_tile_kernel<FLAT>", ""),
         tuning=_t(tile4=0)),
    Case("sw-tile4_lds-0", ("synthetic", 32, True, False), (93, 51), dict(renderer=FL), ("", "", "pt_tile4_kernel<FLAT, noLDS>", ""),
         tuning=_t(tile4_lds=0)),
    Case("sw-qchoice-0", ("synthetic", 32, True, False), (75, 41), dict(CLI),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", ""), tuning=_t(qchoice=0)),
    Case("sw-qchoice-2", ("synthetic", 32, True, False), (77, 39), dict(CLI, num_of_rays=2, max_depth=4, pcg_mode=abi.PCG_SAMPLE),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, SPLIT>"),
         tuning=_t(qchoice=2), worker=PATH, changes=("q_min_flagged",)),
    Case("sw-q_wg_per_cu-1", ("synthetic", 32, True, False), (331, 201), dict(CLI, num_of_rays=3, max_depth=5, rr_limit=2),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, SPLIT>"),
         tuning=dict(Q_HANDOVER, q_wg_per_cu=1), worker=PATH, handover=True, changes=("grid_alt",)),
    Case("sw-q_frames_home-2", ("synthetic", 32, True, False), (79, 43), dict(CLI),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, SPLIT>"),
         tuning=dict(Q_ONLY, q_frames_home=2), worker=PATH, handover=False),
    Case("sw-q_min_flagged-1", ("synthetic", 32, True, False), (81, 41), dict(CLI, num_of_rays=5, samples_per_side=0),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>"),
         tuning=_t(q_min_flagged=1), worker=PATH, changes=("q_min_flagged",)),
    Case("sw-q_budget-1", ("synthetic", 128, False, False), (75, 45), dict(CLI, num_of_rays=4, samples_per_side=2),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_tree_kernel", "pt_path_flagged_kernel<LDS>"),
         tuning=_t(qchoice=2, q_budget=1, q_tail_budget=0, q_few_lanes=0), worker=PATH, handover=True, changes=("alt_budget",)),
    Case("sw-q_tail_budget-2", ("synthetic", 32, True, False), (87, 43), dict(CLI, num_of_rays=3, samples_per_side=2),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>"),
         tuning=_t(qchoice=2, q_budget=0, q_tail_budget=2, q_few_lanes=0), worker=PATH, handover=True,
         why_not_in_plan="the one-queue kernel's queue block (not reported by the plan info)"),
    Case("sw-q_few_lanes-64", ("synthetic", 32, True, False), (85, 47), dict(CLI, num_of_rays=3, max_depth=4),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, SPLIT>"),
         tuning=_t(qchoice=2, q_budget=0, q_tail_budget=0, q_few_lanes=64), worker=PATH, handover=True,
         why_not_in_plan="the one-queue kernel's queue block (not reported by the plan info)"),
    Case("sw-p_maxpath-s_min-regions", ("synthetic", 32, True, False), (83, 45), dict(C3, pcg_mode=abi.PCG_PIXEL),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(p_maxpath=24, s_min=8),
         why_not_in_plan="the second pass's step batching (kernel arguments, not reported by the plan info)"),
    Case("sw-p_maxpath-s_min-one-lane", ("synthetic", 32, True, False), (67, 39), dict(C3, pcg_mode=abi.PCG_SAMPLE),
         ("", "", "pt_path_kernel", ""), tuning=_t(cull=0, p_maxpath=5, s_min=3),
         why_not_in_plan="pt_path_kernel's step batching (kernel arguments, not reported by the plan info)"),
    Case("sw-unit_lanes_cap-0", ("synthetic", 32, True, False), (89, 49), dict(C3),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(unit_lanes_cap=0),
         changes=("units_need",)),
    Case("sw-unit_lanes_cap-100", ("synthetic", 32, True, False), (91, 47), dict(C3, pcg_mode=abi.PCG_SAMPLE),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(unit_lanes_cap=100),
         changes=("units_need",)),
    Case("sw-unit_min_rounds-1", ("synthetic", 32, True, False), (87, 49), dict(C3, samples_per_side=3),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(unit_min_rounds=1),
         changes=("min_rounds",)),
    Case("sw-unit_min_rounds-5-sample", ("synthetic", 32, True, False), (85, 51), dict(C3, samples_per_side=3, pcg_mode=abi.PCG_SAMPLE),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(unit_min_rounds=5),
         changes=("min_rounds",)),
    Case("sw-spec_draws-0", ("synthetic", 32, True, False), (83, 53), dict(C3),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(spec_draws=0),
         changes=("spec_draws",)),
    Case("sw-spec_draws-9", ("synthetic", 32, True, False), (81, 51), dict(C3, samples_per_side=0),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(spec_draws=9),
         changes=("spec_draws",)),
    Case("sw-tree_scene_lds-0", ("synthetic", 32, False, False), (89, 45), dict(CLI),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN>", "pt_path_flagged_kernel<LEAN, LDS>"),
         tuning=_t(tree_scene_lds=0), worker=TREE, handover=False),
    Case("sw-tree_jump-0", ("synthetic", 32, False, False), (87, 47), dict(CLI, num_of_rays=6, samples_per_side=2),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>"),
         tuning=_t(tree_jump=0), worker=TREE, handover=False, changes=("lds_main",)),
    Case("sw-pixel_dome-0", ("synthetic", 32, False, False), (95, 49), dict(C3),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(pixel_dome=0),
         why_not_in_plan="the first pass's per-pixel dome classification (a launch argument, not reported by the plan info)"),
    Case("sw-hier_min-16-flat", ("synthetic", 32, True, False), (93, 55), dict(renderer=FL, samples_per_side=2),
         ("pt_cell_kernel", "", "pt_tile_kernel<FLAT, HIER>", ""), tuning=_t(hier_min=16)),
    Case("sw-hier_min-16-path", ("synthetic", 32, True, False), (91, 53), dict(C3),
         ("pt_cell_kernel", "pt_tile_kernel<PATHTRACER, HIER>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", ""), tuning=_t(hier_min=16)),
    Case("sw-hier_min-never", ("synthetic", 300, True, True), (101, 55), dict(renderer=FL),
         ("", "", "pt_tile_kernel<FLAT>", ""), tuning=_t(hier_min=-1)),
    Case("sw-block_h-1", ("synthetic", 128, False, False), (99, 57), dict(C3, max_depth=1),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE>", ""), tuning=_t(block_h=1), changes=("block_h",)),
    Case("sw-block_h-4", ("synthetic", 255, True, True), (97, 61), dict(C3, samples_per_side=1),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_regions_kernel<LDS, NOGRID>", ""), tuning=_t(block_h=4), changes=("block_h",)),
    Case("sw-small_query-0-regions", ("synthetic", 32, False, False), (89, 53), dict(C3),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_regions_kernel<LDS, SCENE>", ""), tuning=_t(small_query=0)),
    Case("sw-small_query-0-tree", ("synthetic", 32, False, False), (87, 51), dict(CLI),
         ("", "pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel", "pt_path_flagged_kernel<LDS>"),
         tuning=_t(small_query=0), worker=TREE, handover=False),
    Case("sw-small_query-0-regions-lds", ("synthetic", 255, True, True), (95, 59), dict(C3, samples_per_side=1),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_regions_kernel<LDS>", ""), tuning=_t(small_query=0)),
    Case("sw-grid-0", ("synthetic", 1100, True, True), (93, 51), dict(C3, samples_per_side=1, max_depth=2),
         ("pt_cell_kernel", "pt_tile_kernel<PATHTRACER, HIER>", "pt_path_regions_kernel<LDS, NOGRID>", ""), tuning=_t(grid=0),
         changes=("has_grid",)),
    Case("sw-grid_min-100", ("synthetic", 200, True, True), (97, 53), dict(C3, samples_per_side=1, max_depth=2),
         ("", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_path_regions_kernel<LDS>", ""), tuning=_t(grid_min=100), changes=("has_grid",)),
    Case("sw-grid_density-1", ("synthetic", 1100, True, True), (91, 49), dict(C3, samples_per_side=1, max_depth=2),
         ("pt_cell_kernel", "pt_tile_kernel<PATHTRACER, HIER>", "pt_path_regions_kernel<LDS>", ""), tuning=_t(grid_density=1),
         why_not_in_plan="the uniform grid's cell count at upload (not reported by the plan info)"),
    Case("sw-grid_density-20-pointlight", ("synthetic", 1100, True, True), (89, 47), dict(renderer=PL, samples_per_side=1),
         ("pt_cell_kernel", "", "pt_tile_kernel<POINTLIGHT, HIER>", ""), tuning=_t(grid_density=20),
         why_not_in_plan="the uniform grid's cell count at upload (not reported by the plan info)"),
]

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"


# ---- scenes, cameras, parameters --------------------------------------------------------------------------------------------
def _gallery(n_shapes: int, dome: bool = True) -> hm.World:
    """A hand-built world: a dome around the camera, a checkered ground, a textured mirror, a diffuse sphere with a texture,
    an emitting checkered sphere, a mirror, a small diffuse sphere -- the first ``n_shapes`` of them (the dome left out if ``dome`` is False) -- and
    two point lights."""
    tex = hm.HdrImage(8, 4)
    tex.array[...] = [[[0.1 + 0.1 * x, 0.9 - 0.2 * y, 0.3 + 0.05 * (x + y)] for x in range(8)] for y in range(4)]
    w = hm.World()
    w.add_light(hm.PointLight(hm.Vec(-2.0, 4.0, 6.0), hm.Color(1.0, 0.9, 0.8), 0.0))
    w.add_light(hm.PointLight(hm.Vec(3.0, -5.0, 3.0), hm.Color(0.3, 0.4, 0.9), 0.5))
    shapes = [
        hm.Sphere(hm.scaling(hm.Vec(40.0, 40.0, 40.0)),
                  hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.BLACK)), hm.UniformPigment(hm.Color(0.6, 0.5, 0.9)))),
        hm.Plane(hm.Transformation(), hm.Material(hm.DiffuseBRDF(hm.CheckeredPigment(hm.Color(0.3, 0.5, 0.1), hm.Color(0.1, 0.2, 0.5), 4)))),
        hm.Sphere(hm.translation(hm.Vec(3.0, 0.0, 1.0)) * hm.rotation_z(30.0),
                  hm.Material(hm.SpecularBRDF(hm.ImagePigment(tex)), hm.UniformPigment(hm.BLACK))),
        hm.Sphere(hm.translation(hm.Vec(2.0, -1.6, 0.5)) * hm.scaling(hm.Vec(0.5, 0.5, 0.5)),
                  hm.Material(hm.DiffuseBRDF(hm.ImagePigment(tex)), hm.UniformPigment(hm.BLACK))),
        hm.Sphere(hm.translation(hm.Vec(2.5, 1.7, 0.6)) * hm.scaling(hm.Vec(0.6, 0.4, 0.6)),
                  hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(0.8, 0.3, 0.2))),
                              hm.CheckeredPigment(hm.BLACK, hm.Color(0.4, 0.3, 0.1), 3))),
        hm.Sphere(hm.translation(hm.Vec(4.5, 0.8, 2.2)) * hm.scaling(hm.Vec(0.7, 0.7, 0.7)),
                  hm.Material(hm.SpecularBRDF(hm.UniformPigment(hm.Color(0.7, 0.7, 0.6))), hm.UniformPigment(hm.BLACK))),
        hm.Sphere(hm.translation(hm.Vec(1.5, 0.3, 0.25)) * hm.scaling(hm.Vec(0.25, 0.25, 0.25)),
                  hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(0.2, 0.6, 0.9))), hm.UniformPigment(hm.BLACK))),
    ]
    if not dome:
        shapes = shapes[1:]
    assert n_shapes <= len(shapes)
    for s in shapes[:n_shapes]:
        w.add_shape(s)
    return w


_scenes: Dict[Tuple, abi.FlatScene] = {}


def scene(case: Case) -> abi.FlatScene:
    key = case.world
    if key not in _scenes:
        if key[0] == "synthetic":
            world = scenes.synthetic_world(key[1], with_plane=key[2], wide=key[3])
            if len(key) > 4 and not key[4]:
                world.shapes = world.shapes[1:]  # (the sky sphere is the first shape)
        elif key[0] == "rotated":  # (the synthetic world with its plane, every other sphere turned about z)
            world = scenes.synthetic_world(key[1], with_plane=True)
            for i in range(2, key[1], 2):
                world.shapes[i].transformation = world.shapes[i].transformation * hm.rotation_z(20.0)
        else:
            world = _gallery(*key[1:])
        _scenes[key] = flatten.flatten_world(world)
    return _scenes[key]


def camera(case: Case) -> abi.Camera:
    w, h = case.size
    if case.camera == "orthogonal":
        return flatten.flatten_camera(hm.OrthogonalCamera(w / h, hm.translation(hm.Vec(-1.0, 0.0, 1.5)) * hm.scaling(hm.Vec(1.0, 5.0, 3.0))))
    return flatten.flatten_camera(scenes.synthetic_camera(w, h))


def params(case: Case) -> abi.Params:
    kw = dict(case.params)
    return abi.make_params(case.size[0], case.size[1], kw.pop("renderer"), **kw)


def rows(case: Case):
    """The frame's rows this case renders (all of them, or a rank's share)."""
    p = params(case)
    return abi.rows_for_rank(p.height, p.row_block, p.n_ranks, p.rank)


@contextlib.contextmanager
def tuned(case: Case):
    """Every switch at its default from the header, the case's own on top, for the duration of the block; then the values
    they had (the table is process-wide: whatever the environment or an earlier test left in it does not reach the case)."""
    from pytracer_amd import device

    values = dict(tuning_defaults(), **case.tuning)
    saved = {name: device.get_tuning(name) for name in values}
    try:
        for name, value in values.items():
            device.set_tuning(name, value)
        yield
    finally:
        for name, value in saved.items():
            device.set_tuning(name, value)


def plan(case: Case) -> abi.PlanInfo:
    from pytracer_amd import device

    with tuned(case):
        return device.plan(scene(case), camera(case), params(case))


def plan_names(info: abi.PlanInfo) -> Tuple[str, str, str, str]:
    return (info.pre_kernel, info.first_kernel, info.main_kernel, info.alt_kernel)


def switches(case: Case):
    """The table's switches a case sets to a value other than its default (the hand-over cases' zeros included)."""
    return set(case.tuning)


# ---- what the planner can name, read from the header --------------------------------------------------------------------------
def _header() -> str:
    with open(PLAN_H) as f:
        return f.read()


def _string_table(src: str, name: str):
    m = re.search(r"static const char \*" + name + r"\[\d+\]\s*=\s*\{(.*?)\};", src, re.S)
    assert m, f"pt_plan_kernel_name: table {name} not found"
    return re.findall(r'"([^"]*)"', m.group(1))


def plannable_names() -> set:
    """Every name ``pt_plan_kernel_name`` can return, from its string tables and formats, restricted by the rules of
    ``pt_make_plan`` that the names alone do not show (spelled out below).  A format or table the function gains that is
    not understood here fails loudly."""
    src = _header()
    body = src[src.index("pt_plan_kernel_name("):]
    R, TM = _string_table(body, "R"), _string_table(body, "TM")
    S2, A = _string_table(body, "S2"), _string_table(body, "A")
    formats = re.findall(r'snprintf\(buf, n, "([^"]*)"', body)
    known = {"pt_cell_kernel", "pt_tile_kernel<PATHTRACER%s>", "memset", "pt_tile4_kernel<%s, %s>", "%s",
             "pt_tile_kernel<%s%s>", "pt_path_kernel", "pt_simple_kernel<%s, %s>"}
    assert set(formats) == known, f"pt_plan_kernel_name's formats changed: {sorted(set(formats) ^ known)}"
    names = {"pt_cell_kernel", "memset", "pt_path_kernel"}
    names |= {f"pt_tile_kernel<PATHTRACER{tm}>" for tm in TM}
    # 16x16 tiles: OnOff / Flat only; the records are staged for Flat only (pt_plan.h: pl.t4lds)
    names |= {f"pt_tile4_kernel<{r}, {lds}>" for r in R if r in ("ONOFF", "FLAT") for lds in ("LDS", "noLDS")
              if not (r == "ONOFF" and lds == "LDS")}
    names |= {s for s in S2 + A if s}
    # 8x8 tiles of the primary-ray renderers: BLOCKS is the path tracer's first pass only
    names |= {f"pt_tile_kernel<{r}{tm}>" for r in R if r != "PATHTRACER" for tm in TM if tm != ", BLOCKS"}
    # one lane per pixel: the path tracer's is pt_path_kernel
    names |= {f"pt_simple_kernel<{r}, {h}>" for r in R if r != "PATHTRACER" for h in ("HOIST", "noHOIST")}
    return names


def tuning_defaults() -> Dict[str, int]:
    """The ``X(...)`` entries of PT_TUNING_TABLE with their defaults, plus the grid density the table's struct carries beside
    them (cells per sphere)."""
    src = _header()
    m = re.search(r"#define PT_TUNING_TABLE\(X\)(.*?)\nstruct PtTuning", src, re.S)
    assert m, "PT_TUNING_TABLE not found"
    table = {name: int(v) for name, v in re.findall(r"\bX\((\w+),\s*\"PTRACE_\w+\",\s*(-?\d+)\)", m.group(1))}
    d = re.search(r"double grid_density = (\d+)\.0;", src)
    assert d, "grid_density left PtTuning"
    table["grid_density"] = int(d.group(1))
    return table


def tuning_switches() -> set:
    return set(tuning_defaults())


def catalogue_names() -> set:
    """The names the variant cases plan (the switch cases, ``sw-*``, are not counted: each name has a case of its own)."""
    return {n for c in CASES if not c.id.startswith("sw-") for n in c.kernels if n}
