"""csrc/pt_frame_args.h on its own, on the CPU: what a frame hands its kernels, as far as it is made of host values.

tests/frame_args/frame_args_probe.cpp (a program with its own main, no HIP call) builds scene descriptions, runs
pt_build_scene, pt_scene_facts, the planner and the functions launch() fills its argument block with, and prints every
non-pointer field of the block -- and of the one-queue kernel's block where the plan has one.  Nothing here is compared with a
recorded dump: every expectation is computed below from the documented formulas (camera.py:116-124 and 59-78 for the cone
model, the PCG mode mapping and the partition defaults of include/ptrace.h, the dome rule |o'|^2 - 1 < -0.5, "copied from the
plan" against the plan the same program printed and against pt_debug_plan for the same inputs).  The second build runs the
program under the host AddressSanitizer and UndefinedBehaviorSanitizer (the stand-alone program only: nothing is loaded into
Python)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi, build, device, flatten
from pytracer_amd import hostmodel as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "frame_args", "frame_args_probe.cpp")
# host code only (the headers define no kernel); the library's own floating-point flags
FLAGS = ["-x", "hip", "--offload-host-only", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Werror"]
BUILDS = {"plain": ["-O3"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
MOVED = [0.6, -0.8, 0, 1.5, 0.8, 0.6, 0, -2.0, 0, 0, 1, 0.25]  # rotation about z by the 3-4-5 angle behind a translation
PERSPECTIVE, ORTHOGONAL = abi.CAMERA_PERSPECTIVE, abi.CAMERA_ORTHOGONAL


@pytest.fixture(scope="module", params=list(BUILDS))
def blocks(request, tmp_path_factory):
    """{case: {key: value as printed}} from one build of the program (each build is compiled and run once per module)."""
    exe = str(tmp_path_factory.mktemp("frame_args") / ("probe_" + request.param))
    r = subprocess.run([build._hipcc()] + FLAGS + BUILDS[request.param] + ["-o", exe, SOURCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    out = {}
    for line in r.stdout.splitlines():
        case, key, value = line.split(" ", 2)
        assert key not in out.setdefault(case, {}), (case, key)
        out[case][key] = value
    return out


def f32(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", np.float32(x)))[0]


def f64(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def vec(block, key, n=3):
    return [block["%s[%d]" % (key, k)] for k in range(n)]


def ints(block, *keys):
    return tuple(int(block[k]) for k in keys)


# ---- the cone model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, m, kind", [("cone_identity_persp", IDENTITY, PERSPECTIVE), ("cone_identity_ortho", IDENTITY, ORTHOGONAL),
                                           ("cone_moved_persp", MOVED, PERSPECTIVE), ("cone_moved_ortho", MOVED, ORTHOGONAL)])
def test_the_cone_model_is_the_cameras_ray_as_an_affine_function_of_the_pixel(blocks, name, m, kind):
    """camera.py:116-124: a perspective ray starts at (-d, 0, 0) towards (d, (1 - 2u) a, 2v - 1); camera.py:59-78: an orthogonal
    one starts at (-1, (1 - 2u) a, 2v - 1) towards (1, 0, 0); imagetracer.py:56-58: u = x / W, v = 1 - y / H.  Through the camera's
    transformation, in double, rounded to fp32 once."""
    b, W, H, d, a = blocks[name], 4, 2, 1.5, 2.0
    row = [m[0:4], m[4:8], m[8:12]]
    assert ints(b, "cam_kind", "W", "H") == (kind, W, H)
    assert vec(b, "cam_m", 12) == [f64(x) for x in m] and b["cam_dist[0]"] == f64(d) and b["cam_aspect[0]"] == f64(a)
    assert vec(b, "cone_dx") == [f32(r[1] * (-2.0 * a / W)) for r in row]
    assert vec(b, "cone_dy") == [f32(r[2] * (-2.0 / H)) for r in row]
    if kind == PERSPECTIVE:  # directions at pixel (0, 0), the common origin
        assert vec(b, "cone_d0") == [f32(r[0] * d + r[1] * a + r[2]) for r in row]
        assert vec(b, "cone_apex") == [f32(r[0] * -d + r[3]) for r in row]
    else:  # origins at pixel (0, 0), the common direction
        assert vec(b, "cone_d0") == [f32(-r[0] + r[1] * a + r[2] + r[3]) for r in row]
        assert vec(b, "cone_apex") == [f32(r[0]) for r in row]
    # the origin pt_prep_hoist gets: (-d, 0, 0) through the transformation with every product kept, zeros included
    assert vec(b, "hoist_origin") == [f64(-d * r[0] + 0.0 * r[1] + 0.0 * r[2] + r[3]) for r in row]


# ---- pt_params ----------------------------------------------------------------------------------------------------------------
def test_the_generators_mode_and_the_stream_it_names(blocks):
    """PT_PCG_SEQ draws nothing at pixel centres (it is PT_PCG_PIXEL on the path stream) and walks the jitter stream otherwise;
    the device's own alignments pass through.  The probe's seeds: jitter (42, 54), path (45, 59)."""
    assert ints(blocks["pcg_seq_centre"], "pcg_mode", "s0", "q0", "S") == (abi.PCG_PIXEL, 45, 59, 0)
    assert ints(blocks["pcg_seq_jitter"], "pcg_mode", "s0", "q0", "S") == (abi.PCG_SEQ, 42, 54, 2)
    assert ints(blocks["pcg_pixel"], "pcg_mode", "s0", "q0", "S") == (abi.PCG_PIXEL, 45, 59, 2)
    assert ints(blocks["pcg_sample"], "pcg_mode", "s0", "q0", "S") == (abi.PCG_SAMPLE, 45, 59, 2)


def test_partition_defaults_output_format_and_colours(blocks):
    d, p = blocks["defaults_f32"], blocks["partition_f64"]
    assert ints(d, "row_block", "n_ranks", "rank", "out_f32", "rows_local", "npix") == (1, 1, 0, 1, 2, 8)  # (row_block = n_ranks = 0 asked for)
    # 16 rows in blocks of 2, rank 1 of 3 has blocks 1, 4 and 7
    assert ints(p, "row_block", "n_ranks", "rank", "out_f32", "rows_local", "npix") == (2, 3, 1, 0, 6, 24)
    assert int(p["rows_local"]) == len(abi.rows_for_rank(16, 2, 3, 1))
    for b in (d, p):
        assert ints(b, "W", "N", "D", "rr") == (4, 1, 3, 3)
        assert vec(b, "bg") == [f64(x) for x in (0.125, 0.25, 0.5)] and vec(b, "onoff") == [f64(x) for x in (1.0, 0.75, 0.5)]
        assert vec(b, "ambient") == [f64(x) for x in (0.0625, 0.03125, 0.015625)]


# ---- the dome candidate -------------------------------------------------------------------------------------------------------
NESTED = [(0.5, 3.0, True), (4.0, 0.0, True), (10.0, -1.0, True), (20.0, -1.0, False)]  # (radius, centre x, uniform pigment)


def deepest(block, spheres, d=1.0, m=IDENTITY):
    """The slot of the candidate with the most negative |o'|^2 - 1 below -0.5, o' = invm (camera origin), or -1; the camera's
    origin as the dome rule spells it (-d m0 + m3).  Candidates: the spheres of uniform pigments, by slot."""
    slot_of = {int(k[len("dome_cand["):-1]): int(v) for k, v in block.items() if k.startswith("dome_cand[")}
    assert sorted(slot_of) == [i for i, s in enumerate(spheres) if s[2]]
    o = [-d * m[0] + m[3], -d * m[4] + m[7], -d * m[8] + m[11]]
    best, slot = -0.5, -1
    for index in sorted(slot_of, key=slot_of.get):
        r, cx, _ = spheres[index]
        inv = [1.0 / r, 0.0, 0.0, -cx / r, 0.0, 1.0 / r, 0.0, -0.0 / r, 0.0, 0.0, 1.0 / r, -0.0 / r]
        q = [o[0] * inv[4 * k] + o[1] * inv[4 * k + 1] + o[2] * inv[4 * k + 2] + inv[4 * k + 3] for k in range(3)]
        c = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] - 1.0
        if c < best:
            best, slot = c, slot_of[index]
    return slot, best


def test_the_dome_is_the_sphere_the_camera_is_deepest_inside(blocks):
    b = blocks["dome_nested"]
    assert ints(b, "plan.path_tiled", "plan.ortho") == (1, 0)  # (a path-tracer frame with a tiled first pass)
    slot, c = deepest(b, NESTED)
    assert c == -1.0 and slot >= 0 and int(b["dome_slot"]) == slot  # shape 2, around the camera's origin (shape 1: -0.9375)
    assert int(b["dome_shortcut"]) == 1


def test_no_dome_without_depth_perspective_switch_or_candidates(blocks):
    shallow = [(0.5, 3.0, True), (1.0, -0.225, True)]
    slot, c = deepest(blocks["dome_shallow"], shallow)
    assert slot == -1 and c == -0.5 and abs((-1.0 + 0.225) ** 2 - 1.0 + 0.4) < 1e-3  # inside by -0.399 only
    assert ints(blocks["dome_shallow"], "dome_slot", "plan.path_tiled") == (-1, 1)
    assert ints(blocks["dome_ortho"], "dome_slot", "plan.path_tiled", "plan.ortho") == (-1, 1, 1)
    assert ints(blocks["dome_switched_off"], "dome_slot", "plan.path_tiled", "plan.ortho") == (-1, 1, 0)
    none = blocks["dome_no_candidates"]
    assert not [k for k in none if k.startswith("dome_cand[")] and ints(none, "dome_slot", "plan.path_tiled") == (-1, 1)


# ---- what the plan decided, copied ---------------------------------------------------------------------------------------------
ALWAYS = ["rows", "npass", "npix", "bs_levels", "frame_doubles", "diag_lds", "grid_occ_lds", "scene_lds", "nthreads", "block_h"]


def test_every_block_carries_its_plans_fields(blocks):
    """rows_local .. block_h always; the step batching of path-tracer frames; the second pass's fields of tiled path-tracer
    frames (the hand-over table only beside the one-queue kernel, whose budgets its own block carries); the cell table's shape
    where cells are culled.  Everything else stays zero."""
    for name, b in blocks.items():
        plan = {k[len("plan."):]: int(v) for k, v in b.items() if k.startswith("plan.")}
        pathtracer = name.startswith(("dome_", "plan_tree", "plan_zero"))
        want = {k: plan[k] for k in ALWAYS}
        want["rows_local"] = want.pop("rows")
        for k in ("p_max_path", "s_min_path"):
            want[k] = plan[k] if pathtracer else 0
        for k in ("spec_draws", "tree_jump_lds"):
            want[k] = plan[k] if plan["path_tiled"] else 0
        want["handover_cap"] = plan["handover_cap"] if plan["q_alt"] else 0
        for k in ("cells_x", "cell_stride"):
            want[k] = plan[k] if plan["hier"] else 0
        want.update(q_budget=0, q_tail_budget=0, q_few_lanes=0, dbg_trace_unit=0, count_base=0, qpar=0)
        if not plan["path_tiled"]:
            want["dome_slot"] = 0
        assert {k: int(b[k]) for k in want} == want, name
        assert ints(b, "n_shapes", "n_spheres", "n_diag", "bs_levels") == ints(b, "facts.n_shapes", "facts.n_spheres", "facts.n_diag", "plan.bs_levels")
    assert ints(blocks["plan_hier_flat"], "plan.hier", "cells_x", "cell_stride") == (1, 10, 320)  # 320 px / 32, 257 shapes in 64s
    assert ints(blocks["plan_hits"], "plan.tile4", "plan.kernel") == (0, abi.KERNEL_HITS)
    assert ints(blocks["plan_zero_frame"], "D", "plan.npix") == (-1, 1280 * 720) and ints(blocks["plan_no_rows"], "npix", "rows_local") == (0, 0)


def spheres_world(n, with_plane):
    """The probe's row_of_spheres: what the plan reads of it are the counts."""
    w = hm.World()
    for k in range(n):
        w.add_shape(hm.Sphere(hm.translation(hm.Vec(3.0 + 0.01 * k, -8.0 + 0.5 * k, 0.25)) * hm.scaling(hm.Vec(0.4, 0.4, 0.4))))
    if with_plane:
        w.add_shape(hm.Plane(hm.translation(hm.Vec(0.0, 0.0, -1.0))))
    return flatten.flatten_world(w)


def reported_plan(n, with_plane, **kw):
    camera = flatten.flatten_camera(hm.PerspectiveCamera(1.0, 1280 / 720, hm.Transformation()))
    return device.plan(spheres_world(n, with_plane), camera, abi.make_params(1280, 720, **kw), n_cu=256, dome_shortcut=True)


def same_inputs(b, p):
    assert ints(b, "facts.n_spheres", "facts.n_diag", "facts.has_grid", "facts.bs_levels") == (p.n_spheres, p.n_diag, p.has_grid, 0)


def test_the_tree_frame_and_its_one_queue_block_against_pt_debug_plan(blocks):
    b = blocks["plan_tree_q_alt"]
    p = reported_plan(32, False, renderer=abi.RENDERER_PATHTRACER, samples_per_side=1, num_of_rays=10, max_depth=3, rr_limit=3, path_state=45, path_seq=59)
    same_inputs(b, p)
    assert p.kernels == ["pt_tile_kernel<PATHTRACER>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>"]  # (test_plan.py's CLI case)
    assert ints(b, "rows_local", "npix", "frame_doubles", "block_h", "spec_draws", "bs_levels") == (p.rows, p.npix, p.frame_doubles, p.block_h, p.spec_draws, p.ball_levels)
    assert ints(b, "nthreads", "aq.nthreads", "aq.count_base", "aq.q_budget") == (p.grid * 256, p.grid_alt * 256, p.grid + p.grid_first, p.alt_budget)
    assert ints(b, "N", "frame_doubles", "plan.q_alt") == (10, 20, 1) and int(b["handover_cap"]) > 0
    # the one-queue kernel's block: the frame's, but for its grid, a lane's 20 doubles per depth, its step batching, its slots
    # for the ray counts, its budgets, and of the staged tables only the scale+translate records
    aq = {k[3:]: v for k, v in b.items() if k.startswith("aq.")}
    own = {"nthreads": int(b["plan.grid_q"]) * 256, "frame_doubles": 20, "p_max_path": int(b["plan.q_p_max_path"]), "s_min_path": int(b["plan.q_s_min_path"]),
           "count_base": int(b["plan.grid"]) + int(b["plan.grid_first"]), "q_budget": int(b["plan.q_budget"]), "q_tail_budget": int(b["plan.q_tail_budget"]),
           "q_few_lanes": int(b["plan.q_few_lanes"]), "scene_lds": -1, "grid_occ_lds": -1, "diag_lds": int(b["plan.q_diag_lds"])}
    assert {k: int(aq[k]) for k in own} == own
    assert {k for k in aq if aq[k] != b[k]} <= set(own) and set(aq) == {k for k in b if not k.startswith(("plan.", "facts.", "aq.", "dome_cand[", "hoist_origin"))}
    assert ints(b, "aq.q_tail_budget", "aq.q_few_lanes", "aq.p_max_path", "aq.s_min_path") == (50, 16, 48, 16)  # (the table's defaults, pt_plan.h)
    assert int(b["scene_lds"]) >= 0 and int(b["aq.count_base"]) > 0  # (so the blocks do differ there)


def test_the_16x16_flat_frame_against_pt_debug_plan(blocks):
    b = blocks["plan_tile4_flat"]
    p = reported_plan(32, True, renderer=abi.RENDERER_FLAT)
    same_inputs(b, p)
    assert p.kernels == ["pt_tile4_kernel<FLAT, LDS>"] and int(b["plan.tile4"]) == 1  # (test_plan.py's C2 case)
    # (pt_debug_plan reports frame_doubles for path-tracer frames only)
    assert ints(b, "rows_local", "npix", "block_h", "spec_draws", "bs_levels") == (p.rows, p.npix, p.block_h, 0, p.ball_levels)
    assert ints(b, "nthreads", "npass", "n_shapes") == (p.grid * 256, 1, 33)
    assert not [k for k in b if k.startswith("aq.")]
