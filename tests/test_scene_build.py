"""csrc/pt_scene_build.h on its own, on the CPU: tests/scene_build/scene_digest.cpp (a program with its own main, no HIP
call) runs pt_build_scene over generated scenes -- the smallest at which each branch of the analysis runs -- and prints a
digest of every table and every scalar.  tests/golden/g14_scene_build_digests.txt holds what the analysis printed for the
same scenes while it was still ptrace.hip's analyse_scene(): the same program, with the .hip file included in place of the
header.  Every line must be equal: no tolerance, no scene left out.  The second test runs the program under the host
AddressSanitizer and UndefinedBehaviorSanitizer (the stand-alone program only: nothing is loaded into Python)."""
import os
import subprocess

import pytest

from pytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "scene_build", "scene_digest.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "g14_scene_build_digests.txt")
SCENES = ["empty", "plane_only", "general", "spheres_127", "spheres_128", "grid_1100", "grid_1100_off", "grid_1100_density9",
          "grid_130_min64", "grid_130_default", "nonfinite_centre", "nonfinite_centre_few", "m_not_inverse", "singular_scale",
          "huge_radius", "huge_radius_grid", "crowded_cells", "bad_kind", "bad_texture"]
# host code only (the header defines no kernel); the library's own floating-point flags
FLAGS = ["-x", "hip", "--offload-host-only", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Werror"]


def digests(tmp_path, name, extra):
    exe = str(tmp_path / name)
    r = subprocess.run([build._hipcc()] + FLAGS + extra + ["-o", exe, SOURCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    return r.stdout.splitlines()


def compare(got):
    want = open(FIXTURE).read().splitlines()
    assert [s for s in SCENES if not any(line.startswith(s + " ") for line in want)] == [], "a scene is missing from the fixture"
    different = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not different, (len(got), len(want), different[:10])


def test_every_table_and_scalar_equals_what_the_analysis_gave_before_it_moved(tmp_path):
    compare(digests(tmp_path, "scene_digest", ["-O3"]))


def test_the_analysis_is_clean_under_the_host_sanitizers(tmp_path):
    compare(digests(tmp_path, "scene_digest_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))

