"""The Flat palette (csrc/pt_layout.h: PtFlatPal) on the CPU: tests/flat_palette/flat_palette_check.cpp (a program with its own
main, no HIP call) runs pt_build_scene over generated scenes of 0, 1, 63, 64, 65 and 256 shapes and checks every palette entry
against the aux[] record and against the description: needs_uv equal; the colour bit for bit pig_c1 + emi_c1 (= aux.pig_c2)
where both pigments are uniform, sums that are inexact in fp64 among them, and zero elsewhere; the record's padding zero; the
image the upload puts behind aux[] padded with zeros to whole 1 KiB chunks; the four wave slices of pt_tile4_kernel<FLAT, LDS>
inside the LDS block the plan reserves.  The second test runs the same program under the host AddressSanitizer and
UndefinedBehaviorSanitizer (the stand-alone program only: nothing is loaded into Python)."""
import os
import subprocess

from pytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "flat_palette", "flat_palette_check.cpp")
SHAPES = [0, 1, 63, 64, 65, 256]
# host code only (the headers define no kernel); the library's own floating-point flags
FLAGS = ["-x", "hip", "--offload-host-only", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Werror"]


def run_check(tmp_path, name, extra):
    exe = str(tmp_path / name)
    r = subprocess.run([build._hipcc()] + FLAGS + extra + ["-o", exe, SOURCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [line.split() for line in r.stdout.splitlines()]
    assert [int(f[0]) for f in lines] == SHAPES and all(f[1] == "ok" for f in lines), r.stdout
    for n, f in zip(SHAPES, lines):
        checked, uniform, chunks = int(f[2]), int(f[3]), int(f[4])
        assert checked == n and chunks == (32 * n + 1023) // 1024
        assert 0 < uniform < n or n <= 1


def test_every_entry_equals_its_aux_record_and_the_padding_is_zero(tmp_path):
    run_check(tmp_path, "flat_palette_check", ["-O3"])


def test_the_palette_is_clean_under_the_host_sanitizers(tmp_path):
    run_check(tmp_path, "flat_palette_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
