"""A sphere whose hoisted c = |o'|^2 - 1 is <= -0.5 encloses the camera: the kernels leave out the first root's division
(csrc/pt_query.h: PT_SPHERE_ROOTS_IN).  tests/proofs/sphere_inside_roots.c restates shapes.py:103-121 with and without the
skip and compares verdict and accepted t over 1e8 inputs.  CPU only (gcc + OpenMP, a few seconds)."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pytracer_amd", "csrc")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_both_forms_agree_on_1e8_inputs(tmp_path):
    exe = str(tmp_path / "sphere_inside_roots")
    r = subprocess.run(["gcc", "-O2", "-fopenmp", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "proofs", "sphere_inside_roots.c"),
                        "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout
    print(run.stdout)
    n = dict(zip(("inputs", "inside", "outside", "delta", "hit", "equal"), map(int, re.findall(r": (\d+)", run.stdout.splitlines()[0]))))
    assert n["inputs"] >= 100_000_000
    # the inputs are not vacuous: most run the skipping form, with real roots and accepted hits; both sides of the guard; |bb| == sd
    assert n["inside"] > n["inputs"] // 2 and n["outside"] > 1_000_000
    assert n["delta"] > n["inputs"] // 2 and n["hit"] > n["inputs"] // 4 and n["equal"] > 1_000_000
    assert "first root acceptable under the guard: 0; differences between the two forms: 0" in run.stdout


def test_the_kernel_source_is_what_the_program_restates():
    src = open(os.path.join(CSRC, "pt_query.h")).read()
    assert "PT_DEV bool pt_origin_inside(double hoisted_c) { return hoisted_c <= -0.5; }" in src
    body = src[src.index("#define PT_SPHERE_ROOTS_IN(SLOT, INSIDE)"):]
    body = re.sub(r"\s*\\\n\s*", " ", body[:body.index("while (0)")])
    for piece in ("const double delta = bb * bb - 4.0 * aa * cc;", "const double sd = sqrt(delta);", "const double den = 2.0 * aa;",
                  "if (!(INSIDE)) { t = (-bb - sd) / den; ok = (t > tmin) && (t < tmax); }",
                  "if (!ok) { t = (-bb + sd) / den; ok = (t > tmin) && (t < tmax); }"):
        assert piece in body, piece
