"""``python -m pytracer_amd motion``: options and refusals without a GPU, and on the device a three-frame run of a world whose sphere
moves, followed and not followed."""
import numpy as np
import pytest
from click.testing import CliRunner

from pytracer_amd.cli import cli

run = CliRunner().invoke


def test_the_motion_command_is_there_with_its_options():
    r = run(cli, ["motion", "--help"])
    assert r.exit_code == 0
    for option in ("--width", "--height", "--frames", "--step-deg", "--samples", "--move", "--no-follow", "--max-history", "--passes", "--max-depth",
                   "--pfm-output", "--declare-float", "--device"):
        assert option in r.output, option
    assert "SHAPE:DX:DY:DZ" in r.output and "motion" in run(cli, ["--help"]).output
    for other in ("render", "hits", "rays", "radiance", "gather", "bake", "probes", "lit", "denoise", "temporal", "variance", "adaptive", "weighted"):
        assert run(cli, [other, "--help"]).exit_code == 0  # (where they were)
    assert "--move" not in run(cli, ["temporal", "--help"]).output


def test_the_motion_command_checks_its_arguments():
    cases = [(["--width", "0"], "--width"),
             (["--height", "-3"], "--height"),
             (["--frames", "0"], "--frames"),
             (["--step-deg", "nan"], "--step-deg"),
             (["--samples", "0"], "--samples"),
             (["--max-history", "0"], "--max-history"),
             (["--passes", "11"], "--passes"),
             (["--max-depth", "-1"], "--max-depth"),
             (["--move", "2:0:0.4"], "SHAPE:DX:DY:DZ"),
             (["--move", "sphere:0:0.4:0"], "SHAPE:DX:DY:DZ"),
             (["--move", "2:0:far:0"], "SHAPE:DX:DY:DZ"),
             (["--move", "3:0:0.4:0"], "shapes 0 to 2"),
             (["--move", "-1:0:0.4:0"], "shapes 0 to 2"),
             (["--move", "2:0:inf:0"], "finite"),
             (["--move", "2:0:0.4:0", "--move", "1:nan:0:0"], "finite"),
             (["builtin:nowhere"], "no built-in scene"),
             (["-d", "clock"], "NAME:VALUE")]
    for args, word in cases:
        r = run(cli, ["motion"] + args)
        assert r.exit_code == 2 and word in r.output and "pytracer_amd motion:" in r.output, (args, r.exit_code, r.output)
    assert run(cli, ["motion", "--frames", "many"]).exit_code == 2


def _pfm(name, W, H):
    raw = open(name, "rb").read()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + 12 * W * H
    return np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)[::-1]


@pytest.mark.gpu
def test_the_command_follows_a_moving_sphere_or_does_not(tmp_path):
    from pytracer_amd import device

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    W, H, N = 48, 36, 3
    common = ["motion", "--width", str(W), "--height", str(H), "--frames", str(N), "--samples", "2", "--passes", "0", "--move", "2:0:0.4:0"]
    followed, camera_only = str(tmp_path / "followed.pfm"), str(tmp_path / "camera_only.pfm")
    r = run(cli, common + ["--pfm-output", followed, "builtin:demo"])
    assert r.exit_code == 0 and f"{N} frame(s)" in r.output and "1 moving," in r.output and f"longest history {N}" in r.output, r.output
    q = run(cli, common + ["--no-follow", "--pfm-output", camera_only, "builtin:demo"])
    assert q.exit_code == 0 and "(not followed)" in q.output, q.output
    a, b = _pfm(followed, W, H), _pfm(camera_only, W, H)
    assert np.isfinite(a).all() and np.isfinite(b).all() and len(np.unique(a.reshape(-1, 3), axis=0)) > 20
    differ = (a != b).any(axis=-1)
    assert differ.any() and not differ.all()  # (the sphere's pixels differ; the sky and the ground far from it do not)
