"""``python -m pytracer_amd gradient``: options and refusals without a GPU, and on the device a three-frame run of a world whose sphere
moves, with the light followed and not followed."""
import numpy as np
import pytest
from click.testing import CliRunner

from pytracer_amd.cli import cli

run = CliRunner().invoke


def test_the_gradient_command_is_there_with_its_options():
    r = run(cli, ["gradient", "--help"])
    assert r.exit_code == 0
    for option in ("--width", "--height", "--frames", "--step-deg", "--samples", "--move", "--no-follow-light", "--stratum", "--radius", "--gain",
                   "--max-history", "--passes", "--max-depth", "--pfm-output", "--declare-float", "--device"):
        assert option in r.output, option
    assert "SHAPE:DX:DY:DZ" in r.output and "gradient" in run(cli, ["--help"]).output
    for other in ("render", "hits", "rays", "radiance", "gather", "bake", "probes", "lit", "denoise", "temporal", "variance", "adaptive", "weighted",
                  "motion"):
        assert run(cli, [other, "--help"]).exit_code == 0  # (where they were)
    assert "--stratum" not in run(cli, ["motion", "--help"]).output


def test_the_gradient_command_checks_its_arguments():
    cases = [(["--width", "0"], "--width"),
             (["--height", "-3"], "--height"),
             (["--frames", "0"], "--frames"),
             (["--step-deg", "nan"], "--step-deg"),
             (["--samples", "0"], "--samples"),
             (["--stratum", "0"], "--stratum"),
             (["--stratum", "17"], "--stratum"),
             (["--radius", "-1"], "--radius"),
             (["--radius", "5"], "--radius"),
             (["--gain", "-0.5"], "--gain"),
             (["--gain", "nan"], "--gain"),
             (["--max-history", "0"], "--max-history"),
             (["--passes", "11"], "--passes"),
             (["--max-depth", "-1"], "--max-depth"),
             (["--move", "2:0:0.4"], "SHAPE:DX:DY:DZ"),
             (["--move", "3:0:0.4:0"], "shapes 0 to 2"),
             (["--move", "2:0:inf:0"], "finite"),
             (["builtin:nowhere"], "no built-in scene"),
             (["-d", "clock"], "NAME:VALUE")]
    for args, word in cases:
        r = run(cli, ["gradient"] + args)
        assert r.exit_code == 2 and word in r.output and "pytracer_amd gradient:" in r.output, (args, r.exit_code, r.output)
    assert run(cli, ["gradient", "--frames", "many"]).exit_code == 2


def _pfm(name, W, H):
    raw = open(name, "rb").read()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + 12 * W * H
    return np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)[::-1]


@pytest.mark.gpu
def test_the_command_follows_the_light_or_does_not(tmp_path):
    from pytracer_amd import device

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    W, H, N = 48, 36, 3
    common = ["gradient", "--width", str(W), "--height", str(H), "--frames", str(N), "--samples", "2", "--passes", "0", "--max-depth", "2"]
    moving = common + ["--move", "2:0:0.4:0"]
    followed, shapes_only, still = str(tmp_path / "followed.pfm"), str(tmp_path / "shapes_only.pfm"), str(tmp_path / "still.pfm")
    r = run(cli, moving + ["--pfm-output", followed, "builtin:demo"])
    assert r.exit_code == 0 and f"{N} frame(s)" in r.output and "1 moving," in r.output and f"longest history {N}" in r.output, r.output
    assert " 0 pixel(s) kept less" not in r.output, r.output
    q = run(cli, moving + ["--no-follow-light", "--pfm-output", shapes_only, "builtin:demo"])
    assert q.exit_code == 0 and "(light not followed)" in q.output, q.output
    a, b = _pfm(followed, W, H), _pfm(shapes_only, W, H)
    assert np.isfinite(a).all() and np.isfinite(b).all() and len(np.unique(a.reshape(-1, 3), axis=0)) > 20
    differ = (a != b).any(axis=-1)
    assert differ.any() and not differ.all()  # (where the light changed the frames differ; the sky and the ground far away do not)
    # a world at rest keeps everything: the two commands write the same bytes
    s = run(cli, common + ["--pfm-output", still, "builtin:demo"])
    assert s.exit_code == 0 and " 0 pixel(s) kept less" in s.output, s.output
    t = run(cli, ["motion"] + common[1:] + ["--pfm-output", shapes_only, "builtin:demo"])
    assert t.exit_code == 0 and open(still, "rb").read() == open(shapes_only, "rb").read()
