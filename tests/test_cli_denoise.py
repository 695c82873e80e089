"""``python -m pytracer_amd denoise``: options and refusals without a GPU, and on the device the command's PFM against
``GpuImageTracer.fire_all_rays(DenoisedGatherShader(...))``, with and without the filter."""
import numpy as np
import pytest
from click.testing import CliRunner

from pytracer_amd.cli import cli

run = CliRunner().invoke


def test_the_denoise_command_is_there_with_its_options():
    r = run(cli, ["denoise", "--help"])
    assert r.exit_code == 0
    for option in ("--width", "--height", "--samples", "--passes", "--sigma-point", "--normal-power-log2", "--sigma-colour", "--pfm-output",
                   "--png-output", "--noisy-output", "--declare-float", "--device"):
        assert option in r.output, option
    assert "denoise" in run(cli, ["--help"]).output
    for other in ("render", "hits", "rays", "radiance", "gather", "bake", "probes", "lit"):  # (the other commands are where they were)
        assert run(cli, [other, "--help"]).exit_code == 0


def test_the_denoise_command_checks_its_arguments():
    cases = [(["--width", "0"], "--width"),
             (["--height", "-3"], "--height"),
             (["--samples", "0"], "--samples"),
             (["--passes", "0"], "--passes"),
             (["--passes", "11"], "--passes"),
             (["--normal-power-log2", "11"], "--normal-power-log2"),
             (["--normal-power-log2", "-1"], "--normal-power-log2"),
             (["--sigma-point", "0"], "--sigma-point"),
             (["--sigma-point", "nan"], "--sigma-point"),
             (["--sigma-colour", "-2"], "--sigma-colour"),
             (["--max-depth", "-1"], "--max-depth"),
             (["builtin:nowhere"], "no built-in scene"),
             (["-d", "clock"], "NAME:VALUE")]
    for args, word in cases:
        r = run(cli, ["denoise"] + args)
        assert r.exit_code == 2 and word in r.output, (args, r.exit_code, r.output)
    assert run(cli, ["denoise", "--width", "wide"]).exit_code == 2 and run(cli, ["denoise", "--sigma-point", "near"]).exit_code == 2


def _pfm(name, W, H):
    raw = open(name, "rb").read()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)[::-1]


@pytest.mark.gpu
def test_the_command_writes_the_shaders_frame_and_the_unfiltered_one(tmp_path):
    from pytracer_amd import device, hostmodel as hm, scenes
    from pytracer_amd.shaders import DenoisedGatherShader
    from pytracer_amd.tracer import GpuImageTracer

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    W, H = 40, 30
    frame, noisy, png = str(tmp_path / "frame.pfm"), str(tmp_path / "noisy.pfm"), str(tmp_path / "frame.png")
    r = run(cli, ["denoise", "--width", str(W), "--height", str(H), "--samples", "4", "--passes", "3", "--sigma-point", "0.25", "--normal-power-log2", "4",
                  "--sigma-colour", "2.0", "--pfm-output", frame, "--png-output", png, "--noisy-output", noisy, "builtin:demo"])
    assert r.exit_code == 0 and "3 filter pass(es)" in r.output, r.output
    assert open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    world, camera = scenes.demo_world()
    image = hm.HdrImage(W, H)
    tracer = GpuImageTracer(image, camera, samples_per_side=0)
    try:
        shader = DenoisedGatherShader(world, tracer, 4, init_state=45, init_seq=54, max_depth=3, passes=3, sigma_point=0.25, normal_power_log2=4,
                                      sigma_colour=2.0)
        for name, filtered in ((frame, True), (noisy, False)):
            shader.filtered = filtered
            tracer.fire_all_rays(shader)
            want = np.asarray(image.array, dtype=np.float64).reshape(H, W, 3)
            got = _pfm(name, W, H)
            assert np.array_equal(got, want.astype(np.float32)), name  # (a PFM holds fp32)
            assert np.isfinite(got).all() and len(np.unique(got.reshape(-1, 3), axis=0)) > 20
    finally:
        tracer.close()
    assert not np.array_equal(_pfm(frame, W, H), _pfm(noisy, W, H))
