"""``python -m pytracer_amd variance``: options and refusals without a GPU, and on the device the command's PFMs against a sequence of
``GpuImageTracer.fire_all_rays(VarianceGuidedGatherShader(...))`` under the same turning camera."""
import numpy as np
import pytest
from click.testing import CliRunner

from pytracer_amd.cli import cli

run = CliRunner().invoke


def test_the_variance_command_is_there_with_its_options():
    r = run(cli, ["variance", "--help"])
    assert r.exit_code == 0
    for option in ("--width", "--height", "--frames", "--step-deg", "--samples", "--max-history", "--min-history", "--normal-min",
                   "--point-tolerance", "--passes", "--sigma-point", "--sigma-luminance", "--epsilon", "--pfm-output", "--variance-output",
                   "--declare-float", "--device"):
        assert option in r.output, option
    assert "variance" in run(cli, ["--help"]).output
    for other in ("render", "hits", "rays", "radiance", "gather", "bake", "probes", "lit", "denoise", "temporal"):  # (where they were)
        assert run(cli, [other, "--help"]).exit_code == 0


def test_the_variance_command_checks_its_arguments():
    cases = [(["--width", "0"], "--width"),
             (["--height", "-3"], "--height"),
             (["--frames", "0"], "--frames"),
             (["--step-deg", "nan"], "--step-deg"),
             (["--step-deg", "inf"], "--step-deg"),
             (["--samples", "0"], "--samples"),
             (["--max-history", "0"], "--max-history"),
             (["--max-history", "1048577"], "--max-history"),
             (["--min-history", "0"], "--min-history"),
             (["--min-history", "1048577"], "--min-history"),
             (["--normal-min", "1.5"], "--normal-min"),
             (["--normal-min", "nan"], "--normal-min"),
             (["--point-tolerance", "0"], "--point-tolerance"),
             (["--point-tolerance", "nan"], "--point-tolerance"),
             (["--passes", "-1"], "--passes"),
             (["--passes", "11"], "--passes"),
             (["--sigma-point", "0"], "--sigma-point"),
             (["--sigma-luminance", "0"], "--sigma-luminance"),
             (["--sigma-luminance", "nan"], "--sigma-luminance"),
             (["--epsilon", "0"], "--epsilon"),
             (["--epsilon", "inf"], "--epsilon"),
             (["--epsilon", "nan"], "--epsilon"),
             (["--max-depth", "-1"], "--max-depth"),
             (["builtin:nowhere"], "no built-in scene"),
             (["-d", "clock"], "NAME:VALUE")]
    for args, word in cases:
        r = run(cli, ["variance"] + args)
        assert r.exit_code == 2 and word in r.output, (args, r.exit_code, r.output)
    assert run(cli, ["variance", "--frames", "many"]).exit_code == 2 and run(cli, ["variance", "--sigma-luminance", "wide"]).exit_code == 2


def _pfm(name, W, H):
    raw = open(name, "rb").read()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)[::-1]


@pytest.mark.gpu
def test_the_command_writes_the_shaders_last_frame_and_its_variance(tmp_path):
    from pytracer_amd import device, hostmodel as hm, scenes
    from pytracer_amd.shaders import VarianceGuidedGatherShader
    from pytracer_amd.tracer import GpuImageTracer

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    W, H, N, step = 40, 30, 3, 2.0
    frame, var = str(tmp_path / "frame.pfm"), str(tmp_path / "variance.pfm")
    r = run(cli, ["variance", "--width", str(W), "--height", str(H), "--frames", str(N), "--step-deg", str(step), "--samples", "4", "--max-history", "8",
                  "--min-history", "2", "--normal-min", "0.8", "--point-tolerance", "0.1", "--passes", "2", "--sigma-point", "0.25",
                  "--sigma-luminance", "2", "--epsilon", "1e-8", "--pfm-output", frame, "--variance-output", var, "builtin:demo"])
    assert r.exit_code == 0 and f"{N} frame(s)" in r.output and f"longest history {N}" in r.output and "mean variance" in r.output, r.output
    world, camera = scenes.demo_world()
    image = hm.HdrImage(W, H)
    tracer = GpuImageTracer(image, camera, samples_per_side=0)
    try:
        shader = VarianceGuidedGatherShader(world, tracer, 4, init_state=45, init_seq=54, max_depth=3, passes=2, sigma_point=0.25, sigma_luminance=2.0,
                                            epsilon=1e-8, max_history=8, min_history=2, normal_min=0.8, point_tolerance=0.1)
        for f in range(N):
            tracer.camera = scenes.turned_camera(camera, step * f)
            tracer.fire_all_rays(shader)
        want = np.asarray(image.array, dtype=np.float64).reshape(H, W, 3)
        got = _pfm(frame, W, H)
        assert np.array_equal(got, want.astype(np.float32))  # (a PFM holds fp32)
        assert np.isfinite(got).all() and len(np.unique(got.reshape(-1, 3), axis=0)) > 20
        got_var = _pfm(var, W, H)
        assert np.array_equal(got_var, np.repeat(shader.last_variance[..., None], 3, axis=-1).astype(np.float32)) and (got_var > 0).any()
        assert shader.frame_no == N and shader.accumulator.count.max() == N
    finally:
        tracer.close()
