"""``python -m pytracer_amd weighted``: options and refusals without a GPU, and on the device the command's PFMs against a sequence of
``GpuImageTracer.fire_all_rays(WeightedAdaptiveGatherShader(...))`` under the same turning camera."""
import numpy as np
import pytest
from click.testing import CliRunner

from pytracer_amd.cli import cli

run = CliRunner().invoke


def test_the_weighted_command_is_there_with_its_options():
    r = run(cli, ["weighted", "--help"])
    assert r.exit_code == 0
    for option in ("--width", "--height", "--frames", "--step-deg", "--samples", "--min-samples", "--max-samples", "--tolerance", "--luminance-floor",
                   "--gain", "--budget", "--max-history", "--max-weight", "--blend-weight", "--min-history", "--passes", "--sigma-luminance",
                   "--max-depth", "--pfm-output", "--counts-output", "--declare-float", "--device"):
        assert option in r.output, option
    assert "weighted" in run(cli, ["--help"]).output
    for other in ("render", "hits", "rays", "radiance", "gather", "bake", "probes", "lit", "denoise", "temporal", "variance", "adaptive"):
        assert run(cli, [other, "--help"]).exit_code == 0  # (where they were)
    assert "--max-weight" not in run(cli, ["adaptive", "--help"]).output


def test_the_weighted_command_checks_its_arguments():
    cases = [(["--width", "0"], "--width"),
             (["--height", "-3"], "--height"),
             (["--frames", "0"], "--frames"),
             (["--step-deg", "nan"], "--step-deg"),
             (["--samples", "0"], "--samples"),
             (["--min-samples", "-1"], "--min-samples"),
             (["--min-samples", "33"], "--min-samples"),
             (["--max-samples", "1048577", "--min-samples", "4"], "--max-samples"),
             (["--tolerance", "0"], "--tolerance"),
             (["--tolerance", "nan"], "--tolerance"),
             (["--luminance-floor", "0"], "--luminance-floor"),
             (["--luminance-floor", "inf"], "--luminance-floor"),
             (["--gain", "0"], "--gain"),
             (["--gain", "inf"], "--gain"),
             (["--gain", "nan"], "--gain"),
             (["--budget", "-1"], "--budget"),
             (["--budget", "2147483648"], "--budget"),
             (["--max-history", "0"], "--max-history"),
             (["--max-weight", "-1"], "--max-weight"),
             (["--max-weight", "nan"], "--max-weight"),
             (["--min-history", "1048577"], "--min-history"),
             (["--passes", "11"], "--passes"),
             (["--sigma-luminance", "0"], "--sigma-luminance"),
             (["--max-depth", "-1"], "--max-depth"),
             (["builtin:nowhere"], "no built-in scene"),
             (["-d", "clock"], "NAME:VALUE")]
    for args, word in cases:
        r = run(cli, ["weighted"] + args)
        assert r.exit_code == 2 and word in r.output and "pytracer_amd weighted:" in r.output, (args, r.exit_code, r.output)
    assert run(cli, ["weighted", "--frames", "many"]).exit_code == 2 and run(cli, ["weighted", "--max-weight", "heavy"]).exit_code == 2
    # --min-samples 0 passes the argument checks here (the next refusal is the scene's), and is still refused by `adaptive`
    r = run(cli, ["weighted", "--min-samples", "0", "builtin:nowhere"])
    assert r.exit_code == 2 and "no built-in scene" in r.output
    assert "--min-samples" in run(cli, ["adaptive", "--min-samples", "0", "builtin:nowhere"]).output


def _pfm(name, W, H):
    raw = open(name, "rb").read()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)[::-1]


@pytest.mark.gpu
def test_the_command_writes_the_shaders_last_frame_and_its_counts(tmp_path):
    from pytracer_amd import device, hostmodel as hm, scenes
    from pytracer_amd.shaders import WeightedAdaptiveGatherShader
    from pytracer_amd.tracer import GpuImageTracer

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    W, H, N, step = 40, 30, 3, 2.0
    frame, cnt = str(tmp_path / "frame.pfm"), str(tmp_path / "counts.pfm")
    r = run(cli, ["weighted", "--width", str(W), "--height", str(H), "--frames", str(N), "--step-deg", str(step), "--samples", "4", "--min-samples", "0",
                  "--max-samples", "16", "--tolerance", "0.1", "--luminance-floor", "0.1", "--gain", "2", "--max-history", "8", "--max-weight", "40",
                  "--blend-weight", "--min-history", "2", "--passes", "2", "--sigma-luminance", "2", "--pfm-output", frame, "--counts-output", cnt,
                  "builtin:demo"])
    assert r.exit_code == 0 and f"{N} frame(s)" in r.output and f"longest history {N}" in r.output and "rays per frame" in r.output, r.output
    assert "largest weight" in r.output
    world, camera = scenes.demo_world()
    image = hm.HdrImage(W, H)
    tracer = GpuImageTracer(image, camera, samples_per_side=0)
    try:
        shader = WeightedAdaptiveGatherShader(world, tracer, 4, init_state=45, init_seq=54, max_depth=3, passes=2, sigma_luminance=2.0, max_history=8,
                                              max_weight=40.0, blend_weight=True, min_history=2, min_samples=0, max_samples=16, tolerance=0.1,
                                              luminance_floor=0.1, gain=2.0)
        totals = []
        for f in range(N):
            tracer.camera = scenes.turned_camera(camera, step * f)
            tracer.fire_all_rays(shader)
            totals.append(shader.last_total)
        want = np.asarray(image.array, dtype=np.float64).reshape(H, W, 3)
        got = _pfm(frame, W, H)
        assert np.array_equal(got, want.astype(np.float32))  # (a PFM holds fp32)
        assert np.isfinite(got).all() and len(np.unique(got.reshape(-1, 3), axis=0)) > 20
        counts = np.asarray(shader.last_counts)
        assert np.array_equal(_pfm(cnt, W, H), np.repeat(counts[..., None], 3, axis=-1).astype(np.float32))
        assert counts.shape == (H, W) and counts.min() >= 0 and counts.max() <= 16 and len(set(counts.reshape(-1).tolist())) > 3
        assert "rays per frame " + " ".join(str(t) for t in totals) in r.output and totals[0] % 4 == 0 and totals[0] > 0 and totals[-1] == int(counts.sum())
        weight = shader.accumulator.weight
        assert shader.frame_no == N and shader.accumulator.count.max() == N and f"largest weight {float(weight.max()):g}" in r.output
        assert weight.max() <= 40.0 + 16.0
    finally:
        tracer.close()
