"""``python -m pytracer_amd lit``: options and refusals without a GPU, and on the device the ``probes`` command followed by ``lit``
against ``GpuImageTracer.fire_all_rays(ProbeLitShader(...))``."""
import numpy as np
import pytest
from click.testing import CliRunner

from pytracer_amd.cli import cli

run = CliRunner().invoke
GRID = "-1,-2,0.5,1.5,3,2,2"


def test_the_lit_command_is_there_with_its_options():
    r = run(cli, ["lit", "--help"])
    assert r.exit_code == 0
    for option in ("--probes", "--grid", "--width", "--height", "--output", "--declare-float", "--device"):
        assert option in r.output, option
    assert "lit" in run(cli, ["--help"]).output
    for other in ("render", "hits", "rays", "radiance", "gather", "bake", "probes"):  # (the other commands are where they were)
        assert run(cli, [other, "--help"]).exit_code == 0


def test_the_lit_command_checks_its_arguments(tmp_path):
    ok = str(tmp_path / "ok.npz")
    np.savez(ok, coefficients=np.zeros((12, 9, 3)), n_rays=np.zeros(12, np.uint64), points=np.zeros((12, 3)))
    np.savez(tmp_path / "bare.npz", points=np.zeros((12, 3)))
    np.savez(tmp_path / "flat.npz", coefficients=np.zeros((12, 27)))
    np.savez(tmp_path / "ints.npz", coefficients=np.zeros((12, 9, 3), np.int64))
    np.save(tmp_path / "array.npy", np.zeros((12, 9, 3)))
    good = ["--probes", ok, "--grid", GRID]
    cases = [(["--grid", GRID], "--probes"),  # (click's own refusals: a required option)
             (["--probes", ok], "--grid"),
             (["--probes", ok, "--grid", "0,0,0,1,2,2"], "ox,oy,oz,step,nx,ny,nz"),
             (["--probes", ok, "--grid", "0,0,0,0,3,2,2"], "step must be positive"),
             (["--probes", ok, "--grid", "0,0,0,1,3,2,3"], "holds 12 probes, the lattice of --grid has 18"),
             (["--probes", ok, "--grid", "0,0,0,1,1,1,1"], "the lattice of --grid has 1"),
             (["--probes", str(tmp_path / "missing.npz"), "--grid", GRID], "missing.npz"),
             (["--probes", str(tmp_path / "bare.npz"), "--grid", GRID], "`coefficients`"),
             (["--probes", str(tmp_path / "flat.npz"), "--grid", GRID], "[n, 9, 3]"),
             (["--probes", str(tmp_path / "ints.npz"), "--grid", GRID], "[n, 9, 3]"),
             (["--probes", str(tmp_path / "array.npy"), "--grid", GRID], "array.npy"),
             (good + ["--width", "0"], "--width"),
             (good + ["--height", "-3"], "--height"),
             (good + ["builtin:nowhere"], "no built-in scene"),
             (good + ["-d", "clock"], "NAME:VALUE")]
    for args, word in cases:
        r = run(cli, ["lit"] + args)
        assert r.exit_code == 2 and word in r.output, (args, r.exit_code, r.output)
    assert run(cli, ["lit"] + good + ["--width", "wide"]).exit_code == 2


@pytest.mark.gpu
def test_probes_then_lit_write_the_shaders_frame(tmp_path):
    from pytracer_amd import device, hostmodel as hm, scenes
    from pytracer_amd import rays as rb
    from pytracer_amd.shaders import ProbeLitShader
    from pytracer_amd.tracer import GpuImageTracer

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    W, H = 40, 30
    probes, frame = str(tmp_path / "probes.npz"), str(tmp_path / "frame.pfm")
    r = run(cli, ["probes", "--grid", GRID, "--samples", "16", "--max-depth", "2", "--output", probes, "builtin:c2"])
    assert r.exit_code == 0, r.output
    r = run(cli, ["lit", "--probes", probes, "--grid", GRID, "--width", str(W), "--height", str(H), "--output", frame, "builtin:c2"])
    assert r.exit_code == 0 and "3x2x2" in r.output, r.output
    raw = open(frame, "rb").read()
    head = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head)
    got = np.frombuffer(raw[len(head):], dtype="<f4").reshape(H, W, 3)[::-1]
    grid = rb.ProbeGrid((-1.0, -2.0, 0.5), 1.5, (3, 2, 2))
    world, camera = scenes.synthetic_world(32, with_plane=True), scenes.synthetic_camera(W, H)
    image = hm.HdrImage(W, H)
    tracer = GpuImageTracer(image, camera, samples_per_side=0)
    try:
        wq = tracer.world_queries(world)
        made = wq.radiance_probes(grid.points(), 16, 45, 54, None, None, 1, 2, 3, (0.0, 0.0, 0.0), 1, "all")
        assert np.load(probes)["coefficients"].tobytes() == np.ascontiguousarray(made.coefficients).tobytes()
        tracer.fire_all_rays(ProbeLitShader(world, grid, made, tracer))
    finally:
        tracer.close()
    want = np.asarray(image.array, dtype=np.float64)
    assert got.shape == (H, W, 3) and np.array_equal(got, want.astype(np.float32))  # (a PFM holds fp32)
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 100 and np.isfinite(got).all()
