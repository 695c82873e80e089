"""``python -m pytracer_amd probes``: options and refusals without a GPU, and one lattice on the device against
``WorldQueries.radiance_probes``."""
import numpy as np
import pytest
from click.testing import CliRunner

from pytracer_amd.cli import cli, parse_grid

run = CliRunner().invoke


def test_the_probes_command_is_there_with_its_options():
    r = run(cli, ["probes", "--help"])
    assert r.exit_code == 0
    for option in ("--grid", "--input", "--output", "--samples", "--num-of-rays", "--max-depth", "--russian-roulette-limit", "--init-state",
                   "--init-seq", "--depth", "--declare-float", "--device"):
        assert option in r.output, option
    assert "probes" in run(cli, ["--help"]).output
    for other in ("render", "hits", "rays", "radiance", "gather", "bake"):  # (the other commands are where they were)
        assert run(cli, [other, "--help"]).exit_code == 0
    assert parse_grid("0,-1.5,2,0.25,3,2,1") == ((0.0, -1.5, 2.0), 0.25, (3, 2, 1))


def test_the_probes_command_checks_its_arguments(tmp_path):
    np.save(tmp_path / "ok.npy", np.zeros((4, 3)))
    np.save(tmp_path / "flat.npy", np.zeros(12))
    np.save(tmp_path / "text.npy", np.array([["a", "b", "c"]]))
    np.savez(tmp_path / "two.npz", a=np.zeros((4, 3)), b=np.zeros((4, 3)))
    np.savez(tmp_path / "named.npz", points=np.zeros((4, 2)), other=np.zeros(3))
    ok, grid = ["--input", str(tmp_path / "ok.npy")], ["--grid", "0,0,0,1,2,2,2"]
    cases = [([], "--grid or from --input"),
             (ok + grid, "--grid or from --input"),
             (["--grid", "0,0,0,1,2,2"], "ox,oy,oz,step,nx,ny,nz"),
             (["--grid", "0,0,0,one,2,2,2"], "ox,oy,oz,step,nx,ny,nz"),
             (["--grid", "0,0,0,1,2,2.5,2"], "ox,oy,oz,step,nx,ny,nz"),
             (["--grid", "0,0,0,0,2,2,2"], "step must be positive"),
             (["--grid", "0,0,0,1,2,0,2"], "at least 1"),
             (["--input", str(tmp_path / "missing.npy")], "missing.npy"),
             (["--input", str(tmp_path / "flat.npy")], "[n, 3]"),
             (["--input", str(tmp_path / "text.npy")], "[n, 3]"),
             (["--input", str(tmp_path / "two.npz")], "`points`"),
             (["--input", str(tmp_path / "named.npz")], "[n, 3]"),
             (ok + ["--samples", "0"], "--samples"),
             (ok + ["--num-of-rays", "0"], "--num-of-rays"),
             (ok + ["--max-depth", "-1"], "--max-depth"),
             (ok + ["--depth", "-1"], "--depth"),
             (ok + ["--max-depth", "70"], "64 levels"),
             (ok + ["--samples", str(2 ** 30)], "2^31 - 1"),
             (["--grid", "0,0,0,1,2048,1024,1024", "--samples", "1"], "2^31 - 1"),
             (ok + ["builtin:nowhere"], "no built-in scene"),
             (ok + ["-d", "clock"], "NAME:VALUE")]
    for args, word in cases:
        r = run(cli, ["probes"] + args)
        assert r.exit_code == 2 and word in r.output, (args, r.exit_code, r.output)
    assert run(cli, ["probes", "--samples", "many"]).exit_code == 2  # (click's own refusal)


@pytest.mark.gpu
def test_a_lattice_in_c2_equals_radiance_probes(tmp_path):
    from pytracer_amd import device, flatten, scenes
    from pytracer_amd import rays as rb

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    K = 6
    out = str(tmp_path / "probes.npz")
    r = run(cli, ["probes", "--grid", "-1,-2,0.5,1.5,3,2,2", "--samples", str(K), "--num-of-rays", "2", "--max-depth", "2",
                  "--russian-roulette-limit", "1", "--init-state", "7", "--init-seq", "1000", "--output", out, "builtin:c2"])
    assert r.exit_code == 0, r.output
    got = np.load(out)
    assert set(got.files) == {"coefficients", "n_rays", "points"} and f"12 probe(s) x {K} sample(s)" in r.output
    grid = rb.ProbeGrid((-1.0, -2.0, 0.5), 1.5, (3, 2, 2))
    assert np.array_equal(got["points"], grid.points()) and got["coefficients"].shape == (12, 9, 3)
    with device.DeviceScene(flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))) as ds:
        want = rb.WorldQueries(ds).radiance_probes(grid.points(), K, 7, 1000, None, None, 2, 2, 1, (0.0, 0.0, 0.0), 1, "all")
        assert got["coefficients"].tobytes() == np.ascontiguousarray(want.coefficients).tobytes() and np.array_equal(got["n_rays"], want.n_rays)
    assert want.n_rays.min() >= K and len(np.unique(got["coefficients"].reshape(12, 27), axis=0)) == 12
    # the same points through the --input route
    np.save(tmp_path / "points.npy", grid.points())
    out2 = str(tmp_path / "again.npz")
    r = run(cli, ["probes", "--input", str(tmp_path / "points.npy"), "--samples", str(K), "--num-of-rays", "2", "--max-depth", "2",
                  "--russian-roulette-limit", "1", "--init-state", "7", "--init-seq", "1000", "--output", out2, "builtin:c2"])
    assert r.exit_code == 0, r.output
    again = np.load(out2)
    assert again["coefficients"].tobytes() == got["coefficients"].tobytes() and np.array_equal(again["n_rays"], got["n_rays"])
