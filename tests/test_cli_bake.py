"""``python -m pytracer_amd bake`` without a GPU: its options are validated before a device is touched, and a bad one ends the
command with status 2 and a message that names it."""
import pytest
from click.testing import CliRunner

from pytracer_amd import cli as C

BAD = [
    (["--shape", "0", "--size", "64"], "--size expects WxH"),
    (["--shape", "0", "--size", "0x8"], "--size expects WxH"),
    (["--shape", "0", "--size", "8x-1"], "--size expects WxH"),
    (["--shape", "0", "--size", "axb"], "--size expects WxH"),
    (["--shape", "0", "--side", "0"], "--side 0"),
    (["--shape", "0", "--side", "2"], "--side 2"),
    (["--shape", "0", "--samples", "0"], "--samples"),
    (["--shape", "0", "--num-of-rays", "0"], "--num-of-rays"),
    (["--shape", "0", "--max-depth", "-1"], "--max-depth"),
    (["--shape", "0", "--depth", "-1"], "--depth"),
    (["--shape", "0", "--max-depth", "70", "--depth", "5"], "64 levels"),
    (["--shape", "0", "--size", "65536x2", "--samples", "32768"], "2^31 - 1"),
    (["--shape", "3"], "--shape 3: the scene has 3 shape(s)"),
    (["--shape", "-1"], "--shape -1"),
    (["--shape", "2"], "SpecularBRDF"),  # demo's mirror sphere
    (["--shape", "0", "-d", "clock"], "-d expects NAME:VALUE"),
    (["--shape", "0", "builtin:nothing"], "no built-in scene"),
]


@pytest.mark.parametrize("args,word", BAD, ids=[" ".join(a) for a, _ in BAD])
def test_bake_refuses_bad_options_with_status_2(args, word, tmp_path):
    out = tmp_path / "map.pfm"
    scene = [] if any(a.startswith("builtin:") for a in args) else ["builtin:demo"]
    r = CliRunner().invoke(C.cli, ["bake", "-o", str(out)] + args + scene)
    assert r.exit_code == 2, (r.exit_code, r.output)
    assert "pytracer_amd bake: " in r.output and word in r.output, r.output
    assert not out.exists()


def test_bake_needs_a_shape_and_lists_its_options():
    r = CliRunner().invoke(C.cli, ["bake", "builtin:demo"])
    assert r.exit_code == 2 and "--shape" in r.output
    r = CliRunner().invoke(C.cli, ["bake", "--help"])
    assert r.exit_code == 0
    for option in ("--shape", "--size", "--samples", "--side", "--no-jitter", "-o, --output"):
        assert option in r.output, option
    assert C.parse_size("512x256") == (512, 256) and C.parse_size("7X5") == (7, 5)
