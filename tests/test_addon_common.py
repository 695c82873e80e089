"""CPU-only tests of what the add-on libraries share since their host layer was written once: the loader (pytracer_amd._addon)
behind the five ``_NAME_lib`` modules, the channel parser behind the four ``*_channels`` functions of pytracer_amd.rays, and
csrc/pt_host_common.h, which every add-on translation unit includes instead of carrying a copy.  The expected values and error
texts of the parsers are those of the four hand-written parsers this replaced."""
import os
import re
import subprocess
import sys

import pytest

from pytracer_amd import rays as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDONS = ("rays", "surface", "scatter", "radiance", "gather")

_CHILD = """
from pytracer_amd import _{name}_lib as m
print("PATH", m.lib_path())
try:
    m.lib()
except ImportError as e:
    print("IMPORTERROR", e)
"""


@pytest.mark.parametrize("name", ADDONS)
def test_a_loader_honours_its_override_and_names_the_build_command_when_the_file_is_missing(name, tmp_path):
    """In a child process: the handle this process may have cached stays what it is."""
    import importlib

    module = importlib.import_module(f"pytracer_amd._{name}_lib")
    if not os.environ.get(f"PTRACE_{name.upper()}_LIB"):
        assert module.lib_path() == os.path.join(ROOT, "pytracer_amd", f"libptrace_{name}.so")
    missing = str(tmp_path / f"elsewhere_{name}.so")
    env = dict(os.environ, **{f"PTRACE_{name.upper()}_LIB": missing})
    r = subprocess.run([sys.executable, "-c", _CHILD.format(name=name)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    assert out["PATH"] == missing
    assert out["IMPORTERROR"].startswith(f"{missing} is missing: the HIP extension has not been built.")
    assert "python -m pytracer_amd.build" in out["IMPORTERROR"] and "no CPU fallback" in out["IMPORTERROR"]
    # (the override of one library is not another's: every other loader still points into the tree)
    for other in ADDONS:
        if other != name and not os.environ.get(f"PTRACE_{other.upper()}_LIB"):
            assert importlib.import_module(f"pytracer_amd._{other}_lib").lib_path().endswith(f"libptrace_{other}.so")


def test_importing_the_loaders_loads_no_library():
    """Lazy as before: nothing is dlopen-ed until the first ``lib()``."""
    code = ("import sys\n"
            "from pytracer_amd import _rays_lib, _surface_lib, _scatter_lib, _radiance_lib, _gather_lib, _lib\n"
            "maps = open('/proc/self/maps').read()\n"
            "print('MAPPED', 'libptrace' in maps, 'libamdhip64' in maps)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "MAPPED False False"


# parser, ALL, a name list and its bits, one name and its bit, the ValueError for unknown names, the ValueError for a stray bit
PARSERS = [
    (rb.surface_channels, 3, " Emitted , brdf_color,emitted,", 3, "emitted", 2,
     "a surface batch has the channels brdf_color, emitted; not bogus, all", "a surface batch has the channels brdf_color (1), emitted (2); not 0x4"),
    (rb.scatter_channels, 3, " Emitted , weight,emitted,", 3, "emitted", 2,
     "a scatter batch has the channels weight, emitted; not bogus, all", "a scatter batch has the channels weight (1), emitted (2); not 0x4"),
    (rb.radiance_channels, 3, " Count , pcg,count,", 3, "count", 2,
     "a radiance batch has the channels pcg, count; not bogus, all", "a radiance batch has the channels pcg (1), count (2); not 0x4"),
    (rb.gather_channels, 1, " Count , count,", 1, "count", 1,
     "a gather batch has the channel count; not bogus, all", "a gather batch has the channel count (1); not 0x2"),
]


@pytest.mark.parametrize("parse, all_bits, listed, listed_bits, second, second_bits, names_error, int_error", PARSERS, ids=lambda x: getattr(x, "__name__", None))
def test_a_channel_parser_gives_the_values_and_the_errors_it_always_gave(parse, all_bits, listed, listed_bits, second, second_bits, names_error, int_error):
    assert parse("all") == parse(" ALL ") == all_bits
    assert parse("none") == parse("None,") == parse("") == parse(" , ") == 0
    assert parse(listed) == listed_bits  # (repeats count once, spaces, case and empty items do not matter)
    assert parse(second) == second_bits
    assert [parse(b) for b in range(all_bits + 1)] == list(range(all_bits + 1))
    with pytest.raises(ValueError) as e:
        parse(f"{second}, bogus,all")  # ("all" is a name only on its own)
    assert str(e.value) == names_error
    with pytest.raises(ValueError) as e:
        parse(all_bits + 1 if all_bits == 1 else 4)  # a stray bit
    assert str(e.value) == int_error
    with pytest.raises(ValueError) as e:
        parse(-1)
    assert str(e.value) == int_error.rsplit("not ", 1)[0] + "not -0x1"


def test_no_addon_translation_unit_carries_its_own_copy_of_the_host_layer():
    csrc = os.path.join(ROOT, "pytracer_amd", "csrc")
    common = open(os.path.join(csrc, "pt_host_common.h")).read()
    assert not re.search(r"__global__|__device__", re.sub(r"//.*", "", common))  # host code only
    for what in (r"thread_local char g_err\[", r"static int fail\(", r"#define HIP_TRY\(", r"static int device_ok\(", r"struct Staged \{",
                 r"static size_t up8\(", r"static dim3 grid_of\(", r"static int check_scene_block\(", r"static int resident_lanes\("):
        assert len(re.findall(what, common)) == 1, what
    for name in ADDONS:
        text = open(os.path.join(csrc, f"ptrace_{name}.hip")).read()
        assert '#include "pt_host_common.h"' in text
        for what in (r"\bg_err\b", r"\bint\s+device_ok\s*\(", r"\bstruct\s+Staged\b", r"\bint\s+fail\s*\(", r"#\s*define\s+HIP_TRY\b",
                     r"\bup8\s*\(size_t", r"\bdim3\s+grid_of\s*\(", r"getenv\s*\(", r"this library's has %zu"):
            assert not re.search(what, text), (name, what)
