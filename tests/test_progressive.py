"""CPU tests of progressive rendering's host side (no GPU needed): the four entry points are declared in the header, exported by both builds
of the library and prototyped in rtamd/abi.py; null handles are refused without a HIP call; the CLI refuses --passes 0."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from rtamd import abi

REPO = Path(__file__).resolve().parent.parent
EXE = REPO / "sycl-ray-tracer_amd" / "host" / "build" / "raytracer"
ENTRY_POINTS = ["rt_renderer_set_progressive", "rt_render_frame_continue", "rt_render_frame_continue_device", "rt_renderer_accumulated_samples"]


def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib):
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rt_mi355x.h").read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"{name} is not declared in include/rt_mi355x.h"
        assert hasattr(rtlib, name) and hasattr(devlib, name), f"{name} is not exported"
        assert name in abi.PROTOTYPES and abi.PROTOTYPES[name][0] is C.c_int


def test_null_handles_are_refused_without_a_device(rtlib):
    n = C.c_uint32(7)
    st = abi.rt_stats()
    assert rtlib.rt_renderer_set_progressive(None, 1) == abi.RT_ERR_INVALID
    assert rtlib.rt_renderer_set_progressive(None, 0) == abi.RT_ERR_INVALID
    assert rtlib.rt_render_frame_continue(None, 4, None, None, C.byref(st)) == abi.RT_ERR_INVALID
    assert rtlib.rt_render_frame_continue_device(None, 4, None, None, None, C.byref(st)) == abi.RT_ERR_INVALID
    assert rtlib.rt_renderer_accumulated_samples(None, C.byref(n)) == abi.RT_ERR_INVALID and n.value == 7
    assert b"null" in rtlib.rt_last_error()


def test_cli_refuses_zero_passes(tmp_path):
    for args, code in ((["--passes", "0"], 105), (["--passes", "x"], 104), (["--passes"], 106)):
        p = subprocess.run([str(EXE), str(REPO / "assets" / "cube.glb")] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == code, (args, p.returncode, p.stdout, p.stderr)
        assert "--passes" in p.stderr
        assert not (tmp_path / "out.png").exists()
    help_text = subprocess.run([str(EXE), "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--passes" in help_text
