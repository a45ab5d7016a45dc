"""Progressive rendering without a GPU: the C ABI is declared and exported, the existing structs keep their sizes,
argument errors come back before any device is touched, and `rtrace` rejects bad progressive flags up front."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
ENTRY_POINTS = ("rt_accum_create", "rt_accum_destroy", "rt_accum_render", "rt_accum_replicas_done", "rt_accum_estimate",
                "rt_accum_estimate_device", "rt_accum_preview_rgb8", "rt_accum_state_size", "rt_accum_save_state",
                "rt_accum_load_state", "rt_tonemap_rgb8_device")


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    lib = C.CDLL(api.DEVICE_LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert "RT_MI355_ABI_VERSION 2 " in text


def test_existing_struct_sizes_are_unchanged(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "rt_mi355.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(RtNode), sizeof(RtTransform), sizeof(RtMesh), sizeof(RtMaterial), sizeof(RtTexture), sizeof(RtSceneDesc), "
                   "sizeof(RtCameraDesc), sizeof(RtRenderParams), sizeof(RtRenderStats)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [176, 256, 72, 24, 88, 88, 168, 80, 152]
    assert [C.sizeof(s) for s in (api.RtNode, api.RtTransform, api.RtMesh, api.RtMaterial, api.RtTexture, api.RtSceneDesc,
                                  api.RtCameraDesc, api.RtRenderParams, api.RtRenderStats)] == sizes


def test_accum_argument_errors_need_no_device():
    lib = api.load_device_lib()
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4"])
    out = C.c_void_p(1)
    assert lib.rt_accum_create(None, C.byref(hs.camera), C.byref(hs.params), C.byref(out)) == api.RT_E_INVALID
    assert out.value is None
    assert b"NULL" in lib.rt_last_error()
    assert lib.rt_accum_create(None, None, None, None) == api.RT_E_INVALID
    assert lib.rt_accum_render(None, 1, None, None) == api.RT_E_INVALID
    assert lib.rt_accum_replicas_done(None) == 0
    assert lib.rt_accum_state_size(None) == 0
    assert lib.rt_accum_estimate(None, None) == api.RT_E_INVALID
    assert lib.rt_accum_load_state(None, b"RTACCUM\0", 8) == api.RT_E_INVALID
    lib.rt_accum_destroy(None)


@pytest.mark.parametrize("flags, message", [
    (["--progressive=0"], "Progressive pass size must be a positive integer"),
    (["--checkpoint=state.bin"], "--checkpoint requires --progressive"),
    (["--progressive=2", "--time-limit=10"], "--time-limit requires --checkpoint"),
    (["--progressive=2", "--gpus=2"], "cannot be combined with --gpus > 1"),
    (["--progressive=2", "--checkpoint=state.bin", "--time-limit=-1"], "Time limit must be"),
])
def test_rtrace_rejects_bad_progressive_flags_before_touching_a_device(tmp_path, flags, message):
    r = subprocess.run([RTRACE, os.path.join(REPO, "scenes", "cornell"), "-w=16", "-s=4"] + flags, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert message in r.stderr
    assert "Rendering" not in r.stdout  # nothing ran: the flags are checked while the command line is read
    assert not (tmp_path / "state.bin").exists()


def test_host_reports_progressive_flags():
    lib = api.load_host_lib()
    for name, res in (("rth_progressive", C.c_uint32), ("rth_checkpoint", C.c_char_p), ("rth_time_limit", C.c_double)):
        getattr(lib, name).argtypes = [C.c_void_p]
        getattr(lib, name).restype = res
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4", "--progressive=3", "--checkpoint=run.state", "--time-limit=2.5"])
    assert lib.rth_progressive(hs._h) == 3 and lib.rth_checkpoint(hs._h) == b"run.state" and lib.rth_time_limit(hs._h) == 2.5
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4"])
    assert lib.rth_progressive(hs._h) == 0 and lib.rth_checkpoint(hs._h) == b"" and lib.rth_time_limit(hs._h) < 0
