"""CPU: the C ABI of the merged cloud's camera lists (sdm_extract_points_voxel_cameras, sdm_voxel_cameras) -- declared in
the header, exported, laid out in ctypes as the C compiler lays out include/sdm_c.h, and refusing bad arguments without
a GPU."""
import ctypes
import os
import re
import subprocess
import sys

from test_extract_abi import ROOT, _c_compiler

FIELDS = ("cam_offsets", "cam_slots", "cam_capacity", "cam_total")


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def test_header_declares_struct_and_function():
    text = open(os.path.join(ROOT, "include", "sdm_c.h")).read()
    assert re.search(r"\}\s*sdm_voxel_cameras\s*;", text)
    m = re.search(r"int\s+sdm_extract_points_voxel_cameras\s*\(([^;]*)\)\s*;", text)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    kinds = [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0].strip() for a in args.split(",")]
    assert kinds == ["sdm_ctx", "int", "const int", "int", "const int", "int", "double", "double", "float",
                     "sdm_point_buffers", "sdm_voxel_buffers", "sdm_voxel_cameras", "long long"], kinds


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    raw = ctypes.CDLL(pkg.lib_path())
    assert hasattr(raw, "sdm_extract_points_voxel_cameras")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_extract_points_voxel_cameras"]
    assert sym[1] is ctypes.c_int
    ip = ctypes.POINTER(ctypes.c_int)
    assert sym[2] == [ctypes.c_void_p, ctypes.c_int, ip, ctypes.c_int, ip, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                      ctypes.c_float, ctypes.POINTER(b.PointBuffers), ctypes.POINTER(b.VoxelBuffers),
                      ctypes.POINTER(b.VoxelCameras), ctypes.POINTER(ctypes.c_longlong)]
    fn = pkg.load_library().sdm_extract_points_voxel_cameras
    assert list(fn.argtypes) == sym[2] and fn.restype is ctypes.c_int
    assert hasattr(pkg.Engine, "extract_points_voxel_cameras")


def test_voxel_cameras_layout_matches_header(pkg, tmp_path):
    b = _binding(pkg)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdm_c.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(sdm_voxel_cameras));\n' +
                   "".join('  printf("%s %%zu %%zu\\n", offsetof(sdm_voxel_cameras, %s), sizeof(((sdm_voxel_cameras*)0)->%s));\n'
                           % (f, f, f) for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([_c_compiler(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines if ln.strip()}
    assert got["size"] == [ctypes.sizeof(b.VoxelCameras)]
    assert [f[0] for f in b.VoxelCameras._fields_] == list(FIELDS)
    for f in FIELDS:
        fd = getattr(b.VoxelCameras, f)
        assert got[f] == [fd.offset, fd.size], f


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    pb, vb, vc = b.PointBuffers(), b.VoxelBuffers(), b.VoxelCameras()
    offs = (ctypes.c_longlong * 2)()
    slots = (ctypes.c_int * 1)(0)
    nbrs = (ctypes.c_int * 1)(0)
    fn = lib.sdm_extract_points_voxel_cameras
    full = [None, 1, slots, 1, nbrs, 1, 0.01, 1e-6, 0.02, ctypes.byref(pb), ctypes.byref(vb), ctypes.byref(vc), offs]
    assert fn(*full) == 1  # no context
    assert fn(None, 1, slots, 1, nbrs, 1, 0.01, 1e-6, 0.02, None, None, None, None) == 1
    vc.cam_total = 77
    assert fn(*full) == 1 and vc.cam_total == 0
    full[11] = None  # no cams
    assert fn(*full) == 1
