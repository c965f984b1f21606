"""CPU: the C ABI of the merged cloud's free-space counts (sdm_extract_points_voxel_freespace, sdm_voxel_freespace) --
declared in the header, exported, laid out in ctypes as the C compiler lays out include/sdm_c.h, and refusing bad
arguments without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

from test_extract_abi import ROOT, _c_compiler

FIELDS = ("crossings", "end_margin", "max_steps", "rays_total", "rays_skipped", "cells_visited")


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def test_header_declares_struct_and_function():
    text = open(os.path.join(ROOT, "include", "sdm_c.h")).read()
    assert re.search(r"\}\s*sdm_voxel_freespace\s*;", text)
    assert re.search(r"#define\s+SDM_FREESPACE_MAX_STEPS\s+65536\b", text)
    m = re.search(r"int\s+sdm_extract_points_voxel_freespace\s*\(([^;]*)\)\s*;", text)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    kinds = [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0].strip() for a in args.split(",")]
    assert kinds == ["sdm_ctx", "int", "const int", "int", "const int", "int", "double", "double", "float",
                     "sdm_point_buffers", "sdm_voxel_buffers", "sdm_voxel_cameras", "sdm_voxel_freespace", "long long"], kinds


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    raw = ctypes.CDLL(pkg.lib_path())
    assert hasattr(raw, "sdm_extract_points_voxel_freespace")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_extract_points_voxel_freespace"]
    assert sym[1] is ctypes.c_int
    ip = ctypes.POINTER(ctypes.c_int)
    assert sym[2] == [ctypes.c_void_p, ctypes.c_int, ip, ctypes.c_int, ip, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                      ctypes.c_float, ctypes.POINTER(b.PointBuffers), ctypes.POINTER(b.VoxelBuffers),
                      ctypes.POINTER(b.VoxelCameras), ctypes.POINTER(b.VoxelFreespace), ctypes.POINTER(ctypes.c_longlong)]
    fn = pkg.load_library().sdm_extract_points_voxel_freespace
    assert list(fn.argtypes) == sym[2] and fn.restype is ctypes.c_int
    assert hasattr(pkg.Engine, "extract_points_voxel_freespace")


def test_voxel_freespace_layout_matches_header(pkg, tmp_path):
    b = _binding(pkg)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdm_c.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(sdm_voxel_freespace));\n'
                   '  printf("limit %d\\n", SDM_FREESPACE_MAX_STEPS);\n' +
                   "".join('  printf("%s %%zu %%zu\\n", offsetof(sdm_voxel_freespace, %s), sizeof(((sdm_voxel_freespace*)0)->%s));\n'
                           % (f, f, f) for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([_c_compiler(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines if ln.strip()}
    assert got["size"] == [ctypes.sizeof(b.VoxelFreespace)]
    assert got["limit"] == [65536]
    assert [f[0] for f in b.VoxelFreespace._fields_] == list(FIELDS)
    for f in FIELDS:
        fd = getattr(b.VoxelFreespace, f)
        assert got[f] == [fd.offset, fd.size], f


def test_bad_arguments_are_einval(pkg):
    """every refusal that needs no GPU: no context, NULL structs, NULL crossings, a bad end_margin or max_steps -- the three
    outputs of fs and cam_total are zeroed whenever their struct is there"""
    b = _binding(pkg)
    lib = pkg.load_library()
    pb, vb, vc, fs = b.PointBuffers(), b.VoxelBuffers(), b.VoxelCameras(), b.VoxelFreespace()
    offs = (ctypes.c_longlong * 2)()
    slots = (ctypes.c_int * 1)(0)
    nbrs = (ctypes.c_int * 1)(0)
    cross = (ctypes.c_uint * 4)(7, 7, 7, 7)
    fn = lib.sdm_extract_points_voxel_freespace

    def call(ctx=None, cams=vc, free=fs):
        fs.rays_total, fs.rays_skipped, fs.cells_visited, vc.cam_total = 11, 12, 13, 77
        rc = fn(ctx, 1, slots, 1, nbrs, 1, 0.01, 1e-6, 0.02, ctypes.byref(pb), ctypes.byref(vb),
                ctypes.byref(cams) if cams is not None else None, ctypes.byref(free) if free is not None else None, offs)
        return rc

    fs.crossings, fs.end_margin, fs.max_steps = ctypes.addressof(cross), 1, 4096
    assert call() == 1  # no context
    assert (fs.rays_total, fs.rays_skipped, fs.cells_visited, vc.cam_total) == (0, 0, 0, 0)
    assert fn(None, 1, slots, 1, nbrs, 1, 0.01, 1e-6, 0.02, None, None, None, None, None) == 1
    assert call(cams=None) == 1 and (fs.rays_total, fs.rays_skipped, fs.cells_visited) == (0, 0, 0)
    assert call(free=None) == 1 and vc.cam_total == 0
    assert b"null fs" in lib.sdm_last_error()
    fs.crossings = None
    assert call() == 1 and b"crossings" in lib.sdm_last_error()
    fs.crossings = ctypes.addressof(cross)
    for margin, steps, word in ((-1, 4096, b"end_margin"), (1, 0, b"max_steps"), (1, -5, b"max_steps"), (1, 65537, b"max_steps")):
        fs.end_margin, fs.max_steps = margin, steps
        assert call() == 1 and word in lib.sdm_last_error(), (margin, steps)
        assert (fs.rays_total, fs.rays_skipped, fs.cells_visited, vc.cam_total) == (0, 0, 0, 0)
    fs.end_margin, fs.max_steps = 0, 65536  # the limits themselves pass these checks: the refusal is the missing context's
    assert call() == 1 and b"null argument" in lib.sdm_last_error()
    assert list(cross) == [7, 7, 7, 7]
