"""CPU: the C ABI of the voxel map's observation log (sdm_vmap_observe, sdm_vmap_get_obs_info, sdm_vmap_fetch_observations,
sdm_vmap_fetch_cameras and their four structs) -- declared in the header, exported, laid out in ctypes as the C compiler
lays out include/sdm_c.h, refusing bad arguments without a GPU, and leaving every earlier struct as it was."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from test_extract_abi import ROOT, _c_compiler

STRUCTS = {
    "sdm_vmap_observe_delta": ("VmapObserveDelta", ("plain_total", "unmapped", "candidates", "first_created", "created")),
    "sdm_vmap_observations": ("VmapObservations", ("entry", "tag", "capacity", "on_device")),
    "sdm_vmap_cameras": ("VmapCameras", ("cam_offsets", "cam_tags", "capacity", "cam_capacity", "on_device", "cam_total")),
    "sdm_vmap_obs_info": ("VmapObsInfo", ("observations", "calls", "table_slots", "rehashes")),
}
FUNCTIONS = {
    "sdm_vmap_observe": ["sdm_ctx", "int", "const int", "const int", "int", "const int", "const int", "int", "double", "double",
                         "sdm_vmap_observe_delta"],
    "sdm_vmap_get_obs_info": ["sdm_ctx", "sdm_vmap_obs_info"],
    "sdm_vmap_fetch_observations": ["sdm_ctx", "long long", "long long", "sdm_vmap_observations"],
    "sdm_vmap_fetch_cameras": ["sdm_ctx", "const unsigned", "long long", "long long", "sdm_vmap_cameras"],
}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = {"sdm_vmap_info": ("VmapInfo", 56), "sdm_vmap_delta": ("VmapDelta", 64), "sdm_vmap_fields": ("VmapFields", 24),
             "sdm_vmap_carve_args": ("VmapCarveArgs", 56), "sdm_vmap_evidence": ("VmapEvidence", 32),
             "sdm_point_buffers": ("PointBuffers", 48), "sdm_voxel_buffers": ("VoxelBuffers", 40),
             "sdm_voxel_cameras": ("VoxelCameras", 32), "sdm_voxel_freespace": ("VoxelFreespace", 40)}


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def _argtypes(b):
    C = ctypes
    ip, ctx = C.POINTER(C.c_int), C.c_void_p
    return {
        "sdm_vmap_observe": [ctx, C.c_int, ip, ip, C.c_int, ip, ip, C.c_int, C.c_double, C.c_double, C.POINTER(b.VmapObserveDelta)],
        "sdm_vmap_get_obs_info": [ctx, C.POINTER(b.VmapObsInfo)],
        "sdm_vmap_fetch_observations": [ctx, C.c_longlong, C.c_longlong, C.POINTER(b.VmapObservations)],
        "sdm_vmap_fetch_cameras": [ctx, C.c_void_p, C.c_longlong, C.c_longlong, C.POINTER(b.VmapCameras)],
    }


def test_header_declares_structs_and_functions():
    text = open(os.path.join(ROOT, "include", "sdm_c.h")).read()
    for name in STRUCTS:
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    for name, want in FUNCTIONS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        kinds = [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0].strip() for a in args.split(",")]
        assert kinds == want, (name, kinds)
    # the limits speak of what exists now
    assert "sdm_vmap_carve (below), camera lists on" not in text  # (what is left for later is removal and shrinking)
    assert re.search(r"camera\s+\*?\s*lists by sdm_vmap_observe", text)
    for phrase in ("an observation cannot be removed", "20 B per set slot", "12 B per log entry", "8 B per record of capacity",
                   "never shrink", "2^40"):
        assert phrase in text, phrase


def test_symbols_exported_and_argtypes(pkg):
    b = _binding(pkg)
    raw = ctypes.CDLL(pkg.lib_path())
    syms = {s[0]: s for s in b.SYMBOLS}
    lib = pkg.load_library()
    for name, want in _argtypes(b).items():
        assert hasattr(raw, name), name
        assert syms[name][1] is ctypes.c_int and syms[name][2] == want, name
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want and fn.restype is ctypes.c_int, name
    assert tuple(b.VMAP_OBSERVATION_FIELDS) == ("entry", "tag")
    assert b.VMAP_OBSERVE_OUTS == tuple(f for f, _ in b.VmapObserveDelta._fields_)


def _layout(tmp_path, cname, fields):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdm_c.h"\nint main(void) {\n'
                   '  printf("size %%zu\\n", sizeof(%s));\n' % cname +
                   "".join('  printf("%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));\n' % (f, cname, f, cname, f)
                           for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([_c_compiler(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines if ln.strip()}


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_layout_matches_header(pkg, tmp_path, cname):
    b = _binding(pkg)
    pyname, fields = STRUCTS[cname]
    st = getattr(b, pyname)
    got = _layout(tmp_path, cname, fields)
    assert got["size"] == [ctypes.sizeof(st)]
    assert [f[0] for f in st._fields_] == list(fields)
    for f in fields:
        fd = getattr(st, f)
        assert got[f] == [fd.offset, fd.size], f


@pytest.mark.parametrize("cname", sorted(UNCHANGED))
def test_existing_structs_keep_their_layout(pkg, tmp_path, cname):
    b = _binding(pkg)
    pyname, size = UNCHANGED[cname]
    st = getattr(b, pyname)
    fields = [f[0] for f in st._fields_]
    got = _layout(tmp_path, cname, fields)
    assert got["size"] == [size] == [ctypes.sizeof(st)]
    for f in fields:
        fd = getattr(st, f)
        assert got[f] == [fd.offset, fd.size], f
    # the observation calls exist beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_observe")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    ob, vo, vc, info = b.VmapObserveDelta(), b.VmapObservations(), b.VmapCameras(), b.VmapObsInfo()
    ob.plain_total = ob.unmapped = ob.candidates = ob.first_created = ob.created = 7
    vc.cam_total = 7
    slots = (ctypes.c_int * 1)(0)
    assert lib.sdm_vmap_observe(None, 1, slots, None, 0, None, None, 1, 0.01, 1e-6, ctypes.byref(ob)) == 1
    assert [getattr(ob, f) for f, _ in b.VmapObserveDelta._fields_] == [0] * 5  # the outs of a refusal
    assert lib.sdm_vmap_observe(None, 1, slots, slots, 1, slots, slots, 1, 0.01, 1e-6, None) == 1
    assert lib.sdm_vmap_get_obs_info(None, ctypes.byref(info)) == 1
    assert lib.sdm_vmap_get_obs_info(None, None) == 1
    assert lib.sdm_vmap_fetch_observations(None, 0, 0, ctypes.byref(vo)) == 1
    assert lib.sdm_vmap_fetch_observations(None, 0, 0, None) == 1
    assert lib.sdm_vmap_fetch_cameras(None, None, 0, 0, ctypes.byref(vc)) == 1
    assert vc.cam_total == 0
    assert lib.sdm_vmap_fetch_cameras(None, None, 0, 0, None) == 1
