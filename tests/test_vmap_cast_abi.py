"""CPU: the C ABI of sdm_vmap_cast_segments and sdm_vmap_render and their struct -- declared in the header, exported, laid
out in ctypes as the C compiler lays out include/sdm_c.h, refusing NULL arguments without a GPU, and leaving every earlier
struct as it was."""
import ctypes
import inspect
import os
import re
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_obs_abi import _layout
from test_vmap_recarve_abi import SIZES as RECARVE_SIZES, STRUCTS as RECARVE_STRUCTS, UNCHANGED as EARLIER

STRUCTS = {
    "sdm_vmap_cast_args": ("VmapCastArgs", ("start_margin", "end_margin", "max_steps", "min_multiplicity", "require_published",
                                            "on_device", "capacity", "hit_id", "hit_step", "hit_rho", "rays_total", "rays_skipped",
                                            "rays_hit", "cells_visited")),
}
FUNCTIONS = {
    "sdm_vmap_cast_segments": ["sdm_ctx", "long long", "const float", "const float", "sdm_vmap_cast_args"],
    "sdm_vmap_render": ["sdm_ctx", "const float", "const float", "int", "int", "float", "sdm_vmap_cast_args"],
}
SIZES = {"sdm_vmap_cast_args": 88}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, **{c: (RECARVE_STRUCTS[c][0], RECARVE_SIZES[c]) for c in RECARVE_STRUCTS})


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def test_header_declares_struct_and_functions():
    text = open(os.path.join(ROOT, "include", "sdm_c.h")).read()
    for name in STRUCTS:
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    for name, want in FUNCTIONS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        kinds = [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0].strip() for a in args.split(",")]
        assert kinds == want, (name, kinds)
    assert text.index("int sdm_vmap_recarve") < text.index("int sdm_vmap_cast_segments") < text.index("int sdm_vmap_render") \
        < text.index("int sdm_extract_bound")
    assert re.search(r"#define SDM_VMAP_NO_HIT 0xFFFFFFFFu\b", text) and re.search(r"#define SDM_VMAP_RAY_SKIPPED 0xFFFFFFFEu\b", text)
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("start_margin <= s <= N - end_margin", "end_margin = 0 examines the end cell",
                   "end_margin = m counts the same cells as end_margin = m + 1 here", "is transparent: the ray goes on",
                   "if no classify has run every flag reads 0", "Ids stay below 2^30", "n == 0 is valid",
                   "up to and including the stopping one", "hit_rho = 1.0f / z", "otherwise hit_rho = +0.0f",
                   "The answer is voxel-level", "need not project into that pixel", "A non-finite pose is no error",
                   "neither call changes the map", "whatever the table layout", "before anything is queued",
                   "no destination at all", "a misaligned device pointer", "require_published not 0 or 1",
                   "(double)rho_far < 1e-6", "raised before any launch", "one rank only", "no sub-voxel intersection, no normals",
                   "belongs to the stored point, not to the ray's crossing", "go stale with sdm_set_pose"):
        assert phrase in flat, phrase


def test_symbols_exported_and_argtypes(pkg):
    b = _binding(pkg)
    C = ctypes
    args = C.POINTER(b.VmapCastArgs)
    want = {"sdm_vmap_cast_segments": [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, args],
            "sdm_vmap_render": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_float, args]}
    raw = ctypes.CDLL(pkg.lib_path())
    lib = pkg.load_library()
    for name, types in want.items():
        assert hasattr(raw, name)
        sym = {s[0]: s for s in b.SYMBOLS}[name]
        assert sym[1] is ctypes.c_int and sym[2] == types
        fn = getattr(lib, name)
        assert list(fn.argtypes) == types and fn.restype is ctypes.c_int
    assert b.VMAP_CAST_OUTS == tuple(f for f, _ in b.VmapCastArgs._fields_[10:])
    assert (b.VMAP_NO_HIT, b.VMAP_RAY_SKIPPED) == (0xFFFFFFFF, 0xFFFFFFFE)
    sig = inspect.signature(pkg.Engine.vmap_cast_segments)
    assert list(sig.parameters)[1:9] == ["origins", "ends", "start_margin", "end_margin", "max_steps", "min_multiplicity",
                                         "require_published", "steps"]
    assert [p.default for p in list(sig.parameters.values())[3:9]] == [0, 0, 4096, 0, False, True]
    sig = inspect.signature(pkg.Engine.vmap_render)
    assert list(sig.parameters)[1:6] == ["K", "Tcw", "W", "H", "rho_far"]
    assert [sig.parameters[f].default for f in ("start_margin", "end_margin", "max_steps", "min_multiplicity", "require_published")] \
        == [0, 0, 4096, 0, False]


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_layout_matches_header(pkg, tmp_path, cname):
    b = _binding(pkg)
    pyname, fields = STRUCTS[cname]
    st = getattr(b, pyname)
    got = _layout(tmp_path, cname, fields)
    assert got["size"] == [ctypes.sizeof(st)] == [SIZES[cname]]
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
    # the ray queries exist beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_cast_segments")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    a = b.VmapCastArgs()
    a.start_margin, a.end_margin, a.max_steps, a.min_multiplicity, a.require_published, a.capacity = 1, 2, 4096, 3, 1, 5
    for f in b.VMAP_CAST_OUTS:
        setattr(a, f, 7)
    fp = ctypes.POINTER(ctypes.c_float)
    K, T = (ctypes.c_float * 4)(1, 1, 0, 0), (ctypes.c_float * 12)()
    assert lib.sdm_vmap_cast_segments(None, 0, None, None, ctypes.byref(a)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(a, f) for f in b.VMAP_CAST_OUTS] == [0] * 4  # the outs of a refusal
    assert (a.start_margin, a.end_margin, a.max_steps, a.min_multiplicity, a.require_published, a.capacity) == (1, 2, 4096, 3, 1, 5)
    for f in b.VMAP_CAST_OUTS:
        setattr(a, f, 7)
    assert lib.sdm_vmap_render(None, ctypes.cast(K, fp), ctypes.cast(T, fp), 4, 4, 0.5, ctypes.byref(a)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(a, f) for f in b.VMAP_CAST_OUTS] == [0] * 4
    assert lib.sdm_vmap_cast_segments(None, 0, None, None, None) == 1
    assert lib.sdm_vmap_render(None, None, None, 4, 4, 0.5, None) == 1
